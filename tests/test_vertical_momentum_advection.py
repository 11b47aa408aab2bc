"""Vertical advection of horizontal momentum, `Grid.vertical_momentum_advection`, on CPU.

The one-pass path runs through the `host_abi` fixture (the product's `xgcm_amd.device` over libxgcm_host.so); the chain it
replaces

    wu = grid.interp(w, X);  wv = grid.interp(w, Y);  du = grid.diff(u, Z);  dv = grid.diff(v, Z)
    gu = -grid.interp(wu * du, Z) [/ metric];  gv = -grid.interp(wv * dv, Z) [/ metric]

runs through the same Grid over the oracle double, installed AFTER the one-pass calls of a test have run (the double
replaces `asdevice`, which the one-pass entry needs as the product's own).  Values are compared bit for bit (NaN = NaN), with
dims, coords and names.  `_want` states the same chain a third time, over plain numpy arrays with the oracle's one-axis
functions.  The fallbacks only call existing device functions and run under the `backend` double.  The direct-ABI cases
(`abi_layout_cases`) are shared with the GPU suite."""

import itertools

import numpy as np
import pytest
import torch

import test_vertical_velocity as TV
from oracle import refimpl as R
from test_fused_layouts import ALIGNED, _contig, _strided
from xgcm_amd import DataArray, Dataset, Grid, _hip
from xgcm_amd.chunked import BlockArray

BCS = ["periodic", "fill", "extend"]
FILL = {"X": 1.75, "Y": -0.625, "Z": 0.375}
FILLS = [FILL, {"X": -0.0, "Y": float("nan"), "Z": -0.0}, {"X": float("nan"), "Y": -0.0, "Z": float("nan")}]
AXES = {"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"}, "Z": {"center": "ZC", "left": "ZL"}}
_same_labelled = TV._same_labelled


def _grid(lead, nz, ny, nx, dtype, padding, metric="drF", axes=AXES, mdtype=None):
    """C-grid with a Z axis.  Z metric: drF(ZC), or thicknesses registered at u's and v's points ("full": (Z, Y, X); "lead":
    with the first leading dim in front); None: no Z metric at all"""
    dims = ("time", "member")[:len(lead)]
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0),
              "YC": ("YC", np.arange(ny) + 0.5), "YG": ("YG", np.arange(ny) * 1.0),
              "ZC": ("ZC", np.arange(nz) + 0.5), "ZL": ("ZL", np.arange(nz) * 1.0)}
    for d, n in zip(dims, lead):
        coords[d] = (d, np.arange(n) * 2.0)
    m = lambda shape, seed: R.synthetic_metric(shape, seed).astype(mdtype or dtype)  # noqa: E731
    data, metrics = {}, {}
    if metric == "drF":
        data["drF"] = (("ZC",), m((nz,), 63))
        metrics = {("Z",): ["drF"]}
    elif metric is not None:
        pl, pd = ((lead[0],), dims[:1]) if metric == "lead" else ((), ())
        data["hFacW"] = (pd + ("ZC", "YC", "XG"), m(pl + (nz, ny, nx), 64))
        data["hFacS"] = (pd + ("ZC", "YG", "XC"), m(pl + (nz, ny, nx), 65))
        metrics = {("Z",): ["hFacW", "hFacS"]}
    ds = Dataset(data, coords)
    grid = Grid(ds, coords=axes, metrics=metrics, padding=padding, autoparse_metadata=False)
    return grid, ds, dims


def _fields(lead, nz, ny, nx, dtype, dims, nan=False, seed=71):
    shape = tuple(lead) + (nz, ny, nx)
    u, v, w = (R.synthetic_field(shape, seed + k).astype(dtype) for k in range(3))
    if nan:
        w.reshape(-1)[3::11] = np.nan
        u.reshape(-1)[5::13] = np.nan
        w[..., :, ny // 2, nx // 2] = np.nan   # a column of w that is all NaN
        v[..., 0, 0, 0] = np.nan               # a NaN in level 0, beside the Z pad
        v[..., nz - 1, ny - 1, nx - 1] = np.nan
    return (DataArray(u, dims + ("ZC", "YC", "XG"), name="u"), DataArray(v, dims + ("ZC", "YG", "XC"), name="v"),
            DataArray(w, dims + ("ZL", "YC", "XC"), name="w"))


def _chain(grid, u, v, w, x_axis="X", y_axis="Y", z_axis="Z", padding=None, fill_value=None, metric_weighted=True):
    kw = dict(padding=padding, fill_value=fill_value)
    wu = grid.interp(w, x_axis, **kw)
    wv = grid.interp(w, y_axis, **kw)
    du = grid.diff(u, z_axis, **kw)
    dv = grid.diff(v, z_axis, **kw)
    gu = -grid.interp(wu * du, z_axis, **kw)
    gv = -grid.interp(wv * dv, z_axis, **kw)
    if metric_weighted:
        gu = gu / grid.get_metric(gu, (z_axis,))
        gv = gv / grid.get_metric(gv, (z_axis,))
    return gu, gv


def _want(u, v, w, px, py, pz, fill=FILL, mu=None, mv=None):
    """the chain over plain numpy arrays, from the oracle's one-axis functions (the metrics broadcast against the fields)"""
    z, y, x = u.ndim - 3, u.ndim - 2, u.ndim - 1
    wu = R.stencil1d("interp", w, x, 1, 0, px, fill["X"])
    wv = R.stencil1d("interp", w, y, 1, 0, py, fill["Y"])
    du = R.stencil1d("diff", u, z, 1, 0, pz, fill["Z"])
    dv = R.stencil1d("diff", v, z, 1, 0, pz, fill["Z"])
    gu = -R.stencil1d("interp", R.binary("mul", wu, du), z, 0, 1, pz, fill["Z"])
    gv = -R.stencil1d("interp", R.binary("mul", wv, dv), z, 0, 1, pz, fill["Z"])
    if mu is not None:
        gu = R.binary("div", gu, mu)
    if mv is not None:
        gv = R.binary("div", gv, mv)
    return gu, gv


def _metrics_of(ds, metric, lead=()):
    """the two metrics of `_grid` as numpy arrays that broadcast against (lead, Z, Y, X)"""
    if metric == "drF":
        m = np.asarray(ds["drF"].values)[:, None, None]
        return m, m
    mu, mv = np.asarray(ds["hFacW"].values), np.asarray(ds["hFacS"].values)
    if metric == "lead" and len(lead) > 1:
        mu, mv = (a.reshape(a.shape[:1] + (1,) * (len(lead) - 1) + a.shape[1:]) for a in (mu, mv))
    return mu, mv


def _compare_with_chain(monkeypatch, cases):
    """cases: (grid, (u, v, w), kwargs); every one-pass call first, then the chain over the oracle double"""
    from oracle import fake_device

    got = [grid.vertical_momentum_advection(*f, **kw) for grid, f, kw in cases]
    fake_device.install(monkeypatch)
    for (grid, f, kw), g in zip(cases, got):
        want = _chain(grid, *f, **kw)
        assert len(g) == 2
        for a, w in zip(g, want):
            _same_labelled(a, w)


def _same_bits(got, want):
    """NaN where the other is NaN; everywhere else the same bit pattern, so that -0.0 is not +0.0"""
    g, w = np.asarray(got), np.asarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan)
    bits = {4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
    assert np.array_equal(np.where(nan, 0, g).view(bits), np.where(nan, 0, w).view(bits))


NEG0 = {"X": -0.0, "Y": -0.0, "Z": -0.0}


def signed_zero_cases(dtype):
    """(grid, (u, v, w), kwargs, (px, py, pz)) whose results are full of exact zeros of both signs: u = v = 0 under a
    negative w (every product is -0.0 or, past a -0.0 pad, a sum of signed zeros), u = v = 0 under a w of both signs, and
    a w of zeros of both signs over random u, v -- under every boundary triple, with -0.0 and with None fills"""
    out = []
    for n, (px, py, pz) in enumerate(PADS3):
        grid, ds, dims = _grid((2,), 3, 4, 6, dtype, {"X": px, "Y": py, "Z": pz})
        u, v, w = _fields((2,), 3, 4, 6, dtype, dims)
        zu, zv = u._replace(data=np.zeros(u.shape, dtype)), v._replace(data=np.zeros(v.shape, dtype))
        nw = w._replace(data=-np.abs(w.values) - dtype(0.25))
        sw = w._replace(data=np.where(w.values > 0, dtype(0.0), dtype(-0.0)).astype(dtype))
        nzu = u._replace(data=-np.zeros(u.shape, dtype))   # u of -0.0: its differences are +0.0
        fields = [(zu, zv, nw), (zu, zv, w), (u, v, sw), (nzu, zv, nw)][n % 4]
        for fill in (NEG0, None, {"X": 0.0, "Y": -0.0, "Z": 0.0}):
            out.append((grid, fields, dict(fill_value=fill, metric_weighted=bool(n % 2)), (px, py, pz)))
    return out


# (lead, nz, ny, nx, metric form): the four lead / metric cases of the boundary matrix
LEAD_CASES = [((), 4, 5, 8, "drF"), ((2,), 3, 5, 6, "full"), ((2, 2), 3, 4, 5, "lead"), ((3,), 5, 3, 12, "lead")]


# ---- 1. the one-pass result equals the chain ------------------------------------------------------------------------------
@pytest.mark.parametrize("px,py,pz", list(itertools.product(BCS, BCS, BCS)))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("weighted", [True, False])
def test_equals_the_chain(host_abi, monkeypatch, px, py, pz, dtype, weighted):
    pad = {"X": px, "Y": py, "Z": pz}
    cases = []
    for n, (lead, nz, ny, nx, metric) in enumerate(LEAD_CASES):
        grid, ds, dims = _grid(lead, nz, ny, nx, dtype, pad, metric=metric)
        for nan in (False, True):
            f = _fields(lead, nz, ny, nx, dtype, dims, nan=nan)
            cases.append((grid, f, dict(fill_value=FILLS[(n + nan) % 3], metric_weighted=weighted)))
    _compare_with_chain(monkeypatch, cases)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_signed_zeros_and_negative_zero_fills_keep_their_sign(host_abi, monkeypatch, dtype):
    """bit patterns, not values: a -0.0 fill is handed on as -0.0 on every axis, as the chain's one-axis operators do"""
    from oracle import fake_device

    cases = signed_zero_cases(dtype)
    got = [grid.vertical_momentum_advection(*f, **kw) for grid, f, kw, _ in cases]
    fake_device.install(monkeypatch)
    zeros = negative = 0
    for (grid, f, kw, (px, py, pz)), g in zip(cases, got):
        want = _chain(grid, *f, **kw)
        fill = kw["fill_value"] or {"X": 0.0, "Y": 0.0, "Z": 0.0}
        m = np.asarray(grid._ds["drF"].values)[:, None, None] if kw["metric_weighted"] else None
        plain = _want(*(a.values for a in f), px, py, pz, fill=fill, mu=m, mv=m)
        for a, w, pw in zip(g, want, plain):
            _same_bits(a.values, w.values)
            _same_bits(a.values, pw)
            zeros += int((a.values == 0).sum())
            negative += int(((a.values == 0) & np.signbit(a.values)).sum())
    assert 0 < negative < zeros   # the cases do hold zeros of both signs


def test_a_negative_zero_fill_reaches_the_last_level_as_the_chain_has_it(host_abi):
    """u = v = 0 under w < 0, `fill` on every axis with -0.0: every product is -0.0, the mean with the -0.0 pad beyond the
    last level is -0.0 and its negation +0.0 (a +0.0 pad would give -(-0.0 + 0.0) / 2 = -0.0)"""
    grid, ds, dims = _grid((), 3, 4, 6, np.float64, {"X": "fill", "Y": "fill", "Z": "fill"})
    u, v, w = _fields((), 3, 4, 6, np.float64, dims)
    zu, zv = u._replace(data=np.zeros(u.shape)), v._replace(data=np.zeros(v.shape))
    nw = w._replace(data=-np.abs(w.values) - 0.25)
    for g in grid.vertical_momentum_advection(zu, zv, nw, fill_value=NEG0, metric_weighted=False):
        assert (g.values == 0).all() and not np.signbit(g.values).any()
    for g in grid.vertical_momentum_advection(zu, zv, nw, fill_value=0.0, metric_weighted=False):
        assert (g.values == 0).all() and np.signbit(g.values[-1]).all()


def test_xarray_in_xarray_out(host_abi, monkeypatch):
    import xarray_standin
    from oracle import fake_device

    xarray_standin.install(monkeypatch)
    import xarray as xr

    grid, ds, dims = _grid((), 3, 4, 6, np.float64, {"X": "periodic", "Y": "fill", "Z": "extend"})
    f = _fields((), 3, 4, 6, np.float64, dims)
    got = grid.vertical_momentum_advection(*(xr.DataArray(a.values, dims=a.dims, name=a.name) for a in f), fill_value=FILL)
    assert all(type(g).__module__.split(".")[0] == "xarray" for g in got)
    fake_device.install(monkeypatch)
    for g, w in zip(got, _chain(grid, *f, fill_value=FILL)):
        assert tuple(g.dims) == tuple(w.dims) and g.name == w.name
        assert np.array_equal(np.asarray(g.values), np.asarray(w.values))


def test_coords_and_names_follow_the_chain(host_abi, monkeypatch):
    cases = []
    for names in (("u", "v", "w"), ("q", "q", "q"), ("drF", "drF", "drF"), (None, "v", None)):
        for metric in ("drF", "full"):
            grid, ds, dims = _grid((2,), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"}, metric=metric)
            f = [a._replace(name=n) for a, n in zip(_fields((2,), 3, 5, 6, np.float64, dims), names)]
            f[0] = f[0].assign_coords({"lonW": (("YC", "XG"), np.ones((5, 6))), "t2": (("time",), np.arange(2) + 7.0)})
            f[2] = f[2].assign_coords({"depth": (("ZL",), np.arange(3) * 10.0), "t2": (("time",), np.arange(2) + 9.0),
                                       "lonC": (("YC", "XC"), np.ones((5, 6)))})
            cases += [(grid, tuple(f), dict(fill_value=FILL, metric_weighted=mw)) for mw in (True, False)]
    _compare_with_chain(monkeypatch, cases)


def test_the_fused_entry_runs_alone(host_abi, monkeypatch):
    """one call of the one-pass device entry and none of the chain's operators"""
    import xgcm_amd.device as D

    grid, ds, dims = _grid((2,), 3, 5, 6, np.float64, {"X": "periodic", "Y": "fill", "Z": "extend"})
    f = _fields((2,), 3, 5, 6, np.float64, dims)
    calls = {"fused": 0, "chain": 0}

    def counted(fn, key):
        def wrapped(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(D, "vertical_momentum_advection", counted(D.vertical_momentum_advection, "fused"))
    for name in ("binary", "stencil1d"):
        monkeypatch.setattr(D, name, counted(getattr(D, name), "chain"))
    gu, gv = grid.vertical_momentum_advection(*f, fill_value=FILL)
    wu, wv = _want(*(a.values for a in f), "periodic", "fill", "extend", mu=ds["drF"].values[:, None, None],
                   mv=ds["drF"].values[:, None, None])
    assert np.array_equal(gu.values, wu) and np.array_equal(gv.values, wv)
    assert gu.dims == ("time", "ZC", "YC", "XG") and gv.dims == ("time", "ZC", "YG", "XC")
    assert calls == {"fused": 1, "chain": 0}


# ---- 2. the smallest shapes at which it can go wrong ----------------------------------------------------------------------
NZS, NYS, NXS = [1, 2, 3, 5], [1, 2, 3, 9], [1, 2, 3, 8, 129, 130, 257]
PADS3 = list(itertools.product(BCS, BCS, BCS))
METRICS = ["drF", "full"]


def shape_table(nx):
    """(nz, ny, nx, (px, py, pz), dtype, metric form, metric_weighted): every nz and ny with this nx -- one level (both Z pads
    touch the same cell), one row (the halo row is the pad), nx across one wave, odd nx (the narrow form) -- the boundaries,
    the dtype and the metric forms rotating so that the table as a whole meets every combination several times"""
    out = []
    for n, (nz, ny) in enumerate(itertools.product(NZS, NYS)):
        k = n + 5 * NXS.index(nx)
        out.append((nz, ny, nx, PADS3[(7 * k) % len(PADS3)], (np.float64, np.float32)[(k // 2) % 2], METRICS[k % 2],
                    bool((k // 3) % 2)))
    return out


def test_the_shape_table_meets_every_boundary_triple():
    seen = {pads for nx in NXS for *_, pads, _, _, _ in shape_table(nx)}
    assert seen == set(PADS3)


@pytest.mark.parametrize("nx", NXS)
def test_small_shapes(host_abi, monkeypatch, nx):
    import xgcm_amd.device as D

    calls = []
    real = D.vertical_momentum_advection
    monkeypatch.setattr(D, "vertical_momentum_advection", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    cases = []
    for nz, ny, nx_, (px, py, pz), dtype, metric, mw in shape_table(nx):
        grid, ds, dims = _grid((), nz, ny, nx_, dtype, {"X": px, "Y": py, "Z": pz}, metric=metric)
        f = _fields((), nz, ny, nx_, dtype, dims, nan=(nz + ny) % 2 == 0)
        cases.append((grid, f, dict(fill_value=FILL, metric_weighted=mw)))
    _compare_with_chain(monkeypatch, cases)
    assert len(calls) == len(cases) == len(NZS) * len(NYS)


# ---- 3. the chain stated independently, over plain numpy arrays -----------------------------------------------------------
@pytest.mark.parametrize("case", range(6))
def test_equals_the_numpy_statement(host_abi, case):
    lead, nz, ny, nx, metric = (LEAD_CASES + [((), 1, 1, 3, "drF"), ((2,), 2, 9, 130, "full")])[case]
    px, py, pz = PADS3[(5 * case + 3) % 27]
    for dtype in (np.float64, np.float32):
        grid, ds, dims = _grid(lead, nz, ny, nx, dtype, {"X": px, "Y": py, "Z": pz}, metric=metric)
        f = _fields(lead, nz, ny, nx, dtype, dims, nan=bool(case % 2))
        for mw in (True, False):
            got = grid.vertical_momentum_advection(*f, fill_value=FILL, metric_weighted=mw)
            mu, mv = _metrics_of(ds, metric, lead) if mw else (None, None)
            for g, w in zip(got, _want(*(a.values for a in f), px, py, pz, mu=mu, mv=mv)):
                assert g.values.dtype == w.dtype == np.dtype(dtype) and np.array_equal(g.values, w, equal_nan=True)


# ---- 4. NaN and Inf -------------------------------------------------------------------------------------------------------
def test_a_nan_in_w_poisons_exactly_its_stencil(host_abi):
    """w[k, j, i] enters wu at columns i and i + 1 and wv at rows j and j + 1, the product of level k, and through it the
    means of levels k - 1 and k: exactly those cells, wrapped under periodic boundaries"""
    nz, ny, nx, (k, j, i) = 5, 6, 8, (0, 5, 7)
    grid, ds, dims = _grid((), nz, ny, nx, np.float64, {"X": "periodic", "Y": "periodic", "Z": "periodic"})
    u, v, w = _fields((), nz, ny, nx, np.float64, dims)
    w.values[k, j, i] = np.nan
    gu, gv = grid.vertical_momentum_advection(u, v, w, fill_value=FILL)
    mask_u, mask_v = np.zeros((nz, ny, nx), bool), np.zeros((nz, ny, nx), bool)
    for kk in ((k - 1) % nz, k):
        mask_u[kk, j, [i, (i + 1) % nx]] = True
        mask_v[kk, [j, (j + 1) % ny], i] = True
    assert np.array_equal(np.isnan(gu.values), mask_u) and np.array_equal(np.isnan(gv.values), mask_v)


def test_all_nan_column_and_inf_times_zero(host_abi, monkeypatch):
    """an all-NaN column of w, and an infinite w over a cell where u does not change along Z: Inf * 0 = NaN, as in the chain"""
    nz, ny, nx = 4, 5, 7
    cases, masks = [], []
    for pz in BCS:
        grid, ds, dims = _grid((2,), nz, ny, nx, np.float64, {"X": "extend", "Y": "fill", "Z": pz})
        u, v, w = _fields((2,), nz, ny, nx, np.float64, dims)
        w.values[:, :, 2, 3] = np.nan
        w.values[:, 2, 4, 1] = np.inf
        u.values[:, 2, 4, 1] = u.values[:, 1, 4, 1]   # du[2] == 0 below an infinite wu
        v.values[:, :, 0, 5] = 0.25                   # dv == 0 in a whole column (not across a fill pad)
        w.values[:, 1, 0, 5] = -np.inf
        cases.append((grid, (u, v, w), dict(fill_value=FILL)))
        masks.append((u, v, w, pz, ds))
    got = [grid.vertical_momentum_advection(*f, **kw) for grid, f, kw in cases]
    for (gu, gv), (u, v, w, pz, ds) in zip(got, masks):
        m = ds["drF"].values[:, None, None]
        wu, wv = _want(u.values, v.values, w.values, "extend", "fill", pz, mu=m, mv=m)
        assert np.array_equal(gu.values, wu, equal_nan=True) and np.array_equal(gv.values, wv, equal_nan=True)
        assert np.isnan(gu.values[:, :, 2, 3]).all() and np.isnan(gu.values[:, :, 2, 4]).all()
        assert np.isnan(gu.values[:, 1:3, 4, 1]).all()            # Inf * 0 at level 2 reaches the means of levels 1 and 2
        assert np.isnan(gv.values[:, 0:2, 0, 5]).all()            # -Inf * 0 at level 1
        assert np.isfinite(gu.values[:, :, 0, 0]).all()
    _compare_with_chain(monkeypatch, cases)


# ---- 5. composition with vertical_velocity --------------------------------------------------------------------------------
def test_w_from_vertical_velocity_goes_straight_in(host_abi, monkeypatch):
    import xgcm_amd.device as D

    calls = []
    real = D.vertical_momentum_advection
    monkeypatch.setattr(D, "vertical_momentum_advection", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    cases = []
    for dtype in (np.float64, np.float32):
        grid, ds, dims = _grid((2,), 4, 5, 8, dtype, {"X": "periodic", "Y": "periodic", "Z": "extend"})
        u, v, _ = _fields((2,), 4, 5, 8, dtype, dims)
        w = grid.vertical_velocity(u, v, metric_weighted=False)
        assert w.dims == ("time", "ZL", "YC", "XC")
        cases.append((grid, (u, v, w), dict(fill_value=FILL)))
        # constant u and v: no shear, so under `extend` on Z (no jump at the pad either) the tendencies vanish exactly
        cu, cv = u._replace(data=np.full(u.shape, 0.75, dtype)), v._replace(data=np.full(v.shape, -1.5, dtype))
        for mw in (True, False):
            gu, gv = grid.vertical_momentum_advection(cu, cv, w, metric_weighted=mw)
            assert (gu.values == 0).all() and (gv.values == 0).all()
    assert len(calls) == 4
    _compare_with_chain(monkeypatch, cases)
    assert len(calls) == 6


# ---- 6. every fallback of the docstring takes the chain -------------------------------------------------------------------
def _no_fused(monkeypatch):
    import xgcm_amd.device as D

    monkeypatch.setattr(D, "vertical_momentum_advection", lambda *a, **k: pytest.fail("one-pass entry called"))


def _fallback_equals_chain(grid, f, **kw):
    got, want = grid.vertical_momentum_advection(*f, **kw), _chain(grid, *f, **kw)
    assert len(got) == 2
    for g, w in zip(got, want):
        _same_labelled(g, w)


def _same_error(fused, chain):
    with pytest.raises(Exception) as fused_err:
        fused()
    with pytest.raises(Exception) as chain_err:
        chain()
    assert type(fused_err.value) is type(chain_err.value) and str(fused_err.value) == str(chain_err.value)
    assert not isinstance(fused_err.value, (AttributeError, NotImplementedError))


@pytest.mark.parametrize("dtype", [np.int64, np.int32, np.float16])
def test_integer_and_half_fields_run_the_chain(backend, monkeypatch, dtype):
    _no_fused(monkeypatch)
    grid, ds, dims = _grid((), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    f = tuple(DataArray((a.values * 100).astype(dtype), a.dims, name=a.name) for a in _fields((), 3, 5, 6, np.float64, dims))
    for kw in (dict(), dict(metric_weighted=False, fill_value=FILL)):
        _fallback_equals_chain(grid, f, **kw)


def test_mixed_dtypes_run_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, dims = _grid((), 3, 5, 6, np.float32, {"X": "fill", "Y": "periodic", "Z": "extend"}, mdtype=np.float64)
    f = _fields((), 3, 5, 6, np.float32, dims)
    _fallback_equals_chain(grid, f, fill_value=FILL)   # float32 fields over float64 metrics; without them: a float64 w
    u, v, w = f
    _fallback_equals_chain(grid, (u, v, w._replace(data=w.values.astype(np.float64))), fill_value=FILL, metric_weighted=False)


def test_permuted_dims_run_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, dims = _grid((2,), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    u, v, w = _fields((2,), 3, 5, 6, np.float64, dims)
    _fallback_equals_chain(grid, (u.transpose("ZC", "time", "YC", "XG"), v, w), fill_value=FILL)
    _fallback_equals_chain(grid, (u, v, w.transpose("time", "YC", "ZL", "XC")), fill_value=FILL, metric_weighted=False)


def test_fields_of_different_shapes_run_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, dims = _grid((2,), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    u, v, w = _fields((2,), 3, 5, 6, np.float64, dims)
    w0 = DataArray(np.ascontiguousarray(w.values[0]), w.dims[1:], name="w")   # w without the leading dim: it broadcasts
    _fallback_equals_chain(grid, (u, v, w0), fill_value=FILL)


def test_chunked_input_runs_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, dims = _grid((4,), 3, 6, 8, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    u, v, w = _fields((4,), 3, 6, 8, np.float64, dims)
    cw = DataArray(BlockArray.from_array(w.values, ((2, 2), (3,), (6,), (8,))), w.dims, name="w")
    got = grid.vertical_momentum_advection(u, v, cw, fill_value=FILL)
    want = _chain(grid, u, v, cw, fill_value=FILL)
    m = ds["drF"].values[:, None, None]
    plain = _want(u.values, v.values, w.values, "periodic", "extend", "fill", mu=m, mv=m)
    for g, w_, pw in zip(got, want, plain):
        assert g.dims == w_.dims and g.name == w_.name
        assert np.array_equal(np.asarray(g.values), np.asarray(w_.values)) and np.array_equal(np.asarray(g.values), pw)


def test_a_metric_with_an_extra_dim_runs_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, dims = _grid((), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    coords = {k: (k, np.asarray(ds.coords[k].values)) for k in ("XC", "XG", "YC", "YG", "ZC", "ZL")}
    coords["time"] = ("time", np.arange(2) * 2.0)
    ds2 = Dataset({"drF": (("ZC", "time"), R.synthetic_metric((3, 2), 66))}, coords)
    g2 = Grid(ds2, coords=AXES, metrics={("Z",): ["drF"]}, padding={"X": "periodic", "Y": "extend", "Z": "fill"},
              autoparse_metadata=False)
    f = _fields((), 3, 5, 6, np.float64, ())
    got, want = g2.vertical_momentum_advection(*f, fill_value=FILL), _chain(g2, *f, fill_value=FILL)
    for g, w in zip(got, want):
        assert "time" in g.dims
        _same_labelled(g, w)


def test_a_chunked_metric_runs_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, dims = _grid((), 4, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"}, metric="full")
    coords = {k: (k, np.asarray(ds.coords[k].values)) for k in ("XC", "XG", "YC", "YG", "ZC", "ZL")}
    chunks = ((2, 2), (5,), (6,))
    ds2 = Dataset({k: (ds[k].dims, BlockArray.from_array(np.asarray(ds[k].values), chunks)) for k in ("hFacW", "hFacS")}, coords)
    g2 = Grid(ds2, coords=AXES, metrics={("Z",): ["hFacW", "hFacS"]}, padding={"X": "periodic", "Y": "extend", "Z": "fill"},
              autoparse_metadata=False)
    f = _fields((), 4, 5, 6, np.float64, ())
    got, want = g2.vertical_momentum_advection(*f, fill_value=FILL), _chain(g2, *f, fill_value=FILL)
    plain = _want(*(a.values for a in f), "periodic", "extend", "fill", mu=ds["hFacW"].values, mv=ds["hFacS"].values)
    for g, w, pw in zip(got, want, plain):
        assert g.dims == w.dims and g.name == w.name
        assert np.array_equal(np.asarray(g.values), np.asarray(w.values)) and np.array_equal(np.asarray(g.values), pw)


def test_a_missing_metric_raises_the_chains_error(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, dims = _grid((), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"}, metric=None)
    f = _fields((), 3, 5, 6, np.float64, dims)
    _same_error(lambda: grid.vertical_momentum_advection(*f), lambda: _chain(grid, *f))


def test_a_missing_metric_is_still_served_unweighted(host_abi, monkeypatch):
    import xgcm_amd.device as D

    calls = []
    real = D.vertical_momentum_advection
    monkeypatch.setattr(D, "vertical_momentum_advection", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    grid, ds, dims = _grid((), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"}, metric=None)
    _compare_with_chain(monkeypatch, [(grid, _fields((), 3, 5, 6, np.float64, dims), dict(metric_weighted=False))])
    assert len(calls) == 1


def test_missing_z_boundary_raises_the_chains_error(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, dims = _grid((), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend"})
    f = _fields((), 3, 5, 6, np.float64, dims)
    _same_error(lambda: grid.vertical_momentum_advection(*f), lambda: _chain(grid, *f))


def test_connected_faces_run_the_chain(backend, monkeypatch):
    from test_topology import COORDS, X_TO_X

    _no_fused(monkeypatch)
    ds = Dataset({"drF": (("zc",), R.synthetic_metric((3,), 63))},
                 coords={"x": np.arange(4), "xl": np.arange(4) - 0.5, "y": np.arange(4), "yl": np.arange(4) - 0.5,
                         "face": np.arange(2), "zc": np.arange(3) + 0.5, "zl": np.arange(3) * 1.0})
    grid = Grid(ds, coords=dict(COORDS, Z={"center": "zc", "left": "zl"}), face_connections=X_TO_X,
                metrics={("Z",): ["drF"]}, padding={"X": "fill", "Y": "extend", "Z": "fill"}, autoparse_metadata=False)
    xl, yl = COORDS["X"]["left"], COORDS["Y"]["left"]
    xc, yc = COORDS["X"]["center"], COORDS["Y"]["center"]
    assert (xl, yl, xc, yc) == ("xl", "yl", "x", "y")
    u = DataArray(R.synthetic_field((2, 3, 4, 4), 82), ("face", "zc", yc, xl), name="u")
    v = DataArray(R.synthetic_field((2, 3, 4, 4), 83), ("face", "zc", yl, xc), name="v")
    w = DataArray(R.synthetic_field((2, 3, 4, 4), 84), ("face", "zl", yc, xc), name="w")
    for mw in (True, False):
        _fallback_equals_chain(grid, (u, v, w), metric_weighted=mw)


Y_TO_Y = {"face": {0: {"Y": (None, (1, "Y", False))}, 1: {"Y": ((0, "Y", False), None)}}}
Z_TO_Z = {"face": {0: {"Z": (None, (1, "Z", False))}, 1: {"Z": ((0, "Z", False), None)}}}


@pytest.mark.parametrize("conn", [Y_TO_Y, Z_TO_Z], ids=["y2y", "z2z"])
def test_faces_connected_along_y_or_z_run_the_chain(backend, monkeypatch, conn):
    """a link along Z is the `complex_topology(z_axis)` refusal this operator makes itself; X and Y are `_second_order_plan`'s"""
    from test_topology import COORDS

    _no_fused(monkeypatch)
    ds = Dataset({"drF": (("zc",), R.synthetic_metric((4,), 63))},
                 coords={"x": np.arange(4), "xl": np.arange(4) - 0.5, "y": np.arange(4), "yl": np.arange(4) - 0.5,
                         "face": np.arange(2), "zc": np.arange(4) + 0.5, "zl": np.arange(4) * 1.0})
    grid = Grid(ds, coords=dict(COORDS, Z={"center": "zc", "left": "zl"}), face_connections=conn,
                metrics={("Z",): ["drF"]}, padding={"X": "periodic", "Y": "extend", "Z": "fill"}, autoparse_metadata=False)
    f = lambda seed, dims: DataArray(R.synthetic_field((2, 4, 4, 4), seed), dims, name="f")  # noqa: E731
    u, v, w = f(82, ("face", "zc", "y", "xl")), f(83, ("face", "zc", "yl", "x")), f(84, ("face", "zl", "y", "x"))
    for mw in (True, False):
        _fallback_equals_chain(grid, (u, v, w), fill_value=FILL, metric_weighted=mw)


def test_fold_grid_runs_the_chain(backend, monkeypatch):
    import warnings

    from test_topology import Nx, Ny

    _no_fused(monkeypatch)
    ds = Dataset({"drF": (("zc",), R.synthetic_metric((2,), 63))},
                 coords={"xh": np.arange(Nx), "xl": np.arange(Nx), "yh": np.arange(Ny), "yl": np.arange(Ny),
                         "zc": np.arange(2) + 0.5, "zl": np.arange(2) * 1.0})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        grid = Grid(ds, coords={"X": {"center": "xh", "left": "xl"}, "Y": {"center": "yh", "left": "yl"},
                                "Z": {"center": "zc", "left": "zl"}}, metrics={("Z",): ["drF"]},
                    padding={"X": "periodic", "Y": {"fold": "corner"}, "Z": "extend"}, autoparse_metadata=False)
        f = lambda seed, dims: DataArray(R.synthetic_field((2, Ny, Nx), seed), dims)  # noqa: E731
        u, v, w = f(92, ("zc", "yh", "xl")), f(93, ("zc", "yl", "xh")), f(94, ("zl", "yh", "xh"))
        for mw in (True, False):
            _fallback_equals_chain(grid, (u, v, w), metric_weighted=mw)


# ---- 7. positions the operator does not take ------------------------------------------------------------------------------
def test_misplaced_fields_and_missing_left_positions_raise(backend):
    grid, ds, dims = _grid((), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    u, v, w = _fields((), 3, 5, 6, np.float64, dims)
    with pytest.raises(NotImplementedError, match="X:left"):
        grid.vertical_momentum_advection(DataArray(u.values, ("ZC", "YC", "XC")), v, w)
    with pytest.raises(NotImplementedError, match="Y:left"):
        grid.vertical_momentum_advection(u, DataArray(v.values, ("ZC", "YC", "XC")), w)
    with pytest.raises(NotImplementedError, match="Z:left"):
        grid.vertical_momentum_advection(u, v, DataArray(w.values, ("ZC", "YC", "XC")))
    with pytest.raises(NotImplementedError, match="Z:left"):
        grid.vertical_momentum_advection(w, v, u)
    # an axis without a left position: Z with an outer one (w sits there), X with a right one (u sits there)
    for name, other, n in (("Z", "outer", 4), ("X", "right", 6), ("Y", "right", 5)):
        dim = AXES[name]["left"]
        axes = dict(AXES, **{name: {"center": AXES[name]["center"], other: dim}})
        coords = {k: (k, np.asarray(ds.coords[k].values)) for k in ("XC", "XG", "YC", "YG", "ZC", "ZL") if k != dim}
        coords[dim] = (dim, np.arange(n) * 1.0)
        g2 = Grid(Dataset({"drF": (("ZC",), np.asarray(ds["drF"].values))}, coords), coords=axes, metrics={("Z",): ["drF"]},
                  padding={"X": "periodic", "Y": "extend", "Z": "fill"}, autoparse_metadata=False)
        w2 = DataArray(np.zeros((4, 5, 6)), ("ZL", "YC", "XC")) if name == "Z" else w
        with pytest.raises(NotImplementedError, match="fused vertical momentum advection"):
            g2.vertical_momentum_advection(u, v, w2)


# ---- 8. the entry of the C ABI called directly, with views ----------------------------------------------------------------
NVS = {np.float64: 2, np.float32: 4}
SFX = {np.float64: "f64", np.float32: "f32"}
TORCH = {np.float64: torch.float64, np.float32: torch.float32}
ABI_NX = {np.float64: 132, np.float32: 264}   # one full 64-lane tile and a partial one
ABI_PADS = [("periodic", "extend", "fill"), ("fill", "periodic", "extend"), ("extend", "fill", "periodic")]


def _abi_call(D, dtype, shape, fields, planes, k):
    """one call of xg_vertical_momentum_advection: `fields` (u, v, w) views, `planes` {mu, mv} views or None"""
    px, py, pz = ABI_PADS[k]
    args = [f.data_ptr() for f in fields]
    for name in ("mu", "mv"):
        m = planes.get(name)
        if m is None:
            args += [None, None]
        else:
            assert all(n in (1, s) for n, s in zip(m.shape, shape))
            args += [m.data_ptr(), _hip.i64([0 if n == 1 else m.stride(d) for d, n in enumerate(m.shape)])]
    outs = [D._empty(shape, TORCH[dtype], D._MEM.device) for _ in range(2)]
    args += [o.data_ptr() for o in outs] + [_hip.i64(shape), len(shape), _hip.BC[px], FILL["X"], _hip.BC[py], FILL["Y"],
                                             _hip.BC[pz], FILL["Z"]]
    D._check(getattr(D._MEM.lib(), "xg_vertical_momentum_advection_" + SFX[dtype])(*args, D._stream()))
    return tuple(o.cpu().numpy() for o in outs)


def abi_layout_cases(dtype):
    """Runs the direct-ABI table on whatever library `xgcm_amd.device._MEM` serves.  Every view lives in a NaN-filled
    allocation, so a read outside it shows in the result; the contiguous, aligned control of each set of planes is compared
    with the numpy chain, every other layout with that control."""
    import xgcm_amd.device as D

    nv = NVS[dtype]
    shape = [2, 5, 7, ABI_NX[dtype]]
    lead, nz, ny, nx = shape
    fv = [R.synthetic_field(tuple(shape), 101 + n).astype(dtype) for n in range(3)]
    fv[2].reshape(-1)[5::17] = np.nan
    vals = {"z": R.synthetic_metric((1, nz, 1, 1), 111).astype(dtype), "p": R.synthetic_metric((1, 1, ny, nx), 112).astype(dtype),
            "v3": R.synthetic_metric((1, nz, ny, nx), 113).astype(dtype), "vl": R.synthetic_metric((lead, nz, ny, nx), 114).astype(dtype)}
    put = lambda a, st=None, off=ALIGNED: _strided(D, a, st or _contig(a.shape), off)  # noqa: E731
    for k in range(len(ABI_PADS)):
        px, py, pz = ABI_PADS[k]
        fields = [put(a) for a in fv]
        assert all(f.is_contiguous() and f.data_ptr() % 16 == 0 for f in fields)
        # each metric alone in each form, both together (a Z-only one beside a volume; transposed), none
        for present in ({"mu": "z"}, {"mv": "z"}, {"mu": "p"}, {"mu": "v3"}, {"mv": "vl"}, {"mu": "z", "mv": "v3"},
                        {"mu": "vl", "mv": "p"}, {}):
            pv = {n: vals[form] for n, form in present.items()}
            control = _abi_call(D, dtype, shape, fields, {n: put(a) for n, a in pv.items()}, k)
            want = _want(*fv, px, py, pz, mu=pv.get("mu"), mv=pv.get("mv"))
            for g, w in zip(control, want):
                assert g.dtype == w.dtype == np.dtype(dtype) and np.array_equal(g, w, equal_nan=True), (k, present)
            views = []
            # a misaligned base: each field in turn, then all three, one element into its allocation (the narrow form)
            for moved in ((0,), (1,), (2,), (0, 1, 2)):
                off = [put(a, off=1) if n in moved else fields[n] for n, a in enumerate(fv)]
                assert all(off[n].data_ptr() % 16 == fv[n].dtype.itemsize for n in moved)
                views.append((off, {n: put(a) for n, a in pv.items()}))
            # the planes one element in; with an odd row pitch; with an odd level pitch (volumes)
            views.append((fields, {n: put(a, off=1) for n, a in pv.items()}))
            pitched = {}
            for n, a in pv.items():
                s = list(a.shape)
                st = _contig(s[:-1] + [s[-1] + 1]) if s[-1] > 1 else _contig(s)
                pitched[n] = put(a, st)
                assert s[-1] == 1 or (pitched[n].stride(-2) == nx + 1 and pitched[n].stride(-1) == 1)
            views.append((fields, pitched))
            for n, form in present.items():
                if form in ("v3", "vl"):
                    a = pv[n]
                    st = [(nz * (ny * nx + 1)) * (a.shape[0] > 1), ny * nx + 1, nx, 1]
                    lev = put(a, [s or 1 for s in st])
                    assert lev.stride(1) == ny * nx + 1
                    views.append((fields, dict({m: put(x) for m, x in pv.items()}, **{n: lev})))
                if form == "z":   # the Z-only metric three elements apart
                    views.append((fields, dict({m: put(x) for m, x in pv.items()}, **{n: put(a := pv[n], [3 * nz, 3, 1, 1], 1)})))
                if form == "p":   # the plane stored (X, Y): a transposed view
                    t = put(np.ascontiguousarray(pv[n].transpose(0, 1, 3, 2))).permute(0, 1, 3, 2)
                    assert t.stride(-1) == ny and t.stride(-2) == 1
                    views.append((fields, dict({m: put(x) for m, x in pv.items()}, **{n: t})))
            for fb, planes in views:
                got = _abi_call(D, dtype, shape, fb, planes, k)
                for g, c in zip(got, control):
                    assert np.array_equal(g, c, equal_nan=True), (k, present)
        # a stride-0 metric along X and Y: one value per level, expanded over the whole volume, equals the Z-only metric
        flat = put(vals["z"]).expand(1, nz, ny, nx)
        assert flat.stride(-1) == 0 and flat.stride(-2) == 0
        full = put(np.ascontiguousarray(np.broadcast_to(vals["z"], (1, nz, ny, nx))))
        a = _abi_call(D, dtype, shape, fields, {"mu": flat, "mv": flat}, k)
        c = _abi_call(D, dtype, shape, fields, {"mu": full, "mv": full}, k)
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, c))
    assert nx % nv == 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_abi_layouts(host_abi, dtype):
    abi_layout_cases(dtype)


def test_abi_refuses_bad_calls(host_abi):
    import xgcm_amd.device as D

    lib = D._MEM.lib()
    shape = [2, 3, 4]
    t = torch.zeros(shape, dtype=torch.float64)
    o1, o2 = torch.zeros_like(t), torch.zeros_like(t)

    def call(u=t, ndim=3, bcx=_hip.BC["periodic"], bcy=_hip.BC["extend"], bcz=_hip.BC["fill"], mu=None, mus=None):
        return lib.xg_vertical_momentum_advection_f64(u.data_ptr() if u is not None else None, t.data_ptr(), t.data_ptr(),
                                                      mu, mus, None, None, o1.data_ptr(), o2.data_ptr(), _hip.i64(shape),
                                                      ndim, bcx, 0.0, bcy, 0.0, bcz, 0.0, None)

    assert call() == 0 and call(bcz=_hip.BC["periodic"]) == 0    # every Z boundary is served
    assert call(u=None) == -1                                    # NULL array: XG_ERR_INVALID
    assert call(bcx=7) == -1 and call(bcz=9) == -1               # unknown boundary codes
    assert call(mu=t.data_ptr(), mus=None) == -1                 # a metric without strides
    assert call(ndim=2) < 0 and call(ndim=2) != -1               # XG_ERR_UNSUPPORTED
