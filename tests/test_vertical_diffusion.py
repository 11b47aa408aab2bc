"""Vertical mixing d/dz(kappa da/dz), `Grid.vertical_diffusion`, on CPU.

The one-pass path runs through the `host_abi` fixture (the product's `xgcm_amd.device` over libxgcm_host.so); the chain it
replaces

    g = grid.derivative(a, Z, to=to);  f = g * kappa;  out = grid.derivative(f, Z)        (`diff` when not metric-weighted)

runs through the same Grid over the oracle double, installed AFTER the one-pass calls of a test have run (the double
replaces `asdevice`, which the one-pass entry needs as the product's own).  Values are compared bit for bit (NaN = NaN), with
dims, coords and name.  `_want` states the same chain a third time, over plain numpy arrays with the oracle's one-axis
functions.  A counter on `device.vertical_diffusion` shows that every case meant for the kernel reached it.  The fallbacks
only call existing device functions and run under the `backend` double.  The case tables and the direct-ABI cases
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
TOS = ["left", "outer"]
FILLS = [0.375, -0.0, float("nan")]
AXES = {"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"},
        "Z": {"center": "ZC", "left": "ZL", "outer": "ZO"}}
HPOS = {"c": ("YC", "XC"), "u": ("YC", "XG"), "v": ("YG", "XC")}   # the rows and columns `a` sits on
ZDIM = {"left": "ZL", "outer": "ZO"}
_same_labelled = TV._same_labelled


def _nf(nz, to):
    return nz + (to == "outer")


def _grid(lead, nz, ny, nx, dtype, pz, metric="1d", hpos="c", axes=AXES, mdtype=None):
    """Grid with a Z axis that has a left and an outer position.  Z metrics: "1d" -- drF(ZC), drCl(ZL), drCo(ZO); "full" --
    thicknesses (Z, Y, X) at the rows and columns of `hpos` for all three Z positions; "lead": the same with the first
    leading dim in front; None: no Z metric at all"""
    dims = ("time", "member")[:len(lead)]
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0),
              "YC": ("YC", np.arange(ny) + 0.5), "YG": ("YG", np.arange(ny) * 1.0),
              "ZC": ("ZC", np.arange(nz) + 0.5), "ZL": ("ZL", np.arange(nz) * 1.0), "ZO": ("ZO", np.arange(nz + 1) * 1.0)}
    for d, n in zip(dims, lead):
        coords[d] = (d, np.arange(n) * 2.0)
    m = lambda shape, seed: R.synthetic_metric(shape, seed).astype(mdtype or dtype)  # noqa: E731
    data, metrics = {}, {}
    zs = (("drF", "ZC", nz), ("drCl", "ZL", nz), ("drCo", "ZO", nz + 1))
    if metric == "1d":
        for k, (name, zd, n) in enumerate(zs):
            data[name] = ((zd,), m((n,), 63 + k))
    elif metric is not None:
        pl, pd = ((lead[0],), dims[:1]) if metric == "lead" else ((), ())
        for k, (name, zd, n) in enumerate(zs):
            data[name] = (pd + (zd,) + HPOS[hpos], m(pl + (n, ny, nx), 66 + k))
    if metric is not None:
        metrics = {("Z",): [name for name, _, _ in zs]}
    ds = Dataset(data, coords)
    padding = {"X": "periodic", "Y": "periodic"}
    if pz is not None:
        padding["Z"] = pz
    grid = Grid(ds, coords=axes, metrics=metrics, padding=padding, autoparse_metadata=False)
    return grid, ds, dims


def _field(lead, nz, ny, nx, dtype, dims, hpos="c", nan=False, seed=71):
    a = R.synthetic_field(tuple(lead) + (nz, ny, nx), seed).astype(dtype)
    if nan:
        a.reshape(-1)[3::11] = np.nan
        a[..., :, ny // 2, nx // 2] = np.nan     # a whole column
        a[..., 0, 0, 0] = np.nan                 # level 0, beside the Z pad
        a[..., nz - 1, ny - 1, nx - 1] = np.nan  # the last level, beside the other one
    return DataArray(a, dims + ("ZC",) + HPOS[hpos], name="T")


def _kappa(form, lead, nz, ny, nx, dtype, dims, to, hpos="c", seed=75):
    """kappa at the flux levels: None, a profile ("1d"), a (Z, Y, X) field ("3d") or one with the first leading dim ("lead")"""
    n, zd = _nf(nz, to), ZDIM[to]
    if form is None:
        return None
    if form == "1d":
        return DataArray(R.synthetic_field((n,), seed).astype(dtype), (zd,), name="kappa")
    pl, pd = ((lead[0],), dims[:1]) if form == "lead" and lead else ((), ())
    return DataArray(R.synthetic_field(pl + (n, ny, nx), seed).astype(dtype), pd + (zd,) + HPOS[hpos], name="kappa")


def _chain(grid, a, kappa=None, z_axis="Z", to=None, padding=None, fill_value=None, metric_weighted=True):
    kw = dict(padding=padding, fill_value=fill_value)
    step = grid.derivative if metric_weighted else grid.diff
    if to is None:   # the operator's default: the flux at Z:outer when the axis has that position, else at Z:left
        to = "outer" if "outer" in grid.axes[z_axis].coords else "left"
    g = step(a, z_axis, to=to, **kw)
    f = g if kappa is None else g * kappa
    return step(f, z_axis, **kw)


def _aligned(da, dims):
    """the values of `da` as a numpy array that broadcasts against an array of `dims`"""
    v = np.asarray(da.values)
    present = [d for d in dims if d in da.dims]
    v = np.transpose(v, [da.dims.index(d) for d in present])
    return v[tuple(slice(None) if d in da.dims else np.newaxis for d in dims)]


def _want(a, kappa, mf, mc, to, pz, fill=0.0):
    """the chain over plain numpy arrays, from the oracle's one-axis functions; kappa and the metrics broadcast against the
    flux / the field"""
    z = a.ndim - 3
    outer = to == "outer"
    g = R.stencil1d("diff", a, z, 1, 1 if outer else 0, pz, fill, m_out=mf)
    f = g if kappa is None else R.binary("mul", g, kappa)
    return R.stencil1d("diff", f, z, 0, 0 if outer else 1, pz, fill, m_out=mc)


def _want_of(grid, ds, a, kappa, to, pz, fill, weighted):
    """`_want` for labelled inputs: the metrics are the dataset's own arrays at the flux' and the field's Z position"""
    f_dims = a.dims[:-3] + (ZDIM[to],) + a.dims[-2:]
    mf = _aligned(ds[{"left": "drCl", "outer": "drCo"}[to]], f_dims) if weighted else None
    mc = _aligned(ds["drF"], a.dims) if weighted else None
    k = None if kappa is None else _aligned(kappa, f_dims)
    return _want(a.values, k, mf, mc, to, pz, 0.0 if fill is None else fill)


def _counted(monkeypatch):
    import xgcm_amd.device as D

    calls = []
    real = D.vertical_diffusion
    monkeypatch.setattr(D, "vertical_diffusion", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def _compare_with_chain(monkeypatch, cases):
    """cases: (grid, (a, kappa), kwargs); every one-pass call first (counted), then the chain over the oracle double"""
    from oracle import fake_device

    calls = _counted(monkeypatch)
    got = [grid.vertical_diffusion(*f, **kw) for grid, f, kw in cases]
    assert len(calls) == len(cases)
    fake_device.install(monkeypatch)
    for (grid, f, kw), g in zip(cases, got):
        _same_labelled(g, _chain(grid, *f, **kw))


def _same_bits(got, want):
    """NaN where the other is NaN; everywhere else the same bit pattern, so that -0.0 is not +0.0"""
    g, w = np.asarray(got), np.asarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan)
    bits = {4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
    assert np.array_equal(np.where(nan, 0, g).view(bits), np.where(nan, 0, w).view(bits))


# (lead, nz, ny, nx, metric form, kappa form, where `a` sits): the lead / metric / kappa cases of the boundary matrix
MATRIX = [((), 4, 5, 8, "1d", "3d", "c"), ((2,), 3, 5, 6, "full", "1d", "u"), ((2, 2), 3, 4, 5, "lead", "lead", "v"),
          ((3,), 5, 3, 12, "lead", None, "c"), ((), 3, 4, 6, "1d", "1d", "v"), ((2,), 4, 3, 5, "full", "lead", "c"),
          ((2,), 1, 2, 4, "1d", "3d", "u"), ((), 2, 1, 1, "full", "3d", "c")]


def matrix_cases(pz, to, dtype):
    """(grid, (a, kappa), kwargs, ds) over MATRIX x {no NaN, NaN} x {metric-weighted, not}, the fills rotating"""
    out = []
    for n, (lead, nz, ny, nx, metric, kform, hpos) in enumerate(MATRIX):
        grid, ds, dims = _grid(lead, nz, ny, nx, dtype, pz, metric=metric, hpos=hpos)
        kappa = _kappa(kform, lead, nz, ny, nx, dtype, dims, to, hpos)
        for nan, weighted in itertools.product((False, True), (True, False)):
            a = _field(lead, nz, ny, nx, dtype, dims, hpos, nan=nan)
            out.append((grid, (a, kappa), dict(to=to, fill_value=FILLS[(n + nan + weighted) % 3], metric_weighted=weighted), ds))
    return out


def signed_zero_cases(dtype):
    """(grid, (a, kappa), kwargs, ds, pz) whose results are full of exact zeros of both signs: a constant `a` (every
    difference is +0.0, every flux +-0.0 by kappa's sign), an `a` of -0.0, a kappa of zeros of both signs over a random `a`
    -- under every Z boundary and both flux positions, with a -0.0, no and a +0.0 fill"""
    out = []
    for n, (pz, to) in enumerate(itertools.product(BCS, TOS)):
        grid, ds, dims = _grid((2,), 3, 4, 6, dtype, pz)
        a = _field((2,), 3, 4, 6, dtype, dims)
        kappa = _kappa("3d", (2,), 3, 4, 6, dtype, dims, to)
        const = a._replace(data=np.full(a.shape, 0.75, dtype))
        neg0 = a._replace(data=-np.zeros(a.shape, dtype))
        skap = kappa._replace(data=np.where(kappa.values > 0, dtype(0.0), dtype(-0.0)).astype(dtype))
        fields = [(const, kappa), (neg0, kappa), (a, skap), (const, skap), (neg0, None)][n % 5]
        for fill in (-0.0, None, 0.0):
            out.append((grid, fields, dict(to=to, fill_value=fill, metric_weighted=bool(n % 2)), ds, pz))
    return out


# ---- 1. the one-pass result equals the chain ------------------------------------------------------------------------------
@pytest.mark.parametrize("pz", BCS)
@pytest.mark.parametrize("to", TOS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_equals_the_chain(host_abi, monkeypatch, pz, to, dtype):
    _compare_with_chain(monkeypatch, [c[:3] for c in matrix_cases(pz, to, dtype)])


@pytest.mark.parametrize("pz", BCS)
@pytest.mark.parametrize("to", TOS)
def test_equals_the_numpy_statement(host_abi, pz, to):
    for dtype in (np.float64, np.float32):
        for grid, (a, kappa), kw, ds in matrix_cases(pz, to, dtype):
            got = grid.vertical_diffusion(a, kappa, **kw)
            want = _want_of(grid, ds, a, kappa, to, pz, kw["fill_value"], kw["metric_weighted"])
            assert got.values.dtype == want.dtype == np.dtype(dtype) and np.array_equal(got.values, want, equal_nan=True)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_signed_zeros_and_negative_zero_fills_keep_their_sign(host_abi, monkeypatch, dtype):
    """bit patterns, not values: a -0.0 fill is handed on as -0.0, as the chain's one-axis operators do"""
    from oracle import fake_device

    calls = _counted(monkeypatch)
    cases = signed_zero_cases(dtype)
    got = [grid.vertical_diffusion(*f, **kw) for grid, f, kw, _, _ in cases]
    assert len(calls) == len(cases)
    fake_device.install(monkeypatch)
    zeros = negative = 0
    for (grid, f, kw, ds, pz), g in zip(cases, got):
        _same_bits(g.values, _chain(grid, *f, **kw).values)
        _same_bits(g.values, _want_of(grid, ds, *f, kw["to"], pz, kw["fill_value"], kw["metric_weighted"]))
        zeros += int((g.values == 0).sum())
        negative += int(((g.values == 0) & np.signbit(g.values)).sum())
    assert 0 < negative < zeros   # the cases do hold zeros of both signs


def test_extend_to_outer_is_the_no_flux_condition(host_abi):
    """`outer` under `extend`: the flux at the top and at the bottom is exactly zero, so the column sum of out * drF vanishes
    up to rounding and a constant `a` gives exact zeros whatever kappa is"""
    grid, ds, dims = _grid((), 6, 3, 4, np.float64, "extend")
    a = _field((), 6, 3, 4, np.float64, dims)
    kappa = _kappa("3d", (), 6, 3, 4, np.float64, dims, "outer")
    out = grid.vertical_diffusion(a, kappa)
    assert out.dims == a.dims
    total = (out.values * ds["drF"].values[:, None, None]).sum(axis=0)
    scale = np.abs(out.values * ds["drF"].values[:, None, None]).sum(axis=0)
    assert (np.abs(total) <= 1e-12 * scale).all()
    flat = grid.vertical_diffusion(a._replace(data=np.full(a.shape, 2.5)), kappa)
    assert (flat.values == 0).all()


def test_to_defaults_to_outer_when_the_axis_has_it_else_left(host_abi, monkeypatch):
    calls = _counted(monkeypatch)
    grid, ds, dims = _grid((2,), 3, 4, 6, np.float64, "fill")
    a = _field((2,), 3, 4, 6, np.float64, dims)
    kl, ko = (_kappa("3d", (2,), 3, 4, 6, np.float64, dims, to) for to in TOS)
    assert np.array_equal(grid.vertical_diffusion(a, ko).values, grid.vertical_diffusion(a, ko, to="outer").values)
    axes = dict(AXES, Z={"center": "ZC", "left": "ZL"})
    g2, ds2, _ = _grid((2,), 3, 4, 6, np.float64, "fill", axes=axes, metric=None)
    assert np.array_equal(g2.vertical_diffusion(a, kl, metric_weighted=False).values,
                          grid.vertical_diffusion(a, kl, to="left", metric_weighted=False).values)
    assert len(calls) == 4


def test_xarray_in_xarray_out(host_abi, monkeypatch):
    import xarray_standin
    from oracle import fake_device

    xarray_standin.install(monkeypatch)
    import xarray as xr

    grid, ds, dims = _grid((), 3, 4, 6, np.float64, "extend")
    a = _field((), 3, 4, 6, np.float64, dims)
    kappa = _kappa("3d", (), 3, 4, 6, np.float64, dims, "outer")
    got = grid.vertical_diffusion(*(xr.DataArray(x.values, dims=x.dims, name=x.name) for x in (a, kappa)))
    assert type(got).__module__.split(".")[0] == "xarray"
    fake_device.install(monkeypatch)
    want = _chain(grid, a, kappa, to="outer")
    assert tuple(got.dims) == tuple(want.dims) and got.name == want.name
    assert np.array_equal(np.asarray(got.values), np.asarray(want.values))


def test_coords_and_names_follow_the_chain(host_abi, monkeypatch):
    cases = []
    for names in (("T", "kappa"), ("q", "q"), ("drF", "drF"), (None, "kappa"), ("drCo", None)):
        for metric, to in (("1d", "outer"), ("full", "left")):
            grid, ds, dims = _grid((2,), 3, 5, 6, np.float64, "fill", metric=metric)
            a = _field((2,), 3, 5, 6, np.float64, dims)._replace(name=names[0])
            kappa = _kappa("3d", (2,), 3, 5, 6, np.float64, dims, to)._replace(name=names[1])
            a = a.assign_coords({"lon": (("YC", "XC"), np.ones((5, 6))), "t2": (("time",), np.arange(2) + 7.0),
                                 "depth": (("ZC",), np.arange(3) * 10.0)})
            kappa = kappa.assign_coords({"depth_f": ((ZDIM[to],), np.arange(_nf(3, to)) * 10.0), "lon": (("YC", "XC"), np.ones((5, 6)))})
            for mw in (True, False):
                cases += [(grid, (a, kappa), dict(to=to, fill_value=0.375, metric_weighted=mw)),
                          (grid, (a, None), dict(to=to, metric_weighted=mw))]
    _compare_with_chain(monkeypatch, cases)


def test_kappa_with_its_dims_in_another_order_is_read_in_place(host_abi, monkeypatch):
    grid, ds, dims = _grid((2,), 3, 5, 6, np.float64, "periodic")
    a = _field((2,), 3, 5, 6, np.float64, dims)
    kappa = _kappa("3d", (2,), 3, 5, 6, np.float64, dims, "left").transpose("XC", "ZL", "YC")
    yx = DataArray(R.synthetic_field((5, 6), 77), ("YC", "XC"), name="kappa")   # no Z dim: the same plane at every level
    _compare_with_chain(monkeypatch, [(grid, (a, kappa), dict(to="left")), (grid, (a, yx), dict(to="outer"))])


def test_the_fused_entry_runs_alone(host_abi, monkeypatch):
    """one call of the one-pass device entry and none of the chain's operators"""
    import xgcm_amd.device as D

    grid, ds, dims = _grid((2,), 3, 5, 6, np.float64, "extend")
    a = _field((2,), 3, 5, 6, np.float64, dims)
    kappa = _kappa("3d", (2,), 3, 5, 6, np.float64, dims, "outer")
    calls = {"fused": 0, "chain": 0}

    def counted(fn, key):
        def wrapped(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(D, "vertical_diffusion", counted(D.vertical_diffusion, "fused"))
    for name in ("binary", "stencil1d"):
        monkeypatch.setattr(D, name, counted(getattr(D, name), "chain"))
    out = grid.vertical_diffusion(a, kappa, fill_value=0.375)
    assert np.array_equal(out.values, _want_of(grid, ds, a, kappa, "outer", "extend", 0.375, True))
    assert out.dims == ("time", "ZC", "YC", "XC")
    assert calls == {"fused": 1, "chain": 0}


# ---- 2. the smallest shapes at which it can go wrong ----------------------------------------------------------------------
NZS, NYS, NXS = [1, 2, 3, 5], [1, 2, 3, 9], [1, 2, 3, 8, 129, 130, 257]
PADS2 = list(itertools.product(BCS, TOS))


def shape_table(nx):
    """(nz, ny, nx, pz, to, dtype, metric form, kappa form, metric_weighted): every nz and ny with this nx -- one level (both Z
    pads touch the same cell), one row, a single column, nx across one x-tile, odd nx (the narrow form), odd ny (a ragged last
    segment) -- the boundary, the flux position, the dtype, the metric and the kappa forms rotating so that the table as a
    whole meets every combination several times"""
    out = []
    for n, (nz, ny) in enumerate(itertools.product(NZS, NYS)):
        k = n + 5 * NXS.index(nx)
        pz, to = PADS2[(5 * k) % len(PADS2)]
        out.append((nz, ny, nx, pz, to, (np.float64, np.float32)[(k // 2) % 2], ("1d", "full")[k % 2],
                    (None, "1d", "3d")[(k // 2) % 3], bool((k // 3) % 2)))
    return out


def shape_cases(nx):
    cases = []
    for nz, ny, nx_, pz, to, dtype, metric, kform, mw in shape_table(nx):
        grid, ds, dims = _grid((), nz, ny, nx_, dtype, pz, metric=metric)
        a = _field((), nz, ny, nx_, dtype, dims, nan=(nz + ny) % 2 == 0)
        kappa = _kappa(kform, (), nz, ny, nx_, dtype, dims, to)
        cases.append((grid, (a, kappa), dict(to=to, fill_value=FILLS[(nz + ny) % 3], metric_weighted=mw)))
    return cases


def test_the_shape_table_meets_every_boundary_position_and_dtype():
    seen = {(pz, to, np.dtype(dt).name) for nx in NXS for _, _, _, pz, to, dt, _, _, _ in shape_table(nx)}
    assert seen == {(pz, to, dt) for pz, to in PADS2 for dt in ("float64", "float32")}


@pytest.mark.parametrize("nx", NXS)
def test_small_shapes(host_abi, monkeypatch, nx):
    cases = shape_cases(nx)
    assert len(cases) == len(NZS) * len(NYS)
    _compare_with_chain(monkeypatch, cases)


# ---- 3. NaN and Inf -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("to", TOS)
def test_a_nan_poisons_exactly_its_stencil(host_abi, to):
    """a[k] enters the fluxes at k and k + 1 and through them the results at k - 1, k and k + 1: exactly those levels of its
    column, wrapped under a periodic boundary"""
    nz, ny, nx, (k, j, i) = 6, 3, 5, (0, 2, 4)
    grid, ds, dims = _grid((), nz, ny, nx, np.float64, "periodic")
    a = _field((), nz, ny, nx, np.float64, dims)
    a.values[k, j, i] = np.nan
    out = grid.vertical_diffusion(a, _kappa("1d", (), nz, ny, nx, np.float64, dims, to), to=to)
    mask = np.zeros((nz, ny, nx), bool)
    mask[[(k - 1) % nz, k, (k + 1) % nz], j, i] = True
    assert np.array_equal(np.isnan(out.values), mask)


def test_inf_times_zero_is_nan_as_in_the_chain(host_abi, monkeypatch):
    cases = []
    for pz, to in PADS2:
        grid, ds, dims = _grid((2,), 4, 3, 5, np.float64, pz)
        a = _field((2,), 4, 3, 5, np.float64, dims)
        kappa = _kappa("3d", (2,), 4, 3, 5, np.float64, dims, to)
        a.values[:, 2, 1, 1] = a.values[:, 1, 1, 1]    # a zero gradient under an infinite kappa
        kappa.values[2, 1, 1] = np.inf
        kappa.values[1, 2, 3] = -np.inf
        cases.append((grid, (a, kappa), dict(to=to, fill_value=0.375)))
    got = [grid.vertical_diffusion(*f, **kw) for grid, f, kw in cases]
    for g in got:
        assert np.isnan(g.values[:, 1:3, 1, 1]).all() and np.isinf(g.values[:, 0:2, 2, 3]).all()
    _compare_with_chain(monkeypatch, cases)


# ---- 4. every fallback of the docstring takes the chain -------------------------------------------------------------------
def _no_fused(monkeypatch):
    import xgcm_amd.device as D

    monkeypatch.setattr(D, "vertical_diffusion", lambda *a, **k: pytest.fail("one-pass entry called"))


def _fallback_equals_chain(grid, a, kappa=None, **kw):
    """what the chain returns, or what it raises"""
    try:
        want = _chain(grid, a, kappa, **kw)
    except Exception as chain_err:   # noqa: BLE001 -- whatever the chain raises, the operator must raise the same
        with pytest.raises(type(chain_err)) as err:
            grid.vertical_diffusion(a, kappa, **kw)
        assert type(err.value) is type(chain_err) and str(err.value) == str(chain_err)
        return "raised"
    _same_labelled(grid.vertical_diffusion(a, kappa, **kw), want)
    return "returned"


def _case(pz="fill", lead=(2,), nz=3, ny=5, nx=6, dtype=np.float64, to="outer", kform="3d", **gk):
    grid, ds, dims = _grid(lead, nz, ny, nx, dtype, pz, **gk)
    return grid, ds, _field(lead, nz, ny, nx, dtype, dims), _kappa(kform, lead, nz, ny, nx, dtype, dims, to)


@pytest.mark.parametrize("dtype", [np.int64, np.int32, np.float16])
def test_integer_and_half_fields_run_the_chain(backend, monkeypatch, dtype):
    _no_fused(monkeypatch)
    grid, ds, a, kappa = _case()
    ai = DataArray((a.values * 100).astype(dtype), a.dims, name="T")
    ki = DataArray((kappa.values * 100).astype(dtype), kappa.dims, name="kappa")
    for kw in (dict(), dict(metric_weighted=False, fill_value=0.375, to="outer")):
        assert _fallback_equals_chain(grid, ai, ki, **kw) == "returned"
        assert _fallback_equals_chain(grid, ai, None, **kw) == "returned"


def test_mixed_dtypes_run_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, a, kappa = _case(dtype=np.float32, mdtype=np.float64)
    assert _fallback_equals_chain(grid, a, kappa, fill_value=0.375) == "returned"       # float32 over float64 metrics
    k64 = kappa._replace(data=kappa.values.astype(np.float64))
    assert _fallback_equals_chain(grid, a, k64, metric_weighted=False) == "returned"    # a kappa of another dtype
    assert _fallback_equals_chain(grid, a, 2.0, metric_weighted=False) == "returned"    # a plain number


def test_fewer_than_three_dims_or_z_elsewhere_run_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, a, kappa = _case()
    col = DataArray(np.ascontiguousarray(a.values[0, :, :, 0]), ("ZC", "YC"), name="T")
    assert _fallback_equals_chain(grid, col, None, fill_value=0.375) == "returned"
    assert _fallback_equals_chain(grid, a.transpose("ZC", "time", "YC", "XC"), kappa, fill_value=0.375) == "returned"
    assert _fallback_equals_chain(grid, a.transpose("time", "YC", "ZC", "XC"), None, metric_weighted=False) == "returned"
    # `a` not at Z:center: whatever the chain makes of it
    _fallback_equals_chain(grid, DataArray(a.values, ("time", "ZL", "YC", "XC"), name="T"), None, to="outer")


@pytest.mark.parametrize("to", ["right", "inner", "center", "nowhere"])
def test_other_targets_run_the_chain(backend, monkeypatch, to):
    _no_fused(monkeypatch)
    grid, ds, a, kappa = _case()
    _fallback_equals_chain(grid, a, None, to=to, metric_weighted=False)
    _fallback_equals_chain(grid, a, None, to=to)


def test_a_position_the_axis_lacks_runs_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    axes = dict(AXES, Z={"center": "ZC", "left": "ZL"})
    grid, ds, dims = _grid((2,), 3, 5, 6, np.float64, "fill", axes=axes, metric=None)
    a = _field((2,), 3, 5, 6, np.float64, dims)
    assert _fallback_equals_chain(grid, a, None, to="outer", metric_weighted=False) == "raised"


def test_kappa_elsewhere_or_with_other_dims_runs_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, a, kappa = _case()
    at_center = DataArray(kappa.values[:3], ("ZC", "YC", "XC"), name="kappa")
    _fallback_equals_chain(grid, a, at_center, metric_weighted=False)            # not at the flux position
    at_left = _kappa("3d", (2,), 3, 5, 6, np.float64, (), "left")
    _fallback_equals_chain(grid, a, at_left, to="outer", metric_weighted=False)  # at the other flux position
    extra = DataArray(R.synthetic_field((4, 4), 78), ("member", "ZO"), name="kappa")
    assert _fallback_equals_chain(grid, a, extra, metric_weighted=False) == "returned"   # a dim `a` lacks: it broadcasts
    short = DataArray(R.synthetic_field((3,), 79), ("ZO",), name="kappa")
    assert _fallback_equals_chain(grid, a, short, metric_weighted=False) == "raised"     # an extent that does not fit


def test_chunked_inputs_run_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, dims = _grid((4,), 3, 6, 8, np.float64, "fill")
    a = _field((4,), 3, 6, 8, np.float64, dims)
    kappa = _kappa("lead", (4,), 3, 6, 8, np.float64, dims, "outer")
    ca = DataArray(BlockArray.from_array(a.values, ((2, 2), (3,), (6,), (8,))), a.dims, name="T")
    ck = DataArray(BlockArray.from_array(kappa.values, ((2, 2), (4,), (6,), (8,))), kappa.dims, name="kappa")
    plain = _want_of(grid, ds, a, kappa, "outer", "fill", 0.375, True)
    for x, k in ((ca, kappa), (a, ck)):
        got, want = grid.vertical_diffusion(x, k, fill_value=0.375), _chain(grid, x, k, fill_value=0.375)
        assert got.dims == want.dims and got.name == want.name
        assert np.array_equal(np.asarray(got.values), np.asarray(want.values)) and np.array_equal(np.asarray(got.values), plain)


def test_a_metric_with_an_extra_dim_runs_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, dims = _grid((), 3, 5, 6, np.float64, "fill")
    coords = {k: (k, np.asarray(ds.coords[k].values)) for k in ("XC", "XG", "YC", "YG", "ZC", "ZL", "ZO")}
    coords["time"] = ("time", np.arange(2) * 2.0)
    data = {"drF": (("ZC", "time"), R.synthetic_metric((3, 2), 66)), "drCo": (("ZO", "time"), R.synthetic_metric((4, 2), 67))}
    g2 = Grid(Dataset(data, coords), coords=AXES, metrics={("Z",): ["drF", "drCo"]},
              padding={"X": "periodic", "Y": "periodic", "Z": "fill"}, autoparse_metadata=False)
    a = _field((), 3, 5, 6, np.float64, ())
    got, want = g2.vertical_diffusion(a, fill_value=0.375), _chain(g2, a, fill_value=0.375)
    assert "time" in got.dims
    _same_labelled(got, want)


def test_a_chunked_metric_runs_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, dims = _grid((), 4, 5, 6, np.float64, "fill", metric="full")
    coords = {k: (k, np.asarray(ds.coords[k].values)) for k in ("XC", "XG", "YC", "YG", "ZC", "ZL", "ZO")}
    data = {k: (ds[k].dims, np.asarray(ds[k].values)) for k in ("drF", "drCl", "drCo")}
    data["drF"] = (ds["drF"].dims, BlockArray.from_array(np.asarray(ds["drF"].values), ((2, 2), (5,), (6,))))
    g2 = Grid(Dataset(data, coords), coords=AXES, metrics={("Z",): ["drF", "drCl", "drCo"]},
              padding={"X": "periodic", "Y": "periodic", "Z": "fill"}, autoparse_metadata=False)
    a = _field((), 4, 5, 6, np.float64, ())
    got, want = g2.vertical_diffusion(a, fill_value=0.375), _chain(g2, a, fill_value=0.375)
    assert got.dims == want.dims and got.name == want.name
    assert np.array_equal(np.asarray(got.values), np.asarray(want.values))
    assert np.array_equal(np.asarray(got.values), _want_of(grid, ds, a, None, "outer", "fill", 0.375, True))


def test_a_missing_metric_raises_the_chains_error(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, a, kappa = _case(metric=None)
    assert _fallback_equals_chain(grid, a, kappa) == "raised"


def test_a_missing_metric_is_still_served_unweighted(host_abi, monkeypatch):
    grid, ds, a, kappa = _case(metric=None)
    _compare_with_chain(monkeypatch, [(grid, (a, kappa), dict(metric_weighted=False))])


def test_missing_z_boundary_raises_the_chains_error(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, a, kappa = _case(pz=None)
    for to in TOS:
        assert _fallback_equals_chain(grid, a, None, to=to) == "raised"


Z_TO_Z = {"face": {0: {"Z": (None, (1, "Z", False))}, 1: {"Z": ((0, "Z", False), None)}}}


def test_faces_connected_along_z_run_the_chain(backend, monkeypatch):
    from test_topology import COORDS

    _no_fused(monkeypatch)
    ds = Dataset({"drF": (("zc",), R.synthetic_metric((4,), 63)), "drC": (("zl",), R.synthetic_metric((4,), 64))},
                 coords={"x": np.arange(4), "xl": np.arange(4) - 0.5, "y": np.arange(4), "yl": np.arange(4) - 0.5,
                         "face": np.arange(2), "zc": np.arange(4) + 0.5, "zl": np.arange(4) * 1.0})
    grid = Grid(ds, coords=dict(COORDS, Z={"center": "zc", "left": "zl"}), face_connections=Z_TO_Z,
                metrics={("Z",): ["drF", "drC"]}, padding={"X": "periodic", "Y": "extend", "Z": "fill"}, autoparse_metadata=False)
    a = DataArray(R.synthetic_field((2, 4, 4, 4), 82), ("face", "zc", "y", "x"), name="T")
    kappa = DataArray(R.synthetic_field((2, 4, 4, 4), 83), ("face", "zl", "y", "x"), name="kappa")
    for mw in (True, False):
        assert _fallback_equals_chain(grid, a, kappa, fill_value=0.375, metric_weighted=mw) == "returned"


def test_a_fold_along_z_runs_the_chain(backend, monkeypatch):
    import warnings

    _no_fused(monkeypatch)
    nz, ny, nx = 4, 3, 6
    ds = Dataset({"drF": (("zc",), R.synthetic_metric((nz,), 63)), "drC": (("zl",), R.synthetic_metric((nz,), 64))},
                 coords={"xh": np.arange(nx), "xl": np.arange(nx), "yh": np.arange(ny), "yl": np.arange(ny),
                         "zc": np.arange(nz) + 0.5, "zl": np.arange(nz) * 1.0})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        grid = Grid(ds, coords={"X": {"center": "xh", "left": "xl"}, "Y": {"center": "yh", "left": "yl"},
                                "Z": {"center": "zc", "left": "zl"}}, metrics={("Z",): ["drF", "drC"]},
                    padding={"X": "periodic", "Y": "extend", "Z": {"fold": "corner"}}, autoparse_metadata=False)
        a = DataArray(R.synthetic_field((2, nz, ny, nx), 92), ("t", "zc", "yh", "xh"), name="T")
        kappa = DataArray(R.synthetic_field((nz, ny, nx), 93), ("zl", "yh", "xh"), name="kappa")
        for mw in (True, False):
            assert _fallback_equals_chain(grid, a, kappa, metric_weighted=mw) == "returned"


# ---- 5. the entry of the C ABI called directly, with views ----------------------------------------------------------------
NVS = {np.float64: 2, np.float32: 4}
TORCH = {np.float64: torch.float64, np.float32: torch.float32}
CODE = {np.float64: _hip.DTYPE["float64"], np.float32: _hip.DTYPE["float32"]}
ABI_NX = {np.float64: 132, np.float32: 264}   # one full 64-lane tile and a partial one
ABI_PADS = [("periodic", "left"), ("fill", "outer"), ("extend", "left"), ("periodic", "outer")]
SENTINEL = 12345.5


def _abi_call(D, dtype, shape, a, planes, k, out_off=ALIGNED):
    """one call of xg_vertical_diffusion: `a` a contiguous view, `planes` {kappa, mf, mc} views or None; the result is written
    `out_off` elements into an allocation full of SENTINEL, which must still surround it afterwards"""
    pz, to = ABI_PADS[k]
    fshape = shape[:-3] + [_nf(shape[-3], to)] + shape[-2:]
    args = [CODE[dtype], a.data_ptr()]
    for name, against in (("kappa", fshape), ("mf", fshape), ("mc", shape)):
        m = planes.get(name)
        if m is None:
            args += [None, None]
        else:
            assert all(n in (1, s) for n, s in zip(m.shape, against))
            args += [m.data_ptr(), _hip.i64([0 if n == 1 else m.stride(d) for d, n in enumerate(m.shape)])]
    n = int(np.prod(shape))
    buf = torch.full((out_off + n + ALIGNED,), SENTINEL, dtype=TORCH[dtype], device=D._MEM.device)
    out = buf[out_off:out_off + n]
    args += [out.data_ptr(), _hip.i64(shape), len(shape), int(to == "outer"), _hip.BC[pz], 0.375]
    D._check(D._MEM.lib().xg_vertical_diffusion(*args, D._stream()))
    whole = buf.cpu().numpy()
    assert (whole[:out_off] == SENTINEL).all() and (whole[out_off + n:] == SENTINEL).all()
    return whole[out_off:out_off + n].reshape(shape)


def abi_layout_cases(dtype):
    """Runs the direct-ABI table on whatever library `xgcm_amd.device._MEM` serves.  Every input view lives in a NaN-filled
    allocation, so a read outside it shows in the result; the contiguous, aligned control of each set of planes is compared
    with the numpy chain, every other layout with that control."""
    import xgcm_amd.device as D

    nv = NVS[dtype]
    shape = [2, 5, 7, ABI_NX[dtype]]
    lead, nz, ny, nx = shape
    av = R.synthetic_field(tuple(shape), 101).astype(dtype)
    av.reshape(-1)[5::17] = np.nan
    put = lambda x, st=None, off=ALIGNED: _strided(D, x, st or _contig(x.shape), off)  # noqa: E731
    for k, (pz, to) in enumerate(ABI_PADS):
        nf = _nf(nz, to)
        levels = {"kappa": nf, "mf": nf, "mc": nz}

        def vals(name, form, seed):
            n = levels[name]
            sh = {"z": (1, n, 1, 1), "p": (1, 1, ny, nx), "v3": (1, n, ny, nx), "vl": (lead, n, ny, nx)}[form]
            make = R.synthetic_field if name == "kappa" else R.synthetic_metric
            return make(sh, seed).astype(dtype)

        a = put(av)
        assert a.is_contiguous() and a.data_ptr() % 16 == 0
        for present in ({"kappa": "v3"}, {"kappa": "z"}, {"kappa": "vl", "mf": "z", "mc": "z"}, {"mf": "v3", "mc": "p"},
                        {"kappa": "p", "mc": "vl"}, {"kappa": "v3", "mf": "vl", "mc": "v3"}, {}):
            pv = {n: vals(n, form, 111 + i) for i, (n, form) in enumerate(present.items())}
            control = _abi_call(D, dtype, shape, a, {n: put(x) for n, x in pv.items()}, k)
            want = _want(av, pv.get("kappa"), pv.get("mf"), pv.get("mc"), to, pz, dtype(0.375))
            assert control.dtype == want.dtype == np.dtype(dtype) and np.array_equal(control, want, equal_nan=True), (k, present)
            views = []
            # a misaligned field, a misaligned result, both: one element into the allocation (the narrow form)
            a1 = put(av, off=1)
            assert a1.data_ptr() % 16 == av.dtype.itemsize
            aligned = {n: put(x) for n, x in pv.items()}
            views += [(a1, aligned, ALIGNED), (a, aligned, 1), (a1, aligned, 1)]
            # the planes one element in; with an odd row pitch; with an odd level pitch (volumes)
            views.append((a, {n: put(x, off=1) for n, x in pv.items()}, ALIGNED))
            pitched = {}
            for n, x in pv.items():
                s = list(x.shape)
                st = _contig(s[:-1] + [s[-1] + 1]) if s[-1] > 1 else _contig(s)
                pitched[n] = put(x, st)
                assert s[-1] == 1 or (pitched[n].stride(-2) == nx + 1 and pitched[n].stride(-1) == 1)
            views.append((a, pitched, ALIGNED))
            for n, form in present.items():
                x = pv[n]
                if form in ("v3", "vl"):
                    st = [(x.shape[1] * (ny * nx + 1)) * (x.shape[0] > 1), ny * nx + 1, nx, 1]
                    lev = put(x, [s or 1 for s in st])
                    assert lev.stride(1) == ny * nx + 1
                    views.append((a, dict(aligned, **{n: lev}), ALIGNED))
                if form == "z":   # the Z-only array three elements apart
                    views.append((a, dict(aligned, **{n: put(x, [3 * x.shape[1], 3, 1, 1], 1)}), ALIGNED))
                if form == "p":   # the plane stored (X, Y): a transposed view
                    t = put(np.ascontiguousarray(x.transpose(0, 1, 3, 2))).permute(0, 1, 3, 2)
                    assert t.stride(-1) == ny and t.stride(-2) == 1
                    views.append((a, dict(aligned, **{n: t}), ALIGNED))
            for fa, planes, out_off in views:
                got = _abi_call(D, dtype, shape, fa, planes, k, out_off)
                assert np.array_equal(got, control, equal_nan=True), (k, present)
        # stride 0 along X and Y: one value per level, expanded over the whole volume, equals the Z-only array
        for name in ("kappa", "mf", "mc"):
            z = vals(name, "z", 121)
            flat = put(z).expand(1, levels[name], ny, nx)
            assert flat.stride(-1) == 0 and flat.stride(-2) == 0
            full = put(np.ascontiguousarray(np.broadcast_to(z, (1, levels[name], ny, nx))))
            assert np.array_equal(_abi_call(D, dtype, shape, a, {name: flat}, k), _abi_call(D, dtype, shape, a, {name: full}, k),
                                  equal_nan=True)
    assert nx % nv == 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_abi_layouts(host_abi, dtype):
    abi_layout_cases(dtype)


def abi_bad_calls():
    """bad calls return an error code and leave the process alone; runs on whatever library `_MEM` serves"""
    import xgcm_amd.device as D

    lib = D._MEM.lib()
    shape = [2, 3, 4]
    t = torch.zeros(shape, dtype=torch.float64, device=D._MEM.device)
    out = torch.zeros_like(t)

    def call(code=CODE[np.float64], a=t, ndim=3, outer=0, bcz=_hip.BC["fill"], kappa=None, ks=None):
        return lib.xg_vertical_diffusion(code, a.data_ptr() if a is not None else None, kappa, ks, None, None, None, None,
                                         out.data_ptr(), _hip.i64(shape), ndim, outer, bcz, 0.0, D._stream())

    assert call() == 0 and call(bcz=_hip.BC["periodic"]) == 0 and call(bcz=_hip.BC["extend"], outer=1) == 0
    for code in (-1, _hip.DTYPE["float16"], _hip.DTYPE["int64"], _hip.DTYPE["int32"], 12, 99):
        assert call(code=code) == -1                             # any other element type: XG_ERR_INVALID
    assert call(a=None) == -1                                    # NULL array
    assert call(bcz=7) == -1 and call(outer=2) == -1             # unknown boundary code, unknown flux position
    assert call(kappa=t.data_ptr(), ks=None) == -1               # kappa without strides
    assert call(ndim=2) < 0 and call(ndim=2) != -1               # XG_ERR_UNSUPPORTED


def test_abi_refuses_bad_calls(host_abi):
    abi_bad_calls()
