"""The isopycnal slopes at the faces of Z, `Grid.isopycnal_slope`, on CPU.

The one-pass path runs through the `host_abi` fixture (the product's `xgcm_amd.device` over libxgcm_host.so); the chain it
replaces

    step = grid.derivative | grid.diff
    gx = interp(interp(step(b, X), X), Z, to);  gy = interp(interp(step(b, Y), Y), Z, to);  bz = step(b, Z, to)
    sx, sy = -(gx / bz), -(gy / bz)

runs through the same Grid over the oracle double, installed AFTER the one-pass calls of a test have run.  `_want` states the
chain a third time, over plain numpy arrays with the oracle's one-axis functions.  Every comparison is bit for bit (NaN where
the other has NaN, -0.0 is not +0.0), with dims, coords and names where labels are compared.  The one-pass device entry is
counted and the chain's device functions are barred wherever a case must not pass by falling back.  The case builders and the
direct-ABI cases are shared with the GPU suite.

`Case.not_hollow` is asserted on the REFERENCE alone: in every case without a planted NaN, without a NaN fill and with two
levels or more, sx and sy are finite on every interior face (1 .. nz-1), under every Z boundary.  The all-zero fields of the
fill tables are 0 / 0 or x / 0 on every face by construction; they are no such cases and say so (`zero`)."""

import itertools

import numpy as np
import pytest
import torch

import guarded_memory as GM
import test_richardson_number as TR
from oracle import refimpl as R
from test_fused_layouts import ALIGNED, _contig, _strided
from xgcm_amd import DataArray, Dataset, Grid, _hip
from xgcm_amd.chunked import BlockArray

BCS, TOS, PADS3, FILL, FILLS, AXES, ZDIM = TR.BCS, TR.TOS, TR.PADS3, TR.FILL, TR.FILLS, TR.AXES, TR.ZDIM
NZS, NYS, NXS = TR.NZS, TR.NYS, TR.NXS
METRICS = [None, "planes", "full", "lead"]
# the dims of the three derivatives behind the leading dims: X at (ZC, YC, XG), Y at (ZC, YG, XC), Z at (Z face, YC, XC)
_same_labelled, _same_bits, _same_error = TR._same_labelled, TR._same_bits, TR._same_error


def _stage_dims(to):
    return ("ZC", "YC", "XG"), ("ZC", "YG", "XC"), (ZDIM[to], "YC", "XC")


def _grid(lead, nz, ny, nx, dtype, padding, metric="planes", mdtype=None):
    """C-grid with a Z axis that has a left and an outer position.  Metrics: "planes" -- dxC(YC, XG), dyC(YG, XC) and the
    profiles drCl(ZL), drCo(ZO); "full" -- 3-D arrays at the three stages' points (hx, hy, hzl, hzo); "lead": the same with
    the first leading dim in front; None: no metric at all"""
    dims = ("time", "member")[:len(lead)]
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0),
              "YC": ("YC", np.arange(ny) + 0.5), "YG": ("YG", np.arange(ny) * 1.0),
              "ZC": ("ZC", np.arange(nz) + 0.5), "ZL": ("ZL", np.arange(nz) * 1.0), "ZO": ("ZO", np.arange(nz + 1) * 1.0)}
    for d, n in zip(dims, lead):
        coords[d] = (d, np.arange(n) * 2.0)
    m = lambda shape, seed: R.synthetic_metric(shape, seed).astype(mdtype or dtype)  # noqa: E731
    data, metrics = {}, {}
    if metric == "planes":
        data = {"dxC": (("YC", "XG"), m((ny, nx), 61)), "dyC": (("YG", "XC"), m((ny, nx), 62)),
                "drCl": (("ZL",), m((nz,), 63)), "drCo": (("ZO",), m((nz + 1,), 64))}
        metrics = {("X",): ["dxC"], ("Y",): ["dyC"], ("Z",): ["drCl", "drCo"]}
    elif metric is not None:
        pl, pd = ((lead[0],), dims[:1]) if metric == "lead" and lead else ((), ())
        data = {"hx": (pd + ("ZC", "YC", "XG"), m(pl + (nz, ny, nx), 66)), "hy": (pd + ("ZC", "YG", "XC"), m(pl + (nz, ny, nx), 67)),
                "hzl": (pd + ("ZL", "YC", "XC"), m(pl + (nz, ny, nx), 68)), "hzo": (pd + ("ZO", "YC", "XC"), m(pl + (nz + 1, ny, nx), 69))}
        metrics = {("X",): ["hx"], ("Y",): ["hy"], ("Z",): ["hzl", "hzo"]}
    ds = Dataset(data, coords)
    return Grid(ds, coords=AXES, metrics=metrics, padding=padding, autoparse_metadata=False), ds, dims


def _field(lead, nz, ny, nx, dtype, dims, nan=False, seed=71, zero=False):
    shape = tuple(lead) + (nz, ny, nx)
    b = np.zeros(shape, dtype) if zero else R.synthetic_field(shape, seed).astype(dtype)
    if nan:
        b.reshape(-1)[3::11] = np.nan
        b[..., 0, 0, 0] = np.nan               # beside all three pads
        b[..., nz - 1, ny - 1, nx - 1] = np.nan
    return DataArray(b, dims + ("ZC", "YC", "XC"), name="b")


def _chain(grid, b, x_axis="X", y_axis="Y", z_axis="Z", to=None, padding=None, fill_value=None, metric_weighted=True):
    """the specification"""
    kw = dict(padding=padding, fill_value=fill_value)
    step = grid.derivative if metric_weighted else grid.diff
    if to is None:   # the operator's default: Z:outer when the axis has that position, else Z:left
        to = "outer" if "outer" in grid.axes[z_axis].coords else "left"
    gx = grid.interp(grid.interp(step(b, x_axis, **kw), x_axis, **kw), z_axis, to=to, **kw)
    gy = grid.interp(grid.interp(step(b, y_axis, **kw), y_axis, **kw), z_axis, to=to, **kw)
    bz = step(b, z_axis, to=to, **kw)
    return -(gx / bz), -(gy / bz)


def _want(b, pads, to, fill=FILL, mx=None, my=None, mz=None):
    """the numpy statement: the oracle's one-axis functions (the metrics broadcast against their stage)"""
    px, py, pz = pads
    z, y, x = b.ndim - 3, b.ndim - 2, b.ndim - 1
    hi = 1 if to == "outer" else 0
    S = R.stencil1d
    with np.errstate(all="ignore"):
        gx = S("interp", S("interp", S("diff", b, x, 1, 0, px, fill["X"], m_out=mx), x, 0, 1, px, fill["X"]), z, 1, hi, pz, fill["Z"])
        gy = S("interp", S("interp", S("diff", b, y, 1, 0, py, fill["Y"], m_out=my), y, 0, 1, py, fill["Y"]), z, 1, hi, pz, fill["Z"])
        bz = S("diff", b, z, 1, hi, pz, fill["Z"], m_out=mz)
        sx, sy = R.binary("mul", -1, R.binary("div", gx, bz)), R.binary("mul", -1, R.binary("div", gy, bz))
    assert sx.dtype == sy.dtype == b.dtype
    return sx, sy


def _metrics_of(ds, metric, to, dims):
    """(mx, my, mz) of `_grid` as numpy arrays that broadcast against their stage of a field with leading dims `dims`"""
    if metric is None:
        return None, None, None
    names = ("dxC", "dyC", "drC" + to[0]) if metric == "planes" else ("hx", "hy", "hz" + to[0])
    return tuple(TR._aligned(ds[n], dims + sd) for n, sd in zip(names, _stage_dims(to)))


class Case:
    """one call of the operator: the grid, its dataset and metric form, b, the keywords and the boundary triple"""

    def __init__(self, lead, nz, ny, nx, dtype, pads, to, metric="planes", weighted=True, fill=FILL, nan=False, seed=71, zero=False):
        self.pads, self.to, self.metric, self.nan, self.zero = tuple(pads), to, metric, nan, zero
        self.grid, self.ds, self.dims = _grid(lead, nz, ny, nx, dtype, dict(zip("XYZ", pads)), metric=metric)
        self.b = _field(lead, nz, ny, nx, dtype, self.dims, nan=nan, seed=seed, zero=zero)
        self.kw = dict(to=to, fill_value=fill, metric_weighted=bool(weighted and metric is not None))
        self.nz = nz

    def __repr__(self):
        return (f"{self.b.shape} {np.dtype(self.b.values.dtype)} {self.pads} {self.to} metric {self.metric} nan {self.nan} "
                f"zero {self.zero} {self.kw}")

    def one_pass(self):
        return self.grid.isopycnal_slope(self.b, **self.kw)

    def chain(self):
        return _chain(self.grid, self.b, **self.kw)

    def want(self):
        fill = self.kw["fill_value"] or {"X": 0.0, "Y": 0.0, "Z": 0.0}
        mets = _metrics_of(self.ds, self.metric if self.kw["metric_weighted"] else None, self.to, self.dims)
        return _want(self.b.values, self.pads, self.to, fill, *mets)

    def not_hollow(self, sx, sy):
        """asserted on the REFERENCE (see the module docstring); returns 1 when the statement was made"""
        fill = self.kw["fill_value"] or {}
        if self.nan or self.zero or any(np.isnan(x) for x in fill.values()) or self.nz < 2:
            return 0
        for s in (np.asarray(sx), np.asarray(sy)):
            assert np.isfinite(s[..., 1:self.nz, :, :]).all(), self
        return 1


def _counted(monkeypatch, bar_chain=True):
    """the calls of the one-pass device entry; `bar_chain`: and those of the chain's own device functions"""
    import xgcm_amd.device as D

    calls = {"fused": 0, "chain": 0}

    def counted(fn, key):
        def wrapped(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(D, "isopycnal_slope", counted(D.isopycnal_slope, "fused"))
    if bar_chain:
        for name in ("binary", "stencil1d"):
            monkeypatch.setattr(D, name, counted(getattr(D, name), "chain"))
    return calls


def compare_with_numpy(cases, monkeypatch=None):
    """both results of every case against the numpy statement, bit for bit, the statement first held to `not_hollow`; on
    whatever library `_MEM` serves.  With `monkeypatch`: exactly one call of the one-pass entry per case and none of the
    chain's.  Returns the number of cases for which `not_hollow` made its statement"""
    calls = _counted(monkeypatch) if monkeypatch is not None else None
    solid = 0
    for c in cases:
        want = c.want()
        solid += c.not_hollow(*want)
        got = c.one_pass()
        try:
            assert len(got) == 2
            for g, w in zip(got, want):
                _same_bits(g.values, w)
                assert g.dims == c.dims + (ZDIM[c.to], "YC", "XC")
        except AssertionError as err:
            raise AssertionError(f"case {c}") from err
    if calls is not None:
        assert calls == {"fused": len(cases), "chain": 0}
    return solid


def compare_with_chain(monkeypatch, cases):
    """every one-pass call first (counted, the chain barred), then the chain over the oracle double: values, dims, coords, names"""
    from oracle import fake_device

    calls = _counted(monkeypatch)
    got = [c.one_pass() for c in cases]
    assert calls == {"fused": len(cases), "chain": 0}
    fake_device.install(monkeypatch)
    for c, pair in zip(cases, got):
        with np.errstate(all="ignore"):
            want = c.chain()
        try:
            for g, w in zip(pair, want):
                _same_labelled(g, w)
                _same_bits(g.values, w.values)
        except AssertionError as err:
            raise AssertionError(f"case {c}") from err


# ---- 1. small shapes -------------------------------------------------------------------------------------------------------
def shape_cases(nx):
    """every nz and ny with this nx -- one level (every face averages a pad), one row and one column (both neighbours are
    pads), nx across a tile's last lane, odd nx (the narrow form) -- the boundary triple, the face position, the dtype, the
    metric form, the fills and the NaNs rotating so that the table as a whole meets every one of them several times"""
    out = []
    for n, (nz, ny) in enumerate(itertools.product(NZS, NYS)):
        k = n + 5 * NXS.index(nx)
        out.append(Case((), nz, ny, nx, (np.float64, np.float32)[(k // 2) % 2], PADS3[(7 * k) % 27], TOS[k % 2],
                        METRICS[(k // 2) % 3 + (k % 5 == 0)], fill=FILLS[(k // 3) % 3], nan=(nz + ny) % 3 == 0, seed=71 + k))
    return out


def test_the_shape_table_meets_every_boundary_triple_position_dtype_and_metric_form():
    cases = [c for nx in NXS for c in shape_cases(nx)]
    assert {c.pads for c in cases} == set(PADS3)
    assert {(c.pads[2], c.to, c.b.values.dtype.itemsize) for c in cases} == set(itertools.product(BCS, TOS, (4, 8)))
    assert {c.metric for c in cases} == set(METRICS)   # ("lead" without a leading dim: the 3-D form)
    assert {(c.nz, c.pads[2], c.to) for c in cases if c.nz == 1} == {(1, pz, to) for pz in BCS for to in TOS}
    assert {(c.b.shape[-2], c.pads[1]) for c in cases if c.b.shape[-2] == 1} == {(1, p) for p in BCS}
    assert {(c.b.shape[-1], c.pads[0]) for c in cases if c.b.shape[-1] == 1} == {(1, p) for p in BCS}


@pytest.mark.parametrize("nx", NXS)
def test_small_shapes(host_abi, monkeypatch, nx):
    cases = shape_cases(nx)
    assert len(cases) == len(NZS) * len(NYS)
    compare_with_numpy(cases)
    compare_with_chain(monkeypatch, cases)


# ---- 2. every boundary triple, metric forms, mid size ----------------------------------------------------------------------
LEAD_CASES = [((), 4, 5, 8, "planes"), ((2,), 3, 5, 6, "full"), ((2, 2), 3, 4, 5, "lead"), ((2, 2), 2, 3, 12, "planes")]


def matrix_cases(pads, dtype):
    """leading dims (), (2,), (2, 2) x both face positions, NaN or not, weighted or not and the fills rotating"""
    out = []
    for n, ((lead, nz, ny, nx, metric), to) in enumerate(itertools.product(LEAD_CASES, TOS)):
        out.append(Case(lead, nz, ny, nx, dtype, pads, to, metric, weighted=n % 3 != 2, fill=FILLS[n % 3], nan=n % 4 == 3))
    return out


@pytest.mark.parametrize("px,py,pz", PADS3)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_every_boundary_triple(host_abi, monkeypatch, px, py, pz, dtype):
    cases = matrix_cases((px, py, pz), dtype)
    assert compare_with_numpy(cases) >= 1
    compare_with_chain(monkeypatch, cases)


def metric_cases(dtype):
    """every metric form under every depth of leading dims, both face positions, and the unweighted call"""
    out = []
    for n, (metric, lead, to) in enumerate(itertools.product(METRICS, [(), (2,), (2, 2)], TOS)):
        out.append(Case(lead, 3, 4, 6, dtype, PADS3[(5 * n + 1) % 27], to, metric, fill=FILLS[n % 3], nan=n % 5 == 4))
    out += [Case((2,), 3, 4, 6, dtype, PADS3[(7 * n) % 27], to, metric, weighted=False) for n, (metric, to) in
            enumerate(itertools.product(METRICS[1:], TOS))]
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_metric_forms_and_leading_dims(host_abi, monkeypatch, dtype):
    cases = metric_cases(dtype)
    assert compare_with_numpy(cases) > 5
    compare_with_chain(monkeypatch, cases)


def mid_size_cases(dtype, nx):
    """several bands, ragged tiles and a ragged last segment together; nx = 515 takes the narrow form, 516 the vector form"""
    return [Case((2,), 7, 67, nx, dtype, ("periodic", "extend", "fill"), "outer", "full", nan=True),
            Case((2,), 7, 67, nx, dtype, ("fill", "periodic", "extend"), "left", "planes"),
            Case((2,), 7, 67, nx, dtype, ("extend", "fill", "periodic"), "outer", "planes")]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("nx", [515, 516])
def test_mid_size(host_abi, monkeypatch, dtype, nx):
    assert compare_with_numpy(mid_size_cases(dtype, nx), monkeypatch) == 2


# ---- 3. fills, NaNs, zero over zero -----------------------------------------------------------------------------------------
def fill_cases(dtype):
    """the three fill sets, -0.0 and NaN included, over an ordinary and an all-zero field, `fill` on one axis after the other
    and on all three"""
    out = []
    for fill, zero in itertools.product(FILLS, (False, True)):
        for pads in (("fill", "fill", "fill"), ("fill", "periodic", "extend"), ("extend", "fill", "periodic"), ("periodic", "extend", "fill")):
            for to, metric in (("outer", "planes"), ("left", None)):
                out.append(Case((2,), 3, 4, 6, dtype, pads, to, metric, fill=fill, zero=zero))
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_fills_keep_their_bits(host_abi, monkeypatch, dtype):
    cases = fill_cases(dtype)
    assert compare_with_numpy(cases, monkeypatch) == 8
    for c in cases:
        if c.zero:   # bz is 0 on every interior face, so 0 / 0 or x / 0: the module docstring's statement about these fields
            assert not any(np.isfinite(w[..., 1:c.nz, :, :]).any() for w in c.want()), c


NAN_AT = [(0, 0, 0), (4, 2, 3), (2, 5, 3), (2, 2, 7), (4, 5, 7), (2, 2, 3)]   # a corner, beside each pad, all pads, the middle


def check_nan_locality(to, pads):
    """one NaN at a time in b: NaN in the results exactly where the statement has it, and in the middle of the volume exactly
    at columns i-1 .. i+1 of sx and rows j-1 .. j+1 of sy at faces k and k + 1 (through bz: (k, k + 1; j, i) of both)"""
    for at in NAN_AT:
        c = Case((), 5, 6, 8, np.float64, pads, to, "planes")
        c.b.values[at] = np.nan
        (sx, sy), (wx, wy) = c.one_pass(), c.want()
        for g, w in ((sx, wx), (sy, wy)):
            assert np.array_equal(np.isnan(g.values), np.isnan(w)), (c, at)
            assert np.isnan(g.values).any() and not np.isnan(g.values).all()
        if at == NAN_AT[-1]:
            k, j, i = at
            mx_, my_ = np.zeros(sx.shape, bool), np.zeros(sy.shape, bool)
            mx_[k:k + 2, j, i - 1:i + 2] = True
            my_[k:k + 2, j - 1:j + 2, i] = True
            assert np.array_equal(np.isnan(sx.values), mx_) and np.array_equal(np.isnan(sy.values), my_), (c, at)


@pytest.mark.parametrize("to", TOS)
@pytest.mark.parametrize("pads", [("periodic", "periodic", "periodic"), ("extend", "fill", "fill"), ("fill", "extend", "extend")],
                         ids=lambda p: "-".join(p))
def test_a_nan_poisons_exactly_what_the_statement_has_as_nan(host_abi, to, pads):
    check_nan_locality(to, pads)


def zero_over_zero_cases(dtype):
    return [Case(lead, nz, 5, nx, dtype, (px, py, "extend"), "outer", metric)
            for (lead, nz, nx, metric), (px, py) in zip(
                [((), 4, 6, "planes"), ((2,), 3, 132, "full"), ((), 1, 8, None), ((2,), 5, 9, "lead")],
                [("periodic", "periodic"), ("extend", "periodic"), ("extend", "extend"), ("periodic", "extend")])]


def check_zero_over_zero(dtype):
    """`extend` on Z to "outer": bz is exactly 0 at faces 0 and nz, so both results are x / 0 or 0 / 0 there -- nothing
    finite -- and land exactly where the statement has them; every interior face is finite"""
    for c in zero_over_zero_cases(dtype):
        got, want = c.one_pass(), c.want()
        nz, seen = c.nz, set()
        for g, w in zip(got, want):
            outer = w[..., [0, nz], :, :]
            assert not np.isfinite(outer).any() and np.isfinite(w[..., 1:nz, :, :]).all(), c     # the reference
            seen |= {"nan"} if np.isnan(outer).any() else set()
            seen |= {"inf"} if np.isinf(outer).any() else set()
            assert np.array_equal(np.isnan(g.values), np.isnan(w)) and np.array_equal(np.isinf(g.values), np.isinf(w)), c
            _same_bits(g.values, w)
        assert "inf" in seen, c   # (x / 0; with one level under `extend` on X and Y every gradient is 0 too: 0 / 0 alone)
    c = Case((), 3, 4, 6, dtype, ("extend", "extend", "extend"), "outer", None)
    c.b = c.b._replace(data=np.broadcast_to(c.b.values[:, :1, :1], c.b.shape).copy())   # no horizontal gradient: 0 / 0
    for g, w in zip(c.one_pass(), c.want()):
        assert np.isnan(w[[0, 3]]).all() and (w[1:3] == 0).all()
        _same_bits(g.values, w)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_zero_over_zero_lands_where_the_statement_has_it(host_abi, dtype):
    check_zero_over_zero(dtype)


# ---- 4. labels, residency, defaults ----------------------------------------------------------------------------------------
def label_cases():
    cases = []
    for name in ("b", "dxC", "drCo", None, "hx", "hzo"):
        for metric, to in (("planes", "outer"), ("full", "outer"), ("full", "left"), (None, "left")):
            c = Case((2,), 3, 5, 6, np.float64, ("periodic", "extend", "fill"), to, metric)
            c.b = c.b._replace(name=name).assign_coords({"depth": (("ZC",), np.arange(3) * 10.0), "t2": (("time",), np.arange(2) + 9.0),
                                                         "lonC": (("YC", "XC"), np.ones((5, 6)))})
            cases.append(c)
    return cases


def test_coords_and_names_follow_the_chain(host_abi, monkeypatch):
    compare_with_chain(monkeypatch, label_cases())


def test_xarray_in_xarray_out(host_abi, monkeypatch):
    import xarray_standin
    from oracle import fake_device

    xarray_standin.install(monkeypatch)
    import xarray as xr

    c = Case((), 3, 4, 6, np.float64, ("periodic", "fill", "extend"), "left")
    got = c.grid.isopycnal_slope(xr.DataArray(c.b.values, dims=c.b.dims, name=c.b.name), **c.kw)
    assert len(got) == 2 and all(type(g).__module__.split(".")[0] == "xarray" for g in got)
    fake_device.install(monkeypatch)
    with np.errstate(all="ignore"):
        want = c.chain()
    for g, w in zip(got, want):
        assert tuple(g.dims) == tuple(w.dims) and g.name == w.name
        _same_bits(np.asarray(g.values), np.asarray(w.values))


def test_to_defaults_to_outer_when_the_axis_has_it_else_left(host_abi, monkeypatch):
    calls = _counted(monkeypatch)
    c = Case((), 3, 4, 6, np.float64, ("periodic", "fill", "extend"), "outer")
    sx, sy = c.grid.isopycnal_slope(c.b, fill_value=FILL)
    assert sx.dims == sy.dims == ("ZO", "YC", "XC") and isinstance(sx.data, np.ndarray)
    for g, w in zip((sx, sy), c.want()):
        _same_bits(g.values, w)
    axes = dict(AXES, Z={"center": "ZC", "left": "ZL"})
    ds = Dataset({k: (c.ds[k].dims, np.asarray(c.ds[k].values)) for k in ("dxC", "dyC", "drCl")},
                 {k: v for k, v in c.ds.coords.items() if k != "ZO"})
    g2 = Grid(ds, coords=axes, metrics={("X",): ["dxC"], ("Y",): ["dyC"], ("Z",): ["drCl"]}, padding=dict(zip("XYZ", c.pads)),
              autoparse_metadata=False)
    got = g2.isopycnal_slope(c.b)
    assert got[0].dims == ("ZL", "YC", "XC") and calls == {"fused": 2, "chain": 0}
    for g, w in zip(got, _want(c.b.values, c.pads, "left", {"X": 0.0, "Y": 0.0, "Z": 0.0}, *_metrics_of(c.ds, "planes", "left", ()))):
        _same_bits(g.values, w)


def test_a_boundary_given_with_the_call_is_served(host_abi, monkeypatch):
    calls = _counted(monkeypatch)
    grid, ds, dims = _grid((), 3, 5, 6, np.float64, {})
    c = Case((), 3, 5, 6, np.float64, ("fill", "periodic", "extend"), "outer")
    got = grid.isopycnal_slope(c.b, padding=dict(zip("XYZ", c.pads)), fill_value=FILL, to="outer")
    for g, w in zip(got, c.want()):
        _same_bits(g.values, w)
    assert calls == {"fused": 1, "chain": 0}


# ---- 5. seeded fuzz ---------------------------------------------------------------------------------------------------------
def fuzz_cases(seed=20261020, n=120):
    """cases over the small shapes, the boundary triples, both face positions, the fills, the dtype, the metric forms, the
    leading dims and all-zero fields; a third of them with NaNs"""
    rng = np.random.default_rng(seed)
    out = []
    for case in range(n):
        nz, ny, nx = (int(rng.choice(v)) for v in (NZS, NYS, NXS))
        lead = [(), (2,), (2, 2)][int(rng.integers(3))] if nx < 100 else ()
        pads = PADS3[case % 27] if case < 27 else tuple(str(rng.choice(BCS)) for _ in range(3))
        to = TOS[case % 2] if case < 54 else str(rng.choice(TOS))
        dtype = (np.float64, np.float32)[int(rng.integers(2))]
        metric = METRICS[int(rng.integers(4 if lead else 3))]
        out.append(Case(lead, nz, ny, nx, dtype, pads, to, metric, weighted=bool(rng.integers(4)), fill=FILLS[int(rng.integers(3))],
                        nan=bool(rng.integers(3) == 0), seed=500 + 3 * case, zero=bool(rng.integers(10) == 0)))
    return out


def test_seeded_fuzz(host_abi, monkeypatch):
    cases = fuzz_cases()
    assert len(cases) == 120 and compare_with_numpy(cases) >= 10
    compare_with_chain(monkeypatch, cases)


def test_the_tables_are_not_hollow():
    """the reference alone, over every table the CPU and the GPU suite run: no case breaks the statement of `not_hollow`, it
    is made often, and under every Z boundary"""
    tables = [shape_cases(nx) for nx in NXS] + [matrix_cases(p, dt) for p in PADS3 for dt in (np.float64, np.float32)]
    tables += [metric_cases(dt) + fill_cases(dt) for dt in (np.float64, np.float32)] + [fuzz_cases()]
    tables += [mid_size_cases(dt, nx) for dt in (np.float64, np.float32) for nx in (515, 516)]
    made = [c for t in tables for c in t if c.not_hollow(*c.want())]
    # (the boundary matrix alone: 27 triples x 2 dtypes x the 2 of 8 cases with the finite fill set and no NaN = 108)
    assert len(made) >= 108 and {c.pads[2] for c in made} == set(BCS) and {c.to for c in made} == set(TOS), len(made)


# ---- 6. every fallback of the docstring takes the chain ---------------------------------------------------------------------
def _no_fused(monkeypatch):
    import xgcm_amd.device as D

    monkeypatch.setattr(D, "isopycnal_slope", lambda *a, **k: pytest.fail("one-pass entry called"))


def _fallback_equals_chain(grid, b, **kw):
    with np.errstate(all="ignore"):
        for got, want in zip(grid.isopycnal_slope(b, **kw), _chain(grid, b, **kw)):
            _same_labelled(got, want)


def _case(pads=("periodic", "extend", "fill"), lead=(), nz=3, ny=5, nx=6, dtype=np.float64, to="outer", metric="planes", **kw):
    return Case(lead, nz, ny, nx, dtype, pads, to, metric, **kw)


@pytest.mark.parametrize("dtype", [np.int64, np.int32, np.float16])
def test_integer_and_half_fields_run_the_chain(backend, monkeypatch, dtype):
    _no_fused(monkeypatch)
    c = _case()
    b = DataArray((c.b.values * 100).astype(dtype), c.b.dims, name="b")
    for kw in (dict(), dict(metric_weighted=False, fill_value=FILL, to="left")):
        _fallback_equals_chain(c.grid, b, **kw)


def test_mixed_dtypes_run_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, dims = _grid((), 3, 5, 6, np.float32, {"X": "fill", "Y": "periodic", "Z": "extend"}, mdtype=np.float64)
    _fallback_equals_chain(grid, _field((), 3, 5, 6, np.float32, dims), fill_value=FILL)   # a float32 field over float64 metrics


def test_fewer_than_three_dims_or_z_elsewhere_run_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    c = _case(lead=(2,))
    _fallback_equals_chain(c.grid, c.b.transpose("ZC", "time", "YC", "XC"), fill_value=FILL)
    _fallback_equals_chain(c.grid, c.b.transpose("time", "YC", "ZC", "XC"), fill_value=FILL, metric_weighted=False)
    plane = DataArray(np.ascontiguousarray(c.b.values[0, 0]), ("YC", "XC"), name="b")   # no Z dim at all: what the chain raises
    _same_error(lambda: c.grid.isopycnal_slope(plane, metric_weighted=False), lambda: _chain(c.grid, plane, metric_weighted=False), own=AttributeError)


def test_b_elsewhere_runs_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    c = _case(lead=(2,))
    for dims in (("time", "ZC", "YC", "XG"), ("time", "ZC", "YG", "XC")):
        _fallback_equals_chain(c.grid, DataArray(c.b.values, dims, name="b"), fill_value=FILL, metric_weighted=False)


@pytest.mark.parametrize("to", ["right", "inner", "center", "nowhere"])
def test_other_targets_do_what_the_chain_does(backend, monkeypatch, to):
    _no_fused(monkeypatch)
    c = _case()
    _same_error(lambda: c.grid.isopycnal_slope(c.b, to=to), lambda: _chain(c.grid, c.b, to=to), own=AttributeError)


def test_a_position_the_axis_lacks_does_what_the_chain_does(backend, monkeypatch):
    _no_fused(monkeypatch)
    c = _case(to="left")
    axes = dict(AXES, Z={"center": "ZC", "left": "ZL"})
    ds = Dataset({k: (c.ds[k].dims, np.asarray(c.ds[k].values)) for k in ("dxC", "dyC", "drCl")},
                 {k: v for k, v in c.ds.coords.items() if k != "ZO"})
    g2 = Grid(ds, coords=axes, metrics={("X",): ["dxC"], ("Y",): ["dyC"], ("Z",): ["drCl"]}, padding=dict(zip("XYZ", c.pads)),
              autoparse_metadata=False)
    _same_error(lambda: g2.isopycnal_slope(c.b, to="outer"), lambda: _chain(g2, c.b, to="outer"), own=AttributeError)


def test_a_chunked_b_runs_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    c = _case(lead=(4,), ny=6, nx=8)
    b = DataArray(BlockArray.from_array(c.b.values, ((2, 2), (3,), (6,), (8,))), c.b.dims, name="b")
    with np.errstate(all="ignore"):
        got, want = c.grid.isopycnal_slope(b, fill_value=FILL), _chain(c.grid, b, fill_value=FILL)
    for g, w, p in zip(got, want, c.want()):
        assert g.dims == w.dims and g.name == w.name
        assert np.array_equal(np.asarray(g.values), np.asarray(w.values), equal_nan=True)
        assert np.array_equal(np.asarray(g.values), p, equal_nan=True)


def test_a_chunked_metric_runs_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    c = _case(nz=4, metric="full", to="left")
    coords = {k: (k, np.asarray(c.ds.coords[k].values)) for k in ("XC", "XG", "YC", "YG", "ZC", "ZL", "ZO")}
    for chunked in ("hx", "hy", "hzl"):
        data = {k: (c.ds[k].dims, BlockArray.from_array(np.asarray(c.ds[k].values), ((2, 2), (5,), (6,))) if k == chunked
                    else np.asarray(c.ds[k].values)) for k in ("hx", "hy", "hzl")}
        g2 = Grid(Dataset(data, coords), coords=AXES, metrics={("X",): ["hx"], ("Y",): ["hy"], ("Z",): ["hzl"]},
                  padding=dict(zip("XYZ", c.pads)), autoparse_metadata=False)
        kw = dict(to="left", fill_value=FILL)
        with np.errstate(all="ignore"):
            got, want = g2.isopycnal_slope(c.b, **kw), _chain(g2, c.b, **kw)
        for g, w, p in zip(got, want, c.want()):
            assert g.dims == w.dims and g.name == w.name
            assert np.array_equal(np.asarray(g.values), np.asarray(w.values), equal_nan=True)
            assert np.array_equal(np.asarray(g.values), p, equal_nan=True)


@pytest.mark.parametrize("axis", ["X", "Y", "Z"])
def test_a_metric_with_an_extra_dim_runs_the_chain(backend, monkeypatch, axis):
    _no_fused(monkeypatch)
    c = _case()
    coords = {k: (k, np.asarray(c.ds.coords[k].values)) for k in ("XC", "XG", "YC", "YG", "ZC", "ZL", "ZO")}
    coords["time"] = ("time", np.arange(2) * 2.0)
    data = {k: (c.ds[k].dims, np.asarray(c.ds[k].values)) for k in ("dxC", "dyC", "drCo")}
    name = {"X": "dxC", "Y": "dyC", "Z": "drCo"}[axis]
    dims = data[name][0]
    data[name] = (dims + ("time",), R.synthetic_metric(tuple(len(coords[d][1]) for d in dims) + (2,), 66))
    g2 = Grid(Dataset(data, coords), coords=AXES, metrics={("X",): ["dxC"], ("Y",): ["dyC"], ("Z",): ["drCo"]},
              padding=dict(zip("XYZ", c.pads)), autoparse_metadata=False)
    with np.errstate(all="ignore"):
        got, want = g2.isopycnal_slope(c.b, fill_value=FILL), _chain(g2, c.b, fill_value=FILL)
    for g, w in zip(got, want):
        _same_labelled(g, w)
    assert "time" in got["XYZ".index(axis) % 2].dims


@pytest.mark.parametrize("missing", ["X", "Y", "Z", "all"])
def test_a_missing_metric_raises_the_chains_error(backend, monkeypatch, missing):
    _no_fused(monkeypatch)
    c = _case()
    names = {"X": ["dxC"], "Y": ["dyC"], "Z": ["drCl", "drCo"]}
    g2 = Grid(c.ds, coords=AXES, metrics={(ax,): v for ax, v in names.items() if ax != missing and missing != "all"},
              padding=dict(zip("XYZ", c.pads)), autoparse_metadata=False)
    _same_error(lambda: g2.isopycnal_slope(c.b), lambda: _chain(g2, c.b))


def test_a_missing_metric_is_still_served_unweighted(host_abi, monkeypatch):
    c = _case(metric=None)
    c.kw["metric_weighted"] = False
    compare_with_chain(monkeypatch, [c])


@pytest.mark.parametrize("axis", ["X", "Y", "Z"])
def test_an_axis_without_a_boundary_raises_the_chains_error(backend, monkeypatch, axis):
    _no_fused(monkeypatch)
    pad = {"X": "periodic", "Y": "extend", "Z": "fill"}
    del pad[axis]
    grid, ds, dims = _grid((), 3, 5, 6, np.float64, pad)
    b = _field((), 3, 5, 6, np.float64, dims)
    _same_error(lambda: grid.isopycnal_slope(b), lambda: _chain(grid, b))


def test_a_field_without_a_level_does_what_the_chain_does(backend, monkeypatch):
    _no_fused(monkeypatch)
    c = _case()
    b = DataArray(np.zeros((0, 5, 6)), c.b.dims, name="b")
    kw = dict(fill_value=FILL, metric_weighted=False, to="left")
    try:
        want = _chain(c.grid, b, **kw)
    except Exception:
        _same_error(lambda: c.grid.isopycnal_slope(b, **kw), lambda: _chain(c.grid, b, **kw), own=AttributeError)
    else:
        for g, w in zip(c.grid.isopycnal_slope(b, **kw), want):
            _same_labelled(g, w)


@pytest.mark.parametrize("conn", ["x2x", "y2y", "z2z"])
def test_connected_faces_run_the_chain(backend, monkeypatch, conn):
    from test_topology import COORDS, X_TO_X

    _no_fused(monkeypatch)
    ds = Dataset({"drC": (("zo",), R.synthetic_metric((5,), 63)), "dxC": (("y", "xl"), R.synthetic_metric((4, 4), 61)),
                  "dyC": (("yl", "x"), R.synthetic_metric((4, 4), 62))},
                 coords={"x": np.arange(4), "xl": np.arange(4) - 0.5, "y": np.arange(4), "yl": np.arange(4) - 0.5,
                         "face": np.arange(2), "zc": np.arange(4) + 0.5, "zo": np.arange(5) * 1.0})
    grid = Grid(ds, coords=dict(COORDS, Z={"center": "zc", "outer": "zo"}), metrics={("X",): ["dxC"], ("Y",): ["dyC"], ("Z",): ["drC"]},
                face_connections={"x2x": X_TO_X, "y2y": TR.Y_TO_Y, "z2z": TR.Z_TO_Z}[conn],
                padding={"X": "fill", "Y": "extend", "Z": "fill"}, autoparse_metadata=False)
    b = DataArray(R.synthetic_field((2, 4, 4, 4), 81), ("face", "zc", "y", "x"), name="f")
    for mw in (True, False):
        _fallback_equals_chain(grid, b, fill_value=FILL, metric_weighted=mw)


def test_fold_grid_runs_the_chain(backend, monkeypatch):
    import warnings

    from test_topology import Nx, Ny

    _no_fused(monkeypatch)
    ds = Dataset({"drC": (("zo",), R.synthetic_metric((3,), 63))},
                 coords={"xh": np.arange(Nx), "xl": np.arange(Nx), "yh": np.arange(Ny), "yl": np.arange(Ny),
                         "zc": np.arange(2) + 0.5, "zo": np.arange(3) * 1.0})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        grid = Grid(ds, coords={"X": {"center": "xh", "left": "xl"}, "Y": {"center": "yh", "left": "yl"},
                                "Z": {"center": "zc", "outer": "zo"}}, metrics={("Z",): ["drC"]},
                    padding={"X": "periodic", "Y": {"fold": "corner"}, "Z": "fill"}, autoparse_metadata=False)
        b = DataArray(R.synthetic_field((2, Ny, Nx), 91), ("zc", "yh", "xh"))
        _fallback_equals_chain(grid, b, metric_weighted=False)


# ---- 7. the entry of the C ABI called directly, with views ------------------------------------------------------------------
def _abi_call(D, dtype, shape, b, planes, k, offs=(ALIGNED, ALIGNED)):
    """one call of xg_isopycnal_slope: `b` a view, `planes` {mx, my, mz} views; each result is written `offs[n]` elements into
    an allocation of its own full of SENTINEL, which must still surround it afterwards"""
    (px, py, pz), to = TR.ABI_PADS[k]
    fshape = shape[:-3] + [TR._nf(shape[-3], to)] + shape[-2:]
    args = [TR.CODE[dtype], b.data_ptr()]
    for name, against in (("mx", shape), ("my", shape), ("mz", fshape)):
        m = planes.get(name)
        if m is None:
            args += [None, None]
        else:
            assert all(n in (1, s) for n, s in zip(m.shape, against))
            args += [m.data_ptr(), _hip.i64([0 if n == 1 else m.stride(d) for d, n in enumerate(m.shape)])]
    n = int(np.prod(fshape))
    bufs = [torch.full((off + n + ALIGNED,), TR.SENTINEL, dtype=TR.TORCH[dtype], device=D._MEM.device) for off in offs]
    args += [buf[off:off + n].data_ptr() for buf, off in zip(bufs, offs)]
    args += [_hip.i64(shape), len(shape), int(to == "outer"), _hip.BC[px], FILL["X"], _hip.BC[py], FILL["Y"], _hip.BC[pz], FILL["Z"]]
    D._check(D._MEM.lib().xg_isopycnal_slope(*args, D._stream()))
    res = []
    for buf, off in zip(bufs, offs):
        whole = buf.cpu().numpy()
        assert (whole[:off] == TR.SENTINEL).all() and (whole[off + n:] == TR.SENTINEL).all()
        res.append(whole[off:off + n].reshape(fshape))
    return res


def abi_layout_cases(dtype):
    """Runs the direct-ABI table on whatever library `xgcm_amd.device._MEM` serves.  Every input view lives in a NaN-filled
    allocation, so a read outside it shows in the results; the contiguous, aligned control of each set of planes is compared
    with the numpy statement, every other layout with that control.  Result offsets: 0, 16 bytes and one element."""
    import xgcm_amd.device as D

    shape = [2, 5, 7, TR.ABI_NX[dtype]]
    lead, nz, ny, nx = shape
    bv = R.synthetic_field(tuple(shape), 101).astype(dtype)
    bv.reshape(-1)[5::97] = np.nan
    put = lambda a, st=None, off=ALIGNED: _strided(D, a, st or _contig(a.shape), off)  # noqa: E731
    same = lambda got, want: [_same_bits(g, w) for g, w in zip(got, want)]  # noqa: E731
    sixteen = 16 // np.dtype(dtype).itemsize
    for k, ((px, py, pz), to) in enumerate(TR.ABI_PADS):
        nf = TR._nf(nz, to)
        levels = {"mx": nz, "my": nz, "mz": nf}
        form = lambda f, n: {"z": (1, n, 1, 1), "p": (1, 1, ny, nx), "v3": (1, n, ny, nx), "vl": (lead, n, ny, nx)}[f]  # noqa: E731
        val = lambda name, f: R.synthetic_metric(form(f, levels[name]), 111 + "zpv3vl".index(f) + ord(name[1])).astype(dtype)  # noqa: E731
        b = put(bv)
        assert b.is_contiguous() and b.data_ptr() % 16 == 0
        for present in ({"mx": "p"}, {"my": "p"}, {"mz": "z"}, {"mx": "p", "my": "p", "mz": "z"}, {"mx": "v3", "my": "vl", "mz": "v3"},
                        {"mx": "vl", "my": "z", "mz": "p"}, {"mx": "z", "my": "v3", "mz": "vl"}, {}):
            pv = {n: val(n, f) for n, f in present.items()}
            aligned = {n: put(a) for n, a in pv.items()}
            control = _abi_call(D, dtype, shape, b, aligned, k)
            want = _want(bv, (px, py, pz), to, FILL, pv.get("mx"), pv.get("my"), pv.get("mz"))
            assert control[0].dtype == want[0].dtype == np.dtype(dtype)
            same(control, want)
            assert not np.isnan(want[0]).all() and np.isfinite(want[0]).any() and (want[0] != want[1]).any()
            views = [(put(bv, off=1), aligned, (ALIGNED, ALIGNED))]     # b one element in: the narrow form
            assert views[0][0].data_ptr() % 16 == np.dtype(dtype).itemsize
            views += [(b, aligned, offs) for offs in ((0, 0), (sixteen, sixteen), (1, ALIGNED), (ALIGNED, 1), (1, 1), (0, sixteen))]
            # the planes one element in; with an odd row pitch; with an odd level pitch (volumes)
            views.append((b, {n: put(a, off=1) for n, a in pv.items()}, (ALIGNED, ALIGNED)))
            pitched = {}
            for n, a in pv.items():
                s = list(a.shape)
                pitched[n] = put(a, _contig(s[:-1] + [s[-1] + 1]) if s[-1] > 1 else _contig(s))
                assert s[-1] == 1 or (pitched[n].stride(-2) == nx + 1 and pitched[n].stride(-1) == 1)
            views.append((b, pitched, (ALIGNED, ALIGNED)))
            for n, f in present.items():
                a, nl = pv[n], levels[n]
                if f in ("v3", "vl"):
                    st = [(nl * (ny * nx + 1)) * (a.shape[0] > 1), ny * nx + 1, nx, 1]
                    lev = put(a, [s or 1 for s in st])
                    assert lev.stride(1) == ny * nx + 1
                    views.append((b, dict(aligned, **{n: lev}), (ALIGNED, ALIGNED)))
                if f == "z":   # the Z-only metric three elements apart
                    views.append((b, dict(aligned, **{n: put(a, [3 * nl, 3, 1, 1], 1)}), (ALIGNED, ALIGNED)))
                if f == "p":   # the plane stored (X, Y): a transposed view
                    t = put(np.ascontiguousarray(a.transpose(0, 1, 3, 2))).permute(0, 1, 3, 2)
                    assert t.stride(-1) == ny and t.stride(-2) == 1
                    views.append((b, dict(aligned, **{n: t}), (ALIGNED, ALIGNED)))
            for b_, planes, offs in views:
                same(_abi_call(D, dtype, shape, b_, planes, k, offs), control)
        # stride-0 metrics along X and Y: one value per level, expanded over the whole volume, equal the Z-only metrics
        flat = {n: put(val(n, "z")).expand(1, levels[n], ny, nx) for n in levels}
        assert all(m.stride(-1) == 0 and m.stride(-2) == 0 for m in flat.values())
        full = {n: put(np.ascontiguousarray(np.broadcast_to(val(n, "z"), (1, levels[n], ny, nx)))) for n in levels}
        same(_abi_call(D, dtype, shape, b, flat, k), _abi_call(D, dtype, shape, b, full, k))
    assert nx % TR.NVS[dtype] == 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_abi_layouts(host_abi, dtype):
    abi_layout_cases(dtype)


def abi_bad_calls():
    """bad calls return an error code, write nothing and leave the process alone; runs on whatever library `_MEM` serves"""
    import xgcm_amd.device as D

    lib = D._MEM.lib()
    shape = [2, 3, 4]
    t = torch.ones(shape, dtype=torch.float64, device=D._MEM.device)
    outs = [torch.full([3, 3, 4], TR.SENTINEL, dtype=torch.float64, device=D._MEM.device) for _ in range(2)]   # room for Z:outer
    P = lambda x: None if x is None else x.data_ptr()  # noqa: E731

    def call(code=TR.CODE[np.float64], b=t, o=outs, shape=shape, ndim=3, outer=0, bcx=_hip.BC["periodic"], bcy=_hip.BC["extend"],
             bcz=_hip.BC["fill"], mets=(None, None, None), strides=(None, None, None)):
        margs = [x for pair in zip(mets, strides) for x in pair]
        return lib.xg_isopycnal_slope(code, P(b), *margs, P(o[0]), P(o[1]), None if shape is None else _hip.i64(shape), ndim,
                                      outer, bcx, 0.0, bcy, 0.0, bcz, 0.0, D._stream())

    untouched = lambda: all(bool((o == TR.SENTINEL).all()) for o in outs)  # noqa: E731
    for code in (-1, _hip.DTYPE["float16"], _hip.DTYPE["int64"], _hip.DTYPE["int32"], 12, 99):
        assert call(code=code) == -1                              # any other element type: XG_ERR_INVALID
    assert call(b=None) == -1 and call(shape=None) == -1          # NULL arguments
    assert call(o=[None, outs[1]]) == -1 and call(o=[outs[0], None]) == -1          # a NULL result
    assert call(bcx=7) == -1 and call(bcy=-1) == -1 and call(bcz=9) == -1           # unknown boundary codes
    assert call(outer=2) == -1 and call(outer=-1) == -1           # unknown face position
    assert call(shape=[0, 3, 4]) == -1                            # nz = 0: no level to pad from
    for k in range(3):                                            # a metric without strides, each of the three
        assert call(mets=tuple(t.data_ptr() if j == k else None for j in range(3))) == -1
    assert call(ndim=2) < 0 and call(ndim=2) != -1                # XG_ERR_UNSUPPORTED
    assert untouched()
    assert call(shape=[2, 0, 4]) == 0 and call(shape=[2, 3, 0]) == 0 and untouched()   # an empty plane: nothing to do
    assert call() == 0 and call(bcz=_hip.BC["periodic"], outer=1) == 0 and call(bcz=_hip.BC["extend"], outer=1) == 0
    assert not untouched()


def test_abi_refuses_bad_calls(host_abi):
    abi_bad_calls()


def test_empty_results_return_without_a_launch(host_abi, monkeypatch):
    import xgcm_amd.device as D

    monkeypatch.setattr(D, "_check", lambda rc: pytest.fail("the library was called for an empty result"))
    for shape in ((2, 3, 0, 4), (0, 3, 5, 4), (3, 5, 0)):
        sx, sy = D.isopycnal_slope(np.zeros(shape), None, None, None, True, "periodic", "fill", "extend")
        assert tuple(sx.shape) == tuple(sy.shape) == shape[:-3] + (shape[-3] + 1,) + shape[-2:] and sx.numel() == 0


# ---- 8. the tunable call table, between guard bands -------------------------------------------------------------------------
def tunable_calls(D, dtype):
    """(calls, references) of the K7q tunable sweep: name -> thunk that calls `D` on inputs uploaded once, name -> thunk that
    gives numpy's pair of results of the same call.  The battery's own shapes, both face positions; planes with a profile,
    three volumes, and no metric"""
    f = lambda shape, seed: R.synthetic_field(shape, seed).astype(dtype)  # noqa: E731
    m = lambda shape, seed: R.synthetic_metric(shape, seed).astype(dtype)  # noqa: E731
    calls, references = {}, {}
    for n, shape in enumerate(((5, 300, 264), (3, 65, 131))):
        nz, ny, nx = shape
        b = f(shape, 150 + n)
        b[1, 7, 9] = b[0, 0, 0] = b[nz - 1, ny - 1, nx - 1] = np.nan
        dev = D.asdevice(b)
        for k, (to, pads) in enumerate((("left", ("periodic", "extend", "fill")), ("outer", ("extend", "fill", "periodic")),
                                        ("left", ("fill", "periodic", "extend")), ("outer", ("periodic", "periodic", "fill")))):
            nf = nz + (to == "outer")
            if k % 2:
                mets = [m((1, ny, nx), 170), m((1, ny, nx), 171), m((nf, 1, 1), 172)]
            else:
                mets = [m((nz, ny, nx), 173), m((nz, ny, nx), 174), m((nf, ny, nx), 175)]
            if k == 2:
                mets = [None, None, None]
            dm = tuple(None if x is None else D.asdevice(x) for x in mets)
            key = f"{nx}{to}{pads[2]}"
            fill = [FILL[a] for a in "XYZ"]
            calls[key] = lambda dev=dev, dm=dm, to=to, pads=pads: D.isopycnal_slope(dev, *dm, to == "outer", *pads, *fill)
            references[key] = lambda h=b, mets=mets, to=to, pads=pads: list(_want(h, pads, to, FILL, *mets))
    return calls, references


def _bits_equal(got, want):
    try:
        _same_bits(got, want)
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_the_tunable_call_table_equals_its_numpy_references(host_abi, dtype):
    """the thunks the GPU suite sweeps over every tunable value, once through the host build (which reads no tunable): the
    arguments, their order, the shapes and the references are checked before any GPU time is spent on them"""
    import xgcm_amd.device as D

    calls, references = tunable_calls(D, dtype)
    assert len(calls) == 8 and set(calls) == set(references)
    for name, thunk in calls.items():
        got, want = [D.tohost(x) for x in thunk()], references[name]()
        assert len(got) == len(want) == 2, name
        for g, w in zip(got, want):
            assert g.dtype == np.dtype(dtype) and np.isnan(w).any() and np.isnan(w).mean() < 0.01, name
            assert _bits_equal(g, w), name
        assert (want[0] != want[1]).any()


def guarded_table(D, monkeypatch, dtype, offset, same_bits):
    """the table built and run between guard bands: a store outside either result, a cell left unwritten and a
    result-changing read outside the field or a metric all fail; returns the number of results checked"""
    checked = 0
    with GM.guarded(D, monkeypatch, offset) as g:
        calls, references = tunable_calls(D, dtype)
        assert g.placed >= 2 + 2 * 3 * 3          # the field of both shapes, the metrics of the calls that have them
        for k, fn in calls.items():
            before = g.handed_out
            got = [D.tohost(x) for x in fn()]
            g.check(f"{k} at offset {offset}")
            assert g.handed_out - before >= 2     # both results between guards
            for x, want in zip(got, references[k]()):
                assert same_bits(x, want), f"{k} at offset {offset}: not numpy's result"
                checked += 1
    return checked


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_between_guard_bands_through_the_host_abi(host_abi, monkeypatch, dtype):
    import xgcm_amd.device as D

    for offset in (0, 16, np.dtype(dtype).itemsize):
        assert guarded_table(D, monkeypatch, dtype, offset, _bits_equal) == 16
