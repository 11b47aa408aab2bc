"""The squared vertical shear and the gradient Richardson number at the faces of Z, `Grid.vertical_shear_squared` and
`Grid.richardson_number`, on CPU.

The one-pass path runs through the `host_abi` fixture (the product's `xgcm_amd.device` over libxgcm_host.so); the chain it
replaces

    step = grid.derivative | grid.diff
    uz = grid.interp(step(u, Z, to), X);  vz = grid.interp(step(v, Z, to), Y);  s2 = uz * uz + vz * vz;  ri = step(b, Z, to) / s2

runs through the same Grid over the oracle double, installed AFTER the one-pass calls of a test have run (the double
replaces `asdevice`, which the one-pass entry needs as the product's own).  Values are compared bit for bit (NaN = NaN), with
dims, coords and names.  `_want` states the same chain a third time, over plain numpy arrays with the oracle's one-axis
functions.  The fallbacks only call existing device functions and run under the `backend` double.  The case builders and the
direct-ABI cases are shared with the GPU suite.

Ri is NaN by construction wherever both differences vanish (the outermost faces under `extend` with "outer", everything for
one level under `periodic` or `extend`), so every case also runs `vertical_shear_squared`, and `Case.not_hollow` asserts on the
reference itself that S2 has no NaN and, under `fill` on Z with two levels or more, that Ri is finite on every interior face
-- in the cases without an injected NaN and without a NaN fill value."""

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
FILL = {"X": 1.75, "Y": -0.625, "Z": 0.375}
FILLS = [FILL, {"X": -0.0, "Y": float("nan"), "Z": -0.0}, {"X": float("nan"), "Y": -0.0, "Z": float("nan")}]
AXES = {"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"},
        "Z": {"center": "ZC", "left": "ZL", "outer": "ZO"}}
ZDIM = {"left": "ZL", "outer": "ZO"}
POINTS = (("YC", "XG"), ("YG", "XC"), ("YC", "XC"))    # the rows and columns of u, of v, of b
PADS3 = list(itertools.product(BCS, BCS, BCS))
METRICS = [None, "1d", "full", "lead"]
_same_labelled = TV._same_labelled


def _nf(nz, to):
    return nz + (to == "outer")


def _grid(lead, nz, ny, nx, dtype, padding, metric="1d", axes=AXES, mdtype=None):
    """C-grid with a Z axis that has a left and an outer position.  Z metrics: "1d" -- drCl(ZL), drCo(ZO); "full" --
    thicknesses (Z, Y, X) at u's points, at v's points and at the centre for both face positions (hW, hS, hC + l | o); "lead":
    the same with the first leading dim in front; None: no Z metric at all"""
    dims = ("time", "member")[:len(lead)]
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0),
              "YC": ("YC", np.arange(ny) + 0.5), "YG": ("YG", np.arange(ny) * 1.0),
              "ZC": ("ZC", np.arange(nz) + 0.5), "ZL": ("ZL", np.arange(nz) * 1.0), "ZO": ("ZO", np.arange(nz + 1) * 1.0)}
    for d, n in zip(dims, lead):
        coords[d] = (d, np.arange(n) * 2.0)
    m = lambda shape, seed: R.synthetic_metric(shape, seed).astype(mdtype or dtype)  # noqa: E731
    data = {}
    if metric == "1d":
        data["drCl"] = (("ZL",), m((nz,), 63))
        data["drCo"] = (("ZO",), m((nz + 1,), 64))
    elif metric is not None:
        pl, pd = ((lead[0],), dims[:1]) if metric == "lead" and lead else ((), ())
        for k, (to, n) in enumerate((("left", nz), ("outer", nz + 1))):
            for j, (name, hpos) in enumerate(zip(("hW", "hS", "hC"), POINTS)):
                data[name + to[0]] = (pd + (ZDIM[to],) + hpos, m(pl + (n, ny, nx), 66 + 3 * k + j))
    ds = Dataset(data, coords)
    grid = Grid(ds, coords=axes, metrics={("Z",): list(data)} if data else {}, padding=padding, autoparse_metadata=False)
    return grid, ds, dims


def _fields(lead, nz, ny, nx, dtype, dims, nan=False, seed=71):
    """(b, u, v) at their C-grid points"""
    shape = tuple(lead) + (nz, ny, nx)
    b, u, v = (R.synthetic_field(shape, seed + k).astype(dtype) for k in range(3))
    if nan:
        b.reshape(-1)[3::11] = np.nan
        u.reshape(-1)[5::13] = np.nan
        v[..., :, ny // 2, nx // 2] = np.nan   # a column of v that is all NaN
        v[..., 0, 0, 0] = np.nan               # a NaN in level 0, beside the Z pad
        u[..., nz - 1, ny - 1, nx - 1] = np.nan
    return (DataArray(b, dims + ("ZC", "YC", "XC"), name="b"), DataArray(u, dims + ("ZC", "YC", "XG"), name="u"),
            DataArray(v, dims + ("ZC", "YG", "XC"), name="v"))


def _chain(grid, b, u, v, x_axis="X", y_axis="Y", z_axis="Z", to=None, padding=None, fill_value=None, metric_weighted=True):
    """the specification; b None: the squared shear"""
    kw = dict(padding=padding, fill_value=fill_value)
    step = grid.derivative if metric_weighted else grid.diff
    if to is None:   # the operators' default: Z:outer when the axis has that position, else Z:left
        to = "outer" if "outer" in grid.axes[z_axis].coords else "left"
    uz = grid.interp(step(u, z_axis, to=to, **kw), x_axis, **kw)
    vz = grid.interp(step(v, z_axis, to=to, **kw), y_axis, **kw)
    s2 = uz * uz + vz * vz
    return s2 if b is None else step(b, z_axis, to=to, **kw) / s2


def _aligned(da, dims):
    """the values of `da` as a numpy array that broadcasts against an array of `dims`"""
    v = np.asarray(da.values)
    present = [d for d in dims if d in da.dims]
    v = np.transpose(v, [da.dims.index(d) for d in present])
    return v[tuple(slice(None) if d in da.dims else np.newaxis for d in dims)]


def _want(b, u, v, pads, to, fill=FILL, mu=None, mv=None, mb=None):
    """the chain over plain numpy arrays, from the oracle's one-axis functions (the metrics broadcast against the faces)"""
    px, py, pz = pads
    z, y, x = u.ndim - 3, u.ndim - 2, u.ndim - 1
    hi = 1 if to == "outer" else 0
    uz = R.stencil1d("interp", R.stencil1d("diff", u, z, 1, hi, pz, fill["Z"], m_out=mu), x, 0, 1, px, fill["X"])
    vz = R.stencil1d("interp", R.stencil1d("diff", v, z, 1, hi, pz, fill["Z"], m_out=mv), y, 0, 1, py, fill["Y"])
    s2 = R.binary("add", R.binary("mul", uz, uz), R.binary("mul", vz, vz))
    if b is None:
        return s2
    with np.errstate(divide="ignore", invalid="ignore"):
        return R.binary("div", R.stencil1d("diff", b, z, 1, hi, pz, fill["Z"], m_out=mb), s2)


def _metrics_of(ds, metric, to, dims):
    """(mu, mv, mb) of `_grid` as numpy arrays that broadcast against the faces of fields with leading dims `dims`"""
    if metric is None:
        return None, None, None
    if metric == "1d":
        m = _aligned(ds["drC" + to[0]], dims + (ZDIM[to], "YC", "XC"))
        return m, m, m
    return tuple(_aligned(ds[name + to[0]], dims + (ZDIM[to],) + hpos) for name, hpos in zip(("hW", "hS", "hC"), POINTS))


class Case:
    """one call of both operators: the grid, its dataset and metric form, (b, u, v), the keywords and the boundary triple"""

    def __init__(self, lead, nz, ny, nx, dtype, pads, to, metric="1d", weighted=True, fill=FILL, nan=False, seed=71):
        self.pads, self.to, self.metric, self.nan = tuple(pads), to, metric, nan
        self.grid, self.ds, self.dims = _grid(lead, nz, ny, nx, dtype, dict(zip("XYZ", pads)), metric=metric)
        self.f = _fields(lead, nz, ny, nx, dtype, self.dims, nan=nan, seed=seed)
        self.kw = dict(to=to, fill_value=fill, metric_weighted=bool(weighted and metric is not None))
        self.nz = nz

    def __repr__(self):
        return (f"{self.f[0].shape} {np.dtype(self.f[0].values.dtype)} {self.pads} {self.to} metric {self.metric} "
                f"nan {self.nan} {self.kw}")

    def one_pass(self):
        return self.grid.richardson_number(*self.f, **self.kw), self.grid.vertical_shear_squared(*self.f[1:], **self.kw)

    def chain(self):
        return _chain(self.grid, *self.f, **self.kw), _chain(self.grid, None, *self.f[1:], **self.kw)

    def want(self):
        """(ri, s2) of the numpy statement"""
        fill = self.kw["fill_value"] or {"X": 0.0, "Y": 0.0, "Z": 0.0}
        mets = _metrics_of(self.ds, self.metric if self.kw["metric_weighted"] else None, self.to, self.dims)
        b, u, v = (a.values for a in self.f)
        return (_want(b, u, v, self.pads, self.to, fill, *mets), _want(None, u, v, self.pads, self.to, fill, *mets[:2]))

    def not_hollow(self, ri, s2):
        """asserted on the REFERENCE: without an injected NaN and without a NaN fill, S2 has no NaN and, under `fill` on Z
        with two levels or more, Ri is finite on every interior face"""
        fill = self.kw["fill_value"] or {}
        if self.nan or any(np.isnan(x) for x in fill.values()):
            return 0
        ri, s2 = np.asarray(ri), np.asarray(s2)
        assert not np.isnan(s2).any(), self
        if self.pads[2] == "fill" and self.nz >= 2:
            assert np.isfinite(ri[..., 1:self.nz, :, :]).all(), self
            return 1
        return 0


def _counted(monkeypatch):
    """the calls of the one-pass device entry: True for each Richardson number, False for each squared shear"""
    import xgcm_amd.device as D

    calls = []
    real = D.richardson_number
    monkeypatch.setattr(D, "richardson_number", lambda b, *a, **k: (calls.append(b is not None), real(b, *a, **k))[1])
    return calls


def _compare_with_chain(monkeypatch, cases):
    """every one-pass call first (counted), then the chain over the oracle double; returns the number of non-hollow cases"""
    from oracle import fake_device

    calls = _counted(monkeypatch)
    got = [c.one_pass() for c in cases]
    assert calls == [True, False] * len(cases)
    fake_device.install(monkeypatch)
    solid = 0
    for c, (ri, s2) in zip(cases, got):
        with np.errstate(divide="ignore", invalid="ignore"):
            want_ri, want_s2 = c.chain()
        try:
            _same_labelled(ri, want_ri)
            _same_labelled(s2, want_s2)
        except AssertionError as err:
            raise AssertionError(f"case {c}") from err
        solid += c.not_hollow(want_ri.values, want_s2.values)
    return solid


def _same_bits(got, want):
    """NaN where the other is NaN; everywhere else the same bit pattern, so that -0.0 is not +0.0"""
    g, w = np.asarray(got), np.asarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan)
    bits = {4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
    assert np.array_equal(np.where(nan, 0, g).view(bits), np.where(nan, 0, w).view(bits))


def compare_with_numpy(cases):
    """both operators of every case against the numpy statement, bit for bit; on whatever library `_MEM` serves"""
    solid = 0
    for c in cases:
        (ri, s2), (want_ri, want_s2) = c.one_pass(), c.want()
        try:
            _same_bits(ri.values, want_ri)
            _same_bits(s2.values, want_s2)
            assert ri.dims == s2.dims == c.dims + (ZDIM[c.to], "YC", "XC")
        except AssertionError as err:
            raise AssertionError(f"case {c}") from err
        solid += c.not_hollow(want_ri, want_s2)
    return solid


# (lead, nz, ny, nx, metric form): the lead / metric cases of the boundary matrix
LEAD_CASES = [((), 4, 5, 8, "1d"), ((2,), 3, 5, 6, "full"), ((2, 2), 3, 4, 5, "lead"), ((3,), 5, 3, 12, "lead")]


def matrix_cases(pads, dtype):
    """LEAD_CASES x both face positions, NaN or not, weighted or not and the fills rotating"""
    out = []
    for n, ((lead, nz, ny, nx, metric), to) in enumerate(itertools.product(LEAD_CASES, TOS)):
        out.append(Case(lead, nz, ny, nx, dtype, pads, to, metric, weighted=n % 3 != 2, fill=FILLS[n % 3], nan=n % 4 == 3))
    return out


# ---- 1. the one-pass result equals the chain ------------------------------------------------------------------------------
@pytest.mark.parametrize("px,py,pz", PADS3)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_equals_the_chain(host_abi, monkeypatch, px, py, pz, dtype):
    solid = _compare_with_chain(monkeypatch, matrix_cases((px, py, pz), dtype))
    assert solid >= (2 if pz == "fill" else 0)


@pytest.mark.parametrize("px,py,pz", PADS3[::2])
def test_equals_the_numpy_statement(host_abi, px, py, pz):
    for dtype in (np.float64, np.float32):
        compare_with_numpy(matrix_cases((px, py, pz), dtype))


def metric_cases(dtype):
    """every metric form under every depth of leading dims, both face positions"""
    out = []
    for n, (metric, lead, to) in enumerate(itertools.product(METRICS, [(), (2,), (2, 2)], TOS)):
        out.append(Case(lead, 3, 4, 6, dtype, PADS3[(5 * n + 1) % 27], to, metric, fill=FILLS[n % 3], nan=n % 5 == 4))
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_metric_forms_and_leading_dims(host_abi, monkeypatch, dtype):
    cases = metric_cases(dtype)
    compare_with_numpy(cases)
    assert _compare_with_chain(monkeypatch, cases) > 0


def test_extend_to_outer_has_no_shear_at_the_top_and_the_bottom(host_abi):
    """`extend` pads a level with itself: both differences are exactly 0 at faces 0 and nz, S2 is +0.0 and Ri 0 / 0 = NaN"""
    c = Case((), 4, 5, 6, np.float64, ("periodic", "periodic", "extend"), "outer")
    ri, s2 = c.one_pass()
    for k in (0, 4):
        assert (s2.values[k] == 0).all() and not np.signbit(s2.values[k]).any() and np.isnan(ri.values[k]).all()
    assert (s2.values[1:4] > 0).all() and np.isfinite(ri.values[1:4]).all()


def test_zero_shear_gives_the_ieee_quotient(host_abi):
    """no guard on S2 == 0: constant u and v under stratification give +-inf by the sign of N2, and 0 / 0 is NaN"""
    c = Case((), 3, 4, 6, np.float64, ("extend", "extend", "fill"), "left", metric=None, fill={"X": 0.0, "Y": 0.0, "Z": 0.25})
    b, u, v = c.f
    u, v = u._replace(data=np.full(u.shape, 0.25)), v._replace(data=np.full(v.shape, 0.25))
    b.values[2, 1, 1] = b.values[1, 1, 1]
    ri = c.grid.richardson_number(b, u, v, **c.kw)
    s2 = c.grid.vertical_shear_squared(u, v, **c.kw)
    assert (s2.values == 0).all()
    db = np.diff(np.concatenate([np.full((1, 4, 6), 0.25), b.values]), axis=0)
    assert np.isnan(ri.values[2, 1, 1]) and db[2, 1, 1] == 0
    rest = db != 0
    assert np.array_equal(ri.values[rest], np.where(db[rest] > 0, np.inf, -np.inf))


def test_to_defaults_to_outer_when_the_axis_has_it_else_left(host_abi, monkeypatch):
    calls = _counted(monkeypatch)
    c = Case((), 3, 4, 6, np.float64, ("periodic", "fill", "extend"), "outer")
    assert c.grid.richardson_number(*c.f).dims == ("ZO", "YC", "XC")
    assert c.grid.vertical_shear_squared(*c.f[1:]).dims == ("ZO", "YC", "XC")
    axes = dict(AXES, Z={"center": "ZC", "left": "ZL"})
    ds = Dataset({"drCl": (("ZL",), np.asarray(c.ds["drCl"].values))}, {k: v for k, v in c.ds.coords.items() if k != "ZO"})
    g2 = Grid(ds, coords=axes, metrics={("Z",): ["drCl"]}, padding=dict(zip("XYZ", c.pads)), autoparse_metadata=False)
    got = g2.richardson_number(*c.f)
    assert got.dims == ("ZL", "YC", "XC") and calls == [True, False, True]
    mets = _metrics_of(c.ds, "1d", "left", ())
    _same_bits(got.values, _want(*(a.values for a in c.f), c.pads, "left", {"X": 0.0, "Y": 0.0, "Z": 0.0}, *mets))


def test_xarray_in_xarray_out(host_abi, monkeypatch):
    import xarray_standin
    from oracle import fake_device

    xarray_standin.install(monkeypatch)
    import xarray as xr

    c = Case((), 3, 4, 6, np.float64, ("periodic", "fill", "extend"), "left")
    xs = [xr.DataArray(a.values, dims=a.dims, name=a.name) for a in c.f]
    got = (c.grid.richardson_number(*xs, **c.kw), c.grid.vertical_shear_squared(*xs[1:], **c.kw))
    assert all(type(g).__module__.split(".")[0] == "xarray" for g in got)
    fake_device.install(monkeypatch)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = c.chain()
    for g, w in zip(got, want):
        assert tuple(g.dims) == tuple(w.dims) and g.name == w.name
        assert np.array_equal(np.asarray(g.values), np.asarray(w.values), equal_nan=True)


def test_coords_and_names_follow_the_chain(host_abi, monkeypatch):
    cases = []
    for names in (("b", "u", "v"), ("q", "q", "q"), ("drCo", "drCo", "drCo"), (None, "v", None), ("hCo", "hWo", "hSo")):
        for metric, to in (("1d", "outer"), ("full", "outer"), ("full", "left"), (None, "left")):
            c = Case((2,), 3, 5, 6, np.float64, ("periodic", "extend", "fill"), to, metric)
            f = [a._replace(name=n) for a, n in zip(c.f, names)]
            f[1] = f[1].assign_coords({"lonW": (("YC", "XG"), np.ones((5, 6))), "t2": (("time",), np.arange(2) + 7.0)})
            f[0] = f[0].assign_coords({"depth": (("ZC",), np.arange(3) * 10.0), "t2": (("time",), np.arange(2) + 9.0),
                                       "lonC": (("YC", "XC"), np.ones((5, 6)))})
            c.f = tuple(f)
            cases.append(c)
    _compare_with_chain(monkeypatch, cases)


def test_the_fused_entry_runs_alone(host_abi, monkeypatch):
    """one call of the one-pass device entry per operator and none of the chain's operators"""
    import xgcm_amd.device as D

    c = Case((2,), 3, 5, 6, np.float64, ("periodic", "fill", "extend"), "outer")
    calls = {"fused": 0, "chain": 0}

    def counted(fn, key):
        def wrapped(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(D, "richardson_number", counted(D.richardson_number, "fused"))
    for name in ("binary", "stencil1d"):
        monkeypatch.setattr(D, name, counted(getattr(D, name), "chain"))
    (ri, s2), (want_ri, want_s2) = c.one_pass(), c.want()
    _same_bits(ri.values, want_ri)
    _same_bits(s2.values, want_s2)
    assert ri.dims == s2.dims == ("time", "ZO", "YC", "XC") and ri.shape == (2, 4, 5, 6)
    assert calls == {"fused": 2, "chain": 0}


# ---- 2. the smallest shapes at which it can go wrong ----------------------------------------------------------------------
NZS, NYS, NXS = [1, 2, 3, 5], [1, 2, 3, 9], [1, 2, 3, 8, 129, 130, 257]


def shape_cases(nx):
    """every nz and ny with this nx -- one level (every face is a pad), one row (the row above is the Y pad), one column (the
    right neighbour is the X pad), nx across the tile's last lane, odd nx (the narrow form) -- the boundary triple, the face
    position, the dtype, the metric form, the fills and the NaNs rotating so that the table as a whole meets every one of
    them several times"""
    out = []
    for n, (nz, ny) in enumerate(itertools.product(NZS, NYS)):
        k = n + 5 * NXS.index(nx)
        out.append(Case((), nz, ny, nx, (np.float64, np.float32)[(k // 2) % 2], PADS3[(7 * k) % 27], TOS[k % 2],
                        METRICS[(k // 2) % 3 + (k % 5 == 0)], fill=FILLS[(k // 3) % 3], nan=(nz + ny) % 3 == 0, seed=71 + k))
    return out


def test_the_shape_table_meets_every_boundary_triple_position_dtype_and_metric_form():
    cases = [c for nx in NXS for c in shape_cases(nx)]
    assert {c.pads for c in cases} == set(PADS3)
    assert {(c.pads[2], c.to, c.f[0].values.dtype.itemsize) for c in cases} == set(itertools.product(BCS, TOS, (4, 8)))
    assert {c.metric for c in cases} == set(METRICS)
    assert {(c.nz, c.pads[2], c.to) for c in cases if c.nz == 1} == {(1, pz, to) for pz in BCS for to in TOS}


@pytest.mark.parametrize("nx", NXS)
def test_small_shapes(host_abi, monkeypatch, nx):
    cases = shape_cases(nx)
    assert len(cases) == len(NZS) * len(NYS)
    compare_with_numpy(cases)
    _compare_with_chain(monkeypatch, cases)


def mid_size_cases(dtype, nx):
    """several bands, ragged tiles and a ragged last segment together; nx = 515 takes the narrow form, 516 the vector form"""
    return [Case((2,), 7, 67, nx, dtype, ("periodic", "extend", "fill"), "outer", "full", nan=True),
            Case((2,), 7, 67, nx, dtype, ("fill", "periodic", "extend"), "left", "1d")]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("nx", [515, 516])
def test_mid_size(host_abi, monkeypatch, dtype, nx):
    calls = _counted(monkeypatch)
    compare_with_numpy(mid_size_cases(dtype, nx))
    assert calls == [True, False] * 2


# ---- 3. NaN locality ------------------------------------------------------------------------------------------------------
NAN_AT = [(0, 0, 0), (4, 2, 3), (2, 5, 3), (2, 2, 7), (4, 5, 7), (2, 2, 3)]   # a corner, beside each pad, all pads, the middle


def nan_cases(to, pads):
    """one NaN at a time in b, in u and in v, at NAN_AT of a (5, 6, 8) volume; (case, field index, position)"""
    out = []
    for which, at in itertools.product(range(3), NAN_AT):
        c = Case((), 5, 6, 8, np.float64, pads, to, "1d")
        c.f[which].values[at] = np.nan
        out.append((c, which, at))
    return out


def check_nan_locality(to, pads):
    for c, which, at in nan_cases(to, pads):
        (ri, s2), (want_ri, want_s2) = c.one_pass(), c.want()
        assert np.array_equal(np.isnan(ri.values), np.isnan(want_ri)), (c, which, at)
        assert np.array_equal(np.isnan(s2.values), np.isnan(want_s2)), (c, which, at)
        assert np.isnan(ri.values).any() and not np.isnan(ri.values).all()
        assert np.isnan(s2.values).any() == (which != 0)   # b never reaches the squared shear
        if at == NAN_AT[-1] and pads[2] == "fill":
            # the middle: faces k and k + 1; u at column i reaches the centres i - 1 and i, v at row j the centres j - 1 and j
            k, j, i = at
            mask = np.zeros(ri.shape, bool)
            mask[k:k + 2, [j, j - 1] if which == 2 else [j], [i, i - 1] if which == 1 else [i]] = True
            assert np.array_equal(np.isnan(ri.values), mask), (c, which)


@pytest.mark.parametrize("to", TOS)
@pytest.mark.parametrize("pads", [("periodic", "periodic", "periodic"), ("extend", "fill", "fill"), ("fill", "extend", "fill")],
                         ids=lambda p: "-".join(p))
def test_a_nan_poisons_exactly_what_the_chain_has_as_nan(host_abi, to, pads):
    check_nan_locality(to, pads)


# ---- 4. seeded fuzz -------------------------------------------------------------------------------------------------------
def fuzz_cases(seed=20241019, n=240):
    """cases over the small shapes, the boundary triples, both face positions, the fills, the dtype, the metric forms and the
    leading dims; a third of them with NaNs"""
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
                        nan=bool(rng.integers(3) == 0), seed=500 + 3 * case))
    return out


def test_seeded_fuzz(host_abi, monkeypatch):
    cases = fuzz_cases()
    solid = _compare_with_chain(monkeypatch, cases)    # (asserts one call per operator and case: none falls back)
    assert len(cases) == 240 and solid >= 10


# ---- 5. every fallback of the docstring takes the chain -------------------------------------------------------------------
def _no_fused(monkeypatch):
    import xgcm_amd.device as D

    monkeypatch.setattr(D, "richardson_number", lambda *a, **k: pytest.fail("one-pass entry called"))


def _fallback_equals_chain(grid, f, **kw):
    _same_labelled(grid.richardson_number(*f, **kw), _chain(grid, *f, **kw))
    _same_labelled(grid.vertical_shear_squared(*f[1:], **kw), _chain(grid, None, *f[1:], **kw))


def _same_error(fused, chain, own=(AttributeError, NotImplementedError)):
    with pytest.raises(Exception) as fused_err:
        fused()
    with pytest.raises(Exception) as chain_err:
        chain()
    assert type(fused_err.value) is type(chain_err.value) and str(fused_err.value) == str(chain_err.value)
    assert not isinstance(fused_err.value, own)


def _case(pads=("periodic", "extend", "fill"), lead=(), nz=3, ny=5, nx=6, dtype=np.float64, to="outer", metric="1d", **kw):
    return Case(lead, nz, ny, nx, dtype, pads, to, metric, **kw)


@pytest.mark.parametrize("dtype", [np.int64, np.int32, np.float16])
def test_integer_and_half_fields_run_the_chain(backend, monkeypatch, dtype):
    _no_fused(monkeypatch)
    c = _case()
    f = tuple(DataArray((a.values * 100).astype(dtype), a.dims, name=a.name) for a in c.f)
    for kw in (dict(), dict(metric_weighted=False, fill_value=FILL, to="left")):
        with np.errstate(all="ignore"):
            _fallback_equals_chain(c.grid, f, **kw)


def test_mixed_dtypes_run_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, dims = _grid((), 3, 5, 6, np.float32, {"X": "fill", "Y": "periodic", "Z": "extend"}, mdtype=np.float64)
    b, u, v = _fields((), 3, 5, 6, np.float32, dims)
    with np.errstate(all="ignore"):
        _fallback_equals_chain(grid, (b, u, v), fill_value=FILL)   # float32 fields over float64 metrics; without: a float64 v
        _fallback_equals_chain(grid, (b, u, v._replace(data=v.values.astype(np.float64))), fill_value=FILL, metric_weighted=False)


def test_fewer_than_three_dims_or_z_elsewhere_run_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    c = _case(lead=(2,))
    b, u, v = c.f
    with np.errstate(all="ignore"):
        _fallback_equals_chain(c.grid, (b.transpose("ZC", "time", "YC", "XC"), u.transpose("ZC", "time", "YC", "XG"),
                                        v.transpose("ZC", "time", "YG", "XC")), fill_value=FILL)
        _fallback_equals_chain(c.grid, (b, u.transpose("time", "YC", "ZC", "XG"), v), fill_value=FILL, metric_weighted=False)
        # columns: (Z, X) fields on a grid whose Y axis they do not have
        col = lambda a: DataArray(np.ascontiguousarray(a.values[0, :, 0, :]), (a.dims[1], a.dims[3]), name=a.name)  # noqa: E731
        got = c.grid.vertical_shear_squared(col(u), col(u)._replace(name="v"), y_axis="X", fill_value=FILL)
        _same_labelled(got, _chain(c.grid, None, col(u), col(u)._replace(name="v"), y_axis="X", fill_value=FILL))


def test_fields_elsewhere_or_of_different_shapes_run_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    c = _case(lead=(2,))
    b, u, v = c.f
    with np.errstate(all="ignore"):
        # u at the centre, v at the centre, b at u's points: the chain takes them wherever they sit
        _fallback_equals_chain(c.grid, (b, DataArray(u.values, b.dims, name="u"), v), fill_value=FILL)
        _fallback_equals_chain(c.grid, (b, u, DataArray(v.values, b.dims, name="v")), fill_value=FILL, metric_weighted=False)
        _same_labelled(c.grid.richardson_number(DataArray(b.values, u.dims, name="b"), u, v, metric_weighted=False),
                       _chain(c.grid, DataArray(b.values, u.dims, name="b"), u, v, metric_weighted=False))
        v0 = DataArray(np.ascontiguousarray(v.values[0]), v.dims[1:], name="v")   # v without the leading dim: it broadcasts
        _fallback_equals_chain(c.grid, (b, u, v0), fill_value=FILL)


@pytest.mark.parametrize("to", ["right", "inner", "center", "nowhere"])
def test_other_targets_do_what_the_chain_does(backend, monkeypatch, to):
    _no_fused(monkeypatch)
    c = _case()
    # (the chain's own refusal of a step it has no ufunc for is a NotImplementedError)
    _same_error(lambda: c.grid.richardson_number(*c.f, to=to), lambda: _chain(c.grid, *c.f, to=to), own=AttributeError)


def test_chunked_inputs_run_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    c = _case(lead=(4,), ny=6, nx=8)
    b, u, v = c.f
    for which in range(3):
        f = list(c.f)
        f[which] = DataArray(BlockArray.from_array(f[which].values, ((2, 2), (3,), (6,), (8,))), f[which].dims, name=f[which].name)
        if which == 0:
            got, want = c.grid.richardson_number(*f, fill_value=FILL), _chain(c.grid, *f, fill_value=FILL)
        else:
            got, want = c.grid.vertical_shear_squared(*f[1:], fill_value=FILL), _chain(c.grid, None, *f[1:], fill_value=FILL)
        assert got.dims == want.dims and got.name == want.name
        assert np.array_equal(np.asarray(got.values), np.asarray(want.values), equal_nan=True)
        mets = _metrics_of(c.ds, "1d", "outer", c.dims)
        plain = _want(b.values if which == 0 else None, u.values, v.values, c.pads, "outer", FILL, *mets[:3 if which == 0 else 2])
        assert np.array_equal(np.asarray(got.values), plain, equal_nan=True)


def test_a_metric_with_an_extra_dim_runs_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    c = _case()
    coords = {k: (k, np.asarray(c.ds.coords[k].values)) for k in ("XC", "XG", "YC", "YG", "ZC", "ZL", "ZO")}
    coords["time"] = ("time", np.arange(2) * 2.0)
    ds2 = Dataset({"drCo": (("ZO", "time"), R.synthetic_metric((4, 2), 66))}, coords)
    g2 = Grid(ds2, coords=AXES, metrics={("Z",): ["drCo"]}, padding=dict(zip("XYZ", c.pads)), autoparse_metadata=False)
    got, want = g2.richardson_number(*c.f, fill_value=FILL), _chain(g2, *c.f, fill_value=FILL)
    assert "time" in got.dims
    _same_labelled(got, want)


def test_a_chunked_metric_runs_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    c = _case(nz=4, metric="full", to="left")
    coords = {k: (k, np.asarray(c.ds.coords[k].values)) for k in ("XC", "XG", "YC", "YG", "ZC", "ZL", "ZO")}
    names = ("hWl", "hSl", "hCl")
    ds2 = Dataset({k: (c.ds[k].dims, BlockArray.from_array(np.asarray(c.ds[k].values), ((2, 2), (5,), (6,)))) for k in names}, coords)
    g2 = Grid(ds2, coords=AXES, metrics={("Z",): list(names)}, padding=dict(zip("XYZ", c.pads)), autoparse_metadata=False)
    kw = dict(to="left", fill_value=FILL)
    for got, want, plain in zip((g2.richardson_number(*c.f, **kw), g2.vertical_shear_squared(*c.f[1:], **kw)),
                                (_chain(g2, *c.f, **kw), _chain(g2, None, *c.f[1:], **kw)), c.want()):
        assert got.dims == want.dims and got.name == want.name
        assert np.array_equal(np.asarray(got.values), np.asarray(want.values), equal_nan=True)
        assert np.array_equal(np.asarray(got.values), plain, equal_nan=True)


def test_a_missing_metric_raises_the_chains_error(backend, monkeypatch):
    _no_fused(monkeypatch)
    c = _case(metric=None)
    _same_error(lambda: c.grid.richardson_number(*c.f), lambda: _chain(c.grid, *c.f))
    _same_error(lambda: c.grid.vertical_shear_squared(*c.f[1:]), lambda: _chain(c.grid, None, *c.f[1:]))


def test_a_missing_metric_is_still_served_unweighted(host_abi, monkeypatch):
    c = _case(metric=None)
    c.kw["metric_weighted"] = False
    assert _compare_with_chain(monkeypatch, [c]) == 1


@pytest.mark.parametrize("axis", ["X", "Y", "Z"])
def test_an_axis_without_a_boundary_raises_the_chains_error(backend, monkeypatch, axis):
    _no_fused(monkeypatch)
    pad = {"X": "periodic", "Y": "extend", "Z": "fill"}
    del pad[axis]
    grid, ds, dims = _grid((), 3, 5, 6, np.float64, pad)
    f = _fields((), 3, 5, 6, np.float64, dims)
    _same_error(lambda: grid.richardson_number(*f), lambda: _chain(grid, *f))
    _same_error(lambda: grid.vertical_shear_squared(*f[1:]), lambda: _chain(grid, None, *f[1:]))


Y_TO_Y = {"face": {0: {"Y": (None, (1, "Y", False))}, 1: {"Y": ((0, "Y", False), None)}}}
Z_TO_Z = {"face": {0: {"Z": (None, (1, "Z", False))}, 1: {"Z": ((0, "Z", False), None)}}}


@pytest.mark.parametrize("conn", ["x2x", "y2y", "z2z"])
def test_connected_faces_run_the_chain(backend, monkeypatch, conn):
    from test_topology import COORDS, X_TO_X

    _no_fused(monkeypatch)
    ds = Dataset({"drC": (("zo",), R.synthetic_metric((5,), 63))},
                 coords={"x": np.arange(4), "xl": np.arange(4) - 0.5, "y": np.arange(4), "yl": np.arange(4) - 0.5,
                         "face": np.arange(2), "zc": np.arange(4) + 0.5, "zo": np.arange(5) * 1.0})
    grid = Grid(ds, coords=dict(COORDS, Z={"center": "zc", "outer": "zo"}), metrics={("Z",): ["drC"]},
                face_connections={"x2x": X_TO_X, "y2y": Y_TO_Y, "z2z": Z_TO_Z}[conn],
                padding={"X": "fill", "Y": "extend", "Z": "fill"}, autoparse_metadata=False)
    assert (COORDS["X"]["left"], COORDS["Y"]["left"], COORDS["X"]["center"], COORDS["Y"]["center"]) == ("xl", "yl", "x", "y")
    f = lambda seed, dims: DataArray(R.synthetic_field((2, 4, 4, 4), seed), dims, name="f")  # noqa: E731
    b, u, v = f(81, ("face", "zc", "y", "x")), f(82, ("face", "zc", "y", "xl")), f(83, ("face", "zc", "yl", "x"))
    for mw in (True, False):
        _fallback_equals_chain(grid, (b, u, v), fill_value=FILL, metric_weighted=mw)


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
        f = lambda seed, dims: DataArray(R.synthetic_field((2, Ny, Nx), seed), dims)  # noqa: E731
        b, u, v = f(91, ("zc", "yh", "xh")), f(92, ("zc", "yh", "xl")), f(93, ("zc", "yl", "xh"))
        for mw in (True, False):
            _fallback_equals_chain(grid, (b, u, v), metric_weighted=mw)


# ---- 6. the entry of the C ABI called directly, with views ----------------------------------------------------------------
NVS = {np.float64: 2, np.float32: 4}
TORCH = {np.float64: torch.float64, np.float32: torch.float32}
CODE = {np.float64: _hip.DTYPE["float64"], np.float32: _hip.DTYPE["float32"]}
ABI_NX = {np.float64: 132, np.float32: 264}   # one full 64-lane tile and a partial one
ABI_PADS = [(("periodic", "extend", "fill"), "left"), (("fill", "periodic", "extend"), "outer"),
            (("extend", "fill", "periodic"), "outer")]
SENTINEL = 12345.5


def _abi_call(D, dtype, shape, fields, planes, k, out_off=ALIGNED):
    """one call of xg_richardson_number: `fields` (b or None, u, v) views, `planes` {mu, mv, mb} views or None; the result is
    written `out_off` elements into an allocation full of SENTINEL, which must still surround it afterwards"""
    (px, py, pz), to = ABI_PADS[k]
    fshape = shape[:-3] + [_nf(shape[-3], to)] + shape[-2:]
    args = [CODE[dtype]] + [None if f is None else f.data_ptr() for f in fields]
    for name in ("mu", "mv", "mb"):
        m = planes.get(name)
        if m is None:
            args += [None, None]
        else:
            assert all(n in (1, s) for n, s in zip(m.shape, fshape))
            args += [m.data_ptr(), _hip.i64([0 if n == 1 else m.stride(d) for d, n in enumerate(m.shape)])]
    n = int(np.prod(fshape))
    buf = torch.full((out_off + n + ALIGNED,), SENTINEL, dtype=TORCH[dtype], device=D._MEM.device)
    out = buf[out_off:out_off + n]
    args += [out.data_ptr(), _hip.i64(shape), len(shape), int(to == "outer"), _hip.BC[px], FILL["X"], _hip.BC[py], FILL["Y"],
             _hip.BC[pz], FILL["Z"]]
    D._check(D._MEM.lib().xg_richardson_number(*args, D._stream()))
    whole = buf.cpu().numpy()
    assert (whole[:out_off] == SENTINEL).all() and (whole[out_off + n:] == SENTINEL).all()
    return whole[out_off:out_off + n].reshape(fshape)


def abi_layout_cases(dtype):
    """Runs the direct-ABI table on whatever library `xgcm_amd.device._MEM` serves.  Every input view lives in a NaN-filled
    allocation, so a read outside it shows in the result; the contiguous, aligned control of each set of planes is compared
    with the numpy chain, every other layout with that control."""
    import xgcm_amd.device as D

    nv = NVS[dtype]
    shape = [2, 5, 7, ABI_NX[dtype]]
    lead, nz, ny, nx = shape
    fv = [R.synthetic_field(tuple(shape), 101 + n).astype(dtype) for n in range(3)]
    fv[2].reshape(-1)[5::17] = np.nan
    put = lambda a, st=None, off=ALIGNED: _strided(D, a, st or _contig(a.shape), off)  # noqa: E731
    for k, ((px, py, pz), to) in enumerate(ABI_PADS):
        nf = _nf(nz, to)
        forms = {"z": (1, nf, 1, 1), "p": (1, 1, ny, nx), "v3": (1, nf, ny, nx), "vl": (lead, nf, ny, nx)}
        vals = {form: R.synthetic_metric(sh, 111 + i).astype(dtype) for i, (form, sh) in enumerate(forms.items())}
        fields = [put(a) for a in fv]
        assert all(f.is_contiguous() and f.data_ptr() % 16 == 0 for f in fields)
        # each metric alone, in each form; all three in mixed forms; none; the squared shear (b NULL) with and without
        for present, ri in (({"mu": "z"}, True), ({"mv": "p"}, True), ({"mb": "v3"}, True), ({"mu": "v3", "mv": "vl", "mb": "z"}, True),
                            ({"mu": "vl", "mv": "z", "mb": "p"}, True), ({"mu": "p", "mv": "v3"}, False), ({}, True), ({}, False)):
            pv = {n: vals[form] for n, form in present.items()}
            aligned = {n: put(a) for n, a in pv.items()}
            fb = [fields[0] if ri else None] + fields[1:]
            control = _abi_call(D, dtype, shape, fb, aligned, k)
            want = _want(fv[0] if ri else None, fv[1], fv[2], (px, py, pz), to, FILL, pv.get("mu"), pv.get("mv"), pv.get("mb"))
            assert control.dtype == want.dtype == np.dtype(dtype)
            _same_bits(control, want)
            views = []
            # a misaligned base: each field in turn, then all three, one element into its allocation (the narrow form); a
            # misaligned result
            for moved in ((0,), (1,), (2,), (0, 1, 2)):
                off = [put(a, off=1) if n in moved else fields[n] for n, a in enumerate(fv)]
                assert all(off[n].data_ptr() % 16 == fv[n].dtype.itemsize for n in moved)
                views.append(([off[0] if ri else None] + off[1:], aligned, ALIGNED))
            views.append((fb, aligned, 1))
            # the planes one element in; with an odd row pitch; with an odd level pitch (volumes)
            views.append((fb, {n: put(a, off=1) for n, a in pv.items()}, ALIGNED))
            pitched = {}
            for n, a in pv.items():
                s = list(a.shape)
                st = _contig(s[:-1] + [s[-1] + 1]) if s[-1] > 1 else _contig(s)
                pitched[n] = put(a, st)
                assert s[-1] == 1 or (pitched[n].stride(-2) == nx + 1 and pitched[n].stride(-1) == 1)
            views.append((fb, pitched, ALIGNED))
            for n, form in present.items():
                a = pv[n]
                if form in ("v3", "vl"):
                    st = [(nf * (ny * nx + 1)) * (a.shape[0] > 1), ny * nx + 1, nx, 1]
                    lev = put(a, [s or 1 for s in st])
                    assert lev.stride(1) == ny * nx + 1
                    views.append((fb, dict(aligned, **{n: lev}), ALIGNED))
                if form == "z":   # the Z-only metric three elements apart
                    views.append((fb, dict(aligned, **{n: put(a, [3 * nf, 3, 1, 1], 1)}), ALIGNED))
                if form == "p":   # the plane stored (X, Y): a transposed view
                    t = put(np.ascontiguousarray(a.transpose(0, 1, 3, 2))).permute(0, 1, 3, 2)
                    assert t.stride(-1) == ny and t.stride(-2) == 1
                    views.append((fb, dict(aligned, **{n: t}), ALIGNED))
            for f_, planes, out_off in views:
                _same_bits(_abi_call(D, dtype, shape, f_, planes, k, out_off), control)
        # a stride-0 metric along X and Y: one value per face, expanded over the whole volume, equals the Z-only metric
        flat = put(vals["z"]).expand(1, nf, ny, nx)
        assert flat.stride(-1) == 0 and flat.stride(-2) == 0
        full = put(np.ascontiguousarray(np.broadcast_to(vals["z"], (1, nf, ny, nx))))
        _same_bits(_abi_call(D, dtype, shape, fields, {"mu": flat, "mv": flat, "mb": flat}, k),
                   _abi_call(D, dtype, shape, fields, {"mu": full, "mv": full, "mb": full}, k))
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
    out = torch.zeros([3, 3, 4], dtype=torch.float64, device=D._MEM.device)   # room for the faces of Z:outer
    P = lambda x: None if x is None else x.data_ptr()  # noqa: E731

    def call(code=CODE[np.float64], b=t, u=t, v=t, o=out, shape=shape, ndim=3, outer=0, bcx=_hip.BC["periodic"],
             bcy=_hip.BC["extend"], bcz=_hip.BC["fill"], mu=None, mus=None):
        return lib.xg_richardson_number(code, P(b), P(u), P(v), mu, mus, None, None, None, None, P(o), _hip.i64(shape), ndim,
                                        outer, bcx, 0.0, bcy, 0.0, bcz, 0.0, D._stream())

    assert call() == 0 and call(bcz=_hip.BC["periodic"], outer=1) == 0 and call(bcz=_hip.BC["extend"], outer=1) == 0
    assert call(b=None) == 0                                      # no b: the squared shear
    for code in (-1, _hip.DTYPE["float16"], _hip.DTYPE["int64"], _hip.DTYPE["int32"], 12, 99):
        assert call(code=code) == -1                              # any other element type: XG_ERR_INVALID
    assert call(u=None) == -1 and call(v=None) == -1 and call(o=None) == -1   # NULL arrays
    assert call(bcx=7) == -1 and call(bcy=-1) == -1 and call(bcz=9) == -1     # unknown boundary codes
    assert call(outer=2) == -1                                    # unknown face position
    assert call(shape=[0, 3, 4]) == -1                            # nz = 0: no level to pad from
    assert call(shape=[2, 0, 4]) == 0 and call(shape=[2, 3, 0]) == 0          # an empty plane: nothing to do
    assert call(mu=t.data_ptr(), mus=None) == -1                  # a metric without strides
    assert call(ndim=2) < 0 and call(ndim=2) != -1                # XG_ERR_UNSUPPORTED


def test_abi_refuses_bad_calls(host_abi):
    abi_bad_calls()
