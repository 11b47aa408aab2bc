"""The vector-invariant harmonic viscosity, `Grid.horizontal_viscosity`, on CPU.

The one-pass path runs through the `host_abi` fixture (the product's `xgcm_amd.device` over libxgcm_host.so) and is compared
bit for bit with the oracle composing the chain the operator replaces:

    div  = R.divergence(u, v, rA or 1.0, ...)   [* nu_d]             (`R.divergence` always divides: area = 1.0 is exact)
    zeta = R.vorticity(u, v, rAz or 1.0, ...)   [* nu_z]
    dx, dy = R.gradient(div, ..., dxC, dyC)
    zy = R.derivative(zeta, Y, 0, 1, ..., dyG),  zx = R.derivative(zeta, X, 0, 1, ..., dxG)     (unweighted: R.stencil1d diff)
    gu = dx - zy,  gv = dy + zx

Every test of the one-pass path counts the calls of the new device entry; the fallbacks only call existing device functions,
run under the `backend` double and assert that the entry was not called."""

import itertools

import numpy as np
import pytest

from oracle import refimpl as R
from xgcm_amd import DataArray, Dataset, Grid
from xgcm_amd.chunked import BlockArray

BCS = ["periodic", "extend", "fill"]
FILL = {"X": 1.75, "Y": -0.625}
AXES = {"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"}}
METRICS = {("X",): ["dxC", "dxG"], ("Y",): ["dyC", "dyG"], ("X", "Y"): ["rA", "rAz"]}


def _grid(lead, ny, nx, dtype, padding, metrics=METRICS):
    """every metric the operator looks up is registered at its own points: each lookup is an exact match"""
    dims = ("time",)[:len(lead)]
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0),
              "YC": ("YC", np.arange(ny) + 0.5), "YG": ("YG", np.arange(ny) * 1.0)}
    for d, n in zip(dims, lead):
        coords[d] = (d, np.arange(n) * 2.0)
    m = lambda seed: R.synthetic_metric((ny, nx), seed).astype(dtype)  # noqa: E731
    data = {"dxC": (("YC", "XG"), m(61)), "dyC": (("YG", "XC"), m(62)), "rAz": (("YG", "XG"), m(63)), "rA": (("YC", "XC"), m(64)),
            "dyG": (("YC", "XG"), m(65)), "dxG": (("YG", "XC"), m(66)),
            "nu_d": (("YC", "XC"), (R.synthetic_field((ny, nx), 67) * 3.0).astype(dtype)),
            "nu_z": (("YG", "XG"), (R.synthetic_field((ny, nx), 68) * 3.0).astype(dtype))}
    ds = Dataset(data, coords)
    grid = Grid(ds, coords=AXES, metrics=metrics, padding=padding, autoparse_metadata=False)
    return grid, ds, dims


def _fields(lead, ny, nx, dtype, dims, nan=False):
    shape = tuple(lead) + (ny, nx)
    f = lambda seed: R.synthetic_field(shape, seed).astype(dtype)  # noqa: E731
    u, v = f(72), f(73)
    if nan:
        u.reshape(-1)[3::11] = np.nan
        v.reshape(-1)[5::13] = np.nan
    return DataArray(u, dims + ("YC", "XG"), name="u"), DataArray(v, dims + ("YG", "XC"), name="v")


def _coefficients(form, lead, ny, nx, dtype, dims, ds):
    """(nu_d, nu_z) as the operator takes them and as arrays that broadcast against (lead, Y, X) for the oracle"""
    if form == "none":
        return (None, None), (None, None)
    if form == "planes":
        return (ds["nu_d"], ds["nu_z"]), (np.asarray(ds["nu_d"].values), np.asarray(ds["nu_z"].values))
    if form == "rows":  # f(YC) / f(YG)
        a, b = ((R.synthetic_field((ny,), seed) * 2.0).astype(dtype) for seed in (69, 70))
        return (DataArray(a, ("YC",), name="nu_d"), DataArray(b, ("YG",), name="nu_z")), (a[:, None], b[:, None])
    assert form == "full"  # (lead, Y, X)
    shape = tuple(lead) + (ny, nx)
    a, b = ((R.synthetic_field(shape, seed) * 2.0).astype(dtype) for seed in (74, 75))
    return (DataArray(a, dims + ("YC", "XC"), name="nu_d"), DataArray(b, dims + ("YG", "XG"), name="nu_z")), (a, b)


def _want(u, v, px, py, ds=None, nu=(None, None), fill=FILL):
    """the chain; `ds`: the dataset whose six metrics weight it (None: unweighted).  Every operator of the chain, two-axis or
    one-axis, takes its fill as it is: a -0.0 fill keeps its sign."""
    pos = {k: float(f) for k, f in fill.items()}
    one = np.asarray(1.0, dtype=u.dtype)
    met = (lambda k: np.asarray(ds[k].values)) if ds is not None else (lambda k: None)
    div = R.divergence(u, v, one if ds is None else met("rA"), px, py, pos["X"], pos["Y"])
    zeta = R.vorticity(u, v, one if ds is None else met("rAz"), px, py, pos["X"], pos["Y"])
    if nu[0] is not None:
        div = R.binary("mul", div, nu[0])
    if nu[1] is not None:
        zeta = R.binary("mul", zeta, nu[1])
    dx, dy = R.gradient(div, px, py, pos["X"], pos["Y"], met("dxC"), met("dyC"))
    fx, fy = np.asarray(fill["X"], dtype=u.dtype), np.asarray(fill["Y"], dtype=u.dtype)
    if ds is not None:
        zy = R.derivative(zeta, zeta.ndim - 2, 0, 1, py, fy, met("dyG"))
        zx = R.derivative(zeta, zeta.ndim - 1, 0, 1, px, fx, met("dxG"))
    else:
        zy = R.stencil1d("diff", zeta, zeta.ndim - 2, 0, 1, py, fy)
        zx = R.stencil1d("diff", zeta, zeta.ndim - 1, 0, 1, px, fx)
    return R.binary("sub", dx, zy), R.binary("add", dy, zx)


def _same(got, want):
    got = np.asarray(got.values if hasattr(got, "values") else got)
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got, want, equal_nan=True)


def _same_bits(got, want):
    got = np.asarray(got.values if hasattr(got, "values") else got)
    want = np.asarray(want.values if hasattr(want, "values") else want)
    assert got.dtype == want.dtype and got.shape == want.shape
    as_int = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    assert np.array_equal(np.ascontiguousarray(got).view(as_int), np.ascontiguousarray(want).view(as_int))


class _Calls:
    """counts the calls of the new device entry"""

    def __init__(self, monkeypatch):
        import xgcm_amd.device as D

        self.n = 0
        fn = D.horizontal_viscosity

        def wrapped(*a, **k):
            self.n += 1
            return fn(*a, **k)

        monkeypatch.setattr(D, "horizontal_viscosity", wrapped)


# (lead, ny, nx): odd nx, nx below one 16-byte vector, ny not a multiple of the 2-row segment, ny / nx of 1, a lead dim
SHAPES = [((), 6, 8), ((), 7, 5), ((), 1, 6), ((), 6, 1), ((2,), 5, 4), ((2,), 3, 7), ((), 4, 3), ((), 1, 1), ((3,), 2, 2)]
PADS = list(itertools.product(BCS, BCS))


@pytest.mark.parametrize("px,py", PADS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("coefficients", ["none", "planes", "rows", "full"])
def test_horizontal_viscosity_equals_the_oracle_chain(host_abi, monkeypatch, px, py, dtype, weighted, coefficients):
    calls = _Calls(monkeypatch)
    for lead, ny, nx in SHAPES:
        grid, ds, dims = _grid(lead, ny, nx, dtype, {"X": px, "Y": py})
        u, v = _fields(lead, ny, nx, dtype, dims)
        nu, nu_np = _coefficients(coefficients, lead, ny, nx, dtype, dims, ds)
        gu, gv = grid.horizontal_viscosity(u, v, *nu, fill_value=FILL, metric_weighted=weighted)
        wu, wv = _want(u.values, v.values, px, py, ds if weighted else None, nu_np)
        assert gu.dims == dims + ("YC", "XG") and gv.dims == dims + ("YG", "XC")
        _same(gu, wu)
        _same(gv, wv)
    assert calls.n == len(SHAPES)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("coefficients", ["none", "planes"])
def test_nans_propagate_as_in_the_chain(host_abi, monkeypatch, dtype, coefficients):
    calls = _Calls(monkeypatch)
    for px, py in PADS:
        grid, ds, dims = _grid((2,), 7, 9, dtype, {"X": px, "Y": py})
        u, v = _fields((2,), 7, 9, dtype, dims, nan=True)
        nu, nu_np = _coefficients(coefficients, (2,), 7, 9, dtype, dims, ds)
        gu, gv = grid.horizontal_viscosity(u, v, *nu, fill_value=FILL)
        wu, wv = _want(u.values, v.values, px, py, ds, nu_np)
        assert np.isnan(wu).any() and not np.isnan(wu).all()
        _same(gu, wu)
        _same(gv, wv)
    assert calls.n == len(PADS)


# ---- the chain itself, through Grid ---------------------------------------------------------------------------------
def _chain(grid, u, v, viscosity_d=None, viscosity_z=None, x_axis="X", y_axis="Y", padding=None, fill_value=None,
           metric_weighted=True):
    kw = dict(padding=padding, fill_value=fill_value)
    div = grid.divergence(u, v, x_axis, y_axis, metric_weighted=metric_weighted, **kw)
    zeta = grid.vorticity(u, v, x_axis, y_axis, metric_weighted=metric_weighted, **kw)
    if viscosity_d is not None:
        div = div * viscosity_d
    if viscosity_z is not None:
        zeta = zeta * viscosity_z
    dx, dy = grid.gradient(div, x_axis, y_axis, metric_weighted=metric_weighted, **kw)
    op = grid.derivative if metric_weighted else grid.diff
    zy = op(zeta, y_axis, **kw)
    zx = op(zeta, x_axis, **kw)
    gu = dx - zy
    gv = dy + zx
    return gu, gv


# ---- signed zeros ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("which", ["X", "Y", "XY"])
def test_a_negative_zero_fill_leaves_the_chains_bit_patterns(host_abi, monkeypatch, dtype, weighted, which):
    """all-zero fields (+0.0 and -0.0 mixed), fill_value = -0.0: every operator of the chain pads with -0.0, and
    (-0.0) - (+0.0) differs from (+0.0) - (+0.0) in its sign bit.  Compared as integers with the oracle AND with the chain
    itself run through Grid over the oracle double."""
    from oracle import fake_device

    calls = _Calls(monkeypatch)
    fill = {ax: (-0.0 if ax in which else 0.0) for ax in ("X", "Y")}
    cases = []
    for (lead, ny, nx), (px, py) in itertools.product([((), 4, 5), ((2,), 3, 4), ((), 1, 1)], PADS):
        if "fill" not in (px, py):
            continue
        grid, ds, dims = _grid(lead, ny, nx, dtype, {"X": px, "Y": py})
        shape = tuple(lead) + (ny, nx)
        u = np.zeros(shape, dtype=dtype)
        v = np.zeros(shape, dtype=dtype)
        u.reshape(-1)[::2] = -0.0
        v.reshape(-1)[1::3] = -0.0
        u, v = DataArray(u, dims + ("YC", "XG"), name="u"), DataArray(v, dims + ("YG", "XC"), name="v")
        gu, gv = grid.horizontal_viscosity(u, v, fill_value=fill, metric_weighted=weighted)
        wu, wv = _want(u.values, v.values, px, py, ds if weighted else None, fill=fill)
        _same_bits(gu, wu)
        _same_bits(gv, wv)
        cases.append((grid, u, v, gu, gv))
    assert calls.n == len(cases) and len(cases) == 15
    signs = np.concatenate([np.signbit(np.asarray(g.values)).reshape(-1) for c in cases for g in c[3:]])
    assert signs.any() and not signs.all()  # (both signs of zero occur: the comparison sees the trap)
    fake_device.install(monkeypatch)
    for grid, u, v, gu, gv in cases:
        cu, cv = _chain(grid, u, v, fill_value=fill, metric_weighted=weighted)
        _same_bits(gu, cu)
        _same_bits(gv, cv)
    assert calls.n == len(cases)


# ---- dims, coords, names --------------------------------------------------------------------------------------------
def _same_labelled(got, want):
    assert tuple(got.dims) == tuple(want.dims) and got.shape == want.shape and got.name == want.name
    assert list(got.coords) == list(want.coords)
    assert dict(got.attrs) == dict(want.attrs)
    for k in want.coords:
        assert got.coords[k].dims == want.coords[k].dims
        assert np.array_equal(np.asarray(got.coords[k].values), np.asarray(want.coords[k].values))
    g, w = np.asarray(got.values), np.asarray(want.values)
    assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=True)


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("coefficients", ["none", "planes", "rows", "full"])
@pytest.mark.parametrize("names", ["own", "same", "metric"])
def test_dims_coords_and_names_are_the_chains(host_abi, monkeypatch, weighted, coefficients, names):
    """fused through the host ABI first, then the chain itself through Grid over the oracle double (installed after the
    fused call has run): same values, dims, coords, names and attrs.  `names`: every operand its own name, all the same
    one, or all the name of a metric (`derivative` keeps a name only where its metric carries it)."""
    from oracle import fake_device

    calls = _Calls(monkeypatch)
    grid, ds, dims = _grid((2,), 5, 6, np.float64, {"X": "periodic", "Y": "extend"})
    u, v = _fields((2,), 5, 6, np.float64, dims)
    nu, _ = _coefficients(coefficients, (2,), 5, 6, np.float64, dims, ds)
    if names != "own":
        name = "q" if names == "same" else "dyG"
        u, v = (a._replace(name=name) for a in (u, v))
        nu = tuple(None if a is None else a._replace(name=name) for a in nu)
    u = u.assign_coords({"lon_u": (("YC", "XG"), np.ones((5, 6))), "tu": (("time",), np.arange(2) + 7.0)})
    v = v.assign_coords({"tv": (("time",), np.arange(2) - 1.0), "lat_v": (("YG", "XC"), np.ones((5, 6)))})
    if nu[0] is not None:
        nu = (nu[0].assign_coords({"lat_d": (("YC",), np.arange(5) * 3.0)}),
              nu[1].assign_coords({"lat_z": (("YG",), np.arange(5) * 5.0)}))
    kw = dict(fill_value=FILL, metric_weighted=weighted)
    gu, gv = grid.horizontal_viscosity(u, v, *nu, **kw)
    assert calls.n == 1
    fake_device.install(monkeypatch)
    wu, wv = _chain(grid, u, v, *nu, **kw)
    _same_labelled(gu, wu)
    _same_labelled(gv, wv)
    assert calls.n == 1


def test_xarray_in_xarray_out(host_abi, monkeypatch):
    import xarray_standin
    from oracle import fake_device

    xarray_standin.install(monkeypatch)
    import xarray as xr

    calls = _Calls(monkeypatch)
    grid, ds, dims = _grid((), 4, 6, np.float64, {"X": "periodic", "Y": "fill"})
    u, v = _fields((), 4, 6, np.float64, dims)
    xs = [xr.DataArray(a.values, dims=a.dims, name=a.name) for a in (u, v)]
    xn = [xr.DataArray(np.asarray(ds[k].values), dims=ds[k].dims, name=k) for k in ("nu_d", "nu_z")]
    gu, gv = grid.horizontal_viscosity(*xs, *xn, fill_value=FILL)
    assert calls.n == 1
    assert all(type(r).__module__.split(".")[0] == "xarray" for r in (gu, gv))
    fake_device.install(monkeypatch)
    wu, wv = _chain(grid, u, v, ds["nu_d"], ds["nu_z"], fill_value=FILL)
    for got, want in ((gu, wu), (gv, wv)):
        assert tuple(got.dims) == tuple(want.dims) and got.name == want.name
        assert np.array_equal(np.asarray(got.values), np.asarray(want.values))


def test_the_fused_entry_runs_alone(host_abi, monkeypatch):
    """one call of the fused device entry and none of the chain's operators"""
    import xgcm_amd.device as D

    calls = _Calls(monkeypatch)
    chain = {"n": 0}

    def counted(fn):
        def wrapped(*a, **k):
            chain["n"] += 1
            return fn(*a, **k)
        return wrapped

    for name in ("vorticity", "divergence", "gradient", "binary", "stencil1d"):
        monkeypatch.setattr(D, name, counted(getattr(D, name)))
    grid, ds, dims = _grid((2,), 5, 6, np.float64, {"X": "periodic", "Y": "fill"})
    u, v = _fields((2,), 5, 6, np.float64, dims)
    grid.horizontal_viscosity(u, v, ds["nu_d"], ds["nu_z"], fill_value=FILL)
    grid.horizontal_viscosity(u, v, fill_value=FILL, metric_weighted=False)
    assert calls.n == 2 and chain["n"] == 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_applied_twice_it_is_the_biharmonic_operator(host_abi, monkeypatch, dtype):
    calls = _Calls(monkeypatch)
    grid, ds, dims = _grid((2,), 5, 6, dtype, {"X": "periodic", "Y": "extend"})
    u, v = _fields((2,), 5, 6, dtype, dims)
    bu, bv = grid.horizontal_viscosity(*grid.horizontal_viscosity(u, v))
    wu, wv = _want(*_want(u.values, v.values, "periodic", "extend", ds, fill={"X": 0.0, "Y": 0.0}), "periodic", "extend", ds,
                   fill={"X": 0.0, "Y": 0.0})
    _same(bu, wu)
    _same(bv, wv)
    assert calls.n == 2


def test_a_uniform_flow_has_no_viscous_tendency(host_abi, monkeypatch):
    """u = U, v = V on a doubly periodic grid: every difference vanishes exactly, so D, zeta and both tendencies are zeros"""
    calls = _Calls(monkeypatch)
    grid, ds, dims = _grid((), 6, 8, np.float64, {"X": "periodic", "Y": "periodic"})
    u = DataArray(np.full((6, 8), 0.375), ("YC", "XG"))
    v = DataArray(np.full((6, 8), -1.25), ("YG", "XC"))
    gu, gv = grid.horizontal_viscosity(u, v, ds["nu_d"], ds["nu_z"])
    assert not gu.values.any() and not gv.values.any()
    assert calls.n == 1


def test_interpolated_metrics_give_what_the_chain_gives(host_abi, monkeypatch):
    """only dxC and dyC registered: `get_metric` interpolates the other four (and warns); whichever path the call takes,
    the result is the chain's"""
    from oracle import fake_device

    calls = _Calls(monkeypatch)
    grid, ds, dims = _grid((2,), 5, 6, np.float64, {"X": "periodic", "Y": "extend"}, metrics={("X",): ["dxC"], ("Y",): ["dyC"]})
    u, v = _fields((2,), 5, 6, np.float64, dims)
    with pytest.warns(UserWarning, match="interpolated"):
        gu, gv = grid.horizontal_viscosity(u, v, ds["nu_d"], ds["nu_z"], fill_value=FILL)
    n = calls.n
    fake_device.install(monkeypatch)
    with pytest.warns(UserWarning, match="interpolated"):
        wu, wv = _chain(grid, u, v, ds["nu_d"], ds["nu_z"], fill_value=FILL)
    _same_labelled(gu, wu)
    _same_labelled(gv, wv)
    assert calls.n == n


# ---- fallbacks: the chain itself (existing device functions only) ---------------------------------------------------
def _falls_back(grid, u, v, nu=(None, None), labelled=True, **kw):
    same = _same_labelled if labelled else (lambda g, w: _same(g, np.asarray(w.values)))
    gu, gv = grid.horizontal_viscosity(u, v, *nu, **kw)
    wu, wv = _chain(grid, u, v, *nu, **kw)
    same(gu, wu)
    same(gv, wv)


@pytest.mark.parametrize("dtype", [np.int64, np.int32, np.float16])
def test_integer_and_half_fields_run_the_chain(backend, monkeypatch, dtype):
    calls = _Calls(monkeypatch)
    grid, ds, dims = _grid((), 5, 6, np.float64, {"X": "periodic", "Y": "extend"})
    vals = lambda seed: (R.synthetic_field((5, 6), seed) * 100).astype(dtype)  # noqa: E731
    u, v = DataArray(vals(1), ("YC", "XG")), DataArray(vals(2), ("YG", "XC"))
    for kw in (dict(), dict(metric_weighted=False)):
        _falls_back(grid, u, v, (ds["nu_d"], ds["nu_z"]), **kw)
        _falls_back(grid, u, v, **kw)
    assert calls.n == 0


def test_mixed_dtypes_run_the_chain(backend, monkeypatch):
    calls = _Calls(monkeypatch)
    grid, ds, dims = _grid((), 5, 6, np.float64, {"X": "fill", "Y": "periodic"})
    u, v = _fields((), 5, 6, np.float64, dims)
    v32 = DataArray(v.values.astype(np.float32), v.dims)
    _falls_back(grid, u, v32, fill_value=FILL)
    # float32 fields over float64 metrics
    u32, v32 = _fields((), 5, 6, np.float32, dims)
    _falls_back(grid, u32, v32, fill_value=FILL)
    # float32 fields over float64 coefficients, float64 fields over float32 coefficients
    _falls_back(grid, u32, v32, (ds["nu_d"], ds["nu_z"]), fill_value=FILL, metric_weighted=False)
    nu32 = tuple(DataArray(np.asarray(ds[k].values).astype(np.float32), ds[k].dims, name=k) for k in ("nu_d", "nu_z"))
    _falls_back(grid, u, v, nu32, fill_value=FILL)
    _falls_back(grid, u, v, (ds["nu_d"], nu32[1]), fill_value=FILL, metric_weighted=False)
    assert calls.n == 0


def test_x_before_y_and_different_shapes_do_what_the_chain_does(backend, monkeypatch):
    """(X, Y) order: the chain's first operator (the fused divergence) wants (Y, X) last and says so; v with a leading
    extent of 1 under u's 2: whatever the chain does with it"""
    calls = _Calls(monkeypatch)
    grid, ds, dims = _grid((2,), 5, 6, np.float64, {"X": "periodic", "Y": "extend"})
    u, v = _fields((2,), 5, 6, np.float64, dims)
    ut, vt = (a.transpose(a.dims[0], a.dims[2], a.dims[1]) for a in (u, v))
    with pytest.raises(Exception) as fused_err:
        grid.horizontal_viscosity(ut, vt, fill_value=FILL)
    with pytest.raises(Exception) as chain_err:
        _chain(grid, ut, vt, fill_value=FILL)
    assert type(fused_err.value) is type(chain_err.value) and str(fused_err.value) == str(chain_err.value)
    short = DataArray(np.ascontiguousarray(v.values[:1]), v.dims, name="v")
    _does_what_the_chain_does(grid, u, short, fill_value=FILL)
    assert calls.n == 0


def _does_what_the_chain_does(grid, u, v, nu=(None, None), **kw):
    try:
        want = _chain(grid, u, v, *nu, **kw)
    except Exception as chain_err:  # (the chain's fused operators take whole arrays)
        with pytest.raises(type(chain_err)) as fused_err:
            grid.horizontal_viscosity(u, v, *nu, **kw)
        assert str(fused_err.value) == str(chain_err)
    else:
        got = grid.horizontal_viscosity(u, v, *nu, **kw)
        for g, w in zip(got, want):
            assert g.dims == w.dims and g.name == w.name
            assert np.array_equal(np.asarray(g.values), np.asarray(w.values), equal_nan=True)


def test_chunked_inputs_coefficients_and_metrics_do_what_the_chain_does(backend, monkeypatch):
    calls = _Calls(monkeypatch)
    grid, ds, dims = _grid((4,), 6, 8, np.float64, {"X": "periodic", "Y": "extend"})
    u, v = _fields((4,), 6, 8, np.float64, dims)
    chunks = ((2, 2), (6,), (8,))
    cu = DataArray(BlockArray.from_array(u.values, chunks), u.dims, name="u")
    cv = DataArray(BlockArray.from_array(v.values, chunks), v.dims, name="v")
    _does_what_the_chain_does(grid, cu, cv, fill_value=FILL, metric_weighted=False)
    _does_what_the_chain_does(grid, cu, cv, fill_value=FILL)
    # whole fields, chunked coefficients
    (nud, nuz), _ = _coefficients("full", (4,), 6, 8, np.float64, dims, ds)
    cd = DataArray(BlockArray.from_array(nud.values, chunks), nud.dims, name="nu_d")
    cz = DataArray(BlockArray.from_array(nuz.values, chunks), nuz.dims, name="nu_z")
    _does_what_the_chain_does(grid, u, v, (cd, cz), fill_value=FILL, metric_weighted=False)
    _does_what_the_chain_does(grid, u, v, (nud, cz), fill_value=FILL, metric_weighted=False)
    assert calls.n == 0


def test_a_chunked_metric_does_what_the_chain_does(backend, monkeypatch):
    calls = _Calls(monkeypatch)
    grid, ds, dims = _grid((2,), 6, 8, np.float64, {"X": "periodic", "Y": "extend"})
    u, v = _fields((2,), 6, 8, np.float64, dims)
    data = {k: (ds[k].dims, np.asarray(ds[k].values)) for k in ("dxC", "dyC", "dyG", "dxG", "rA", "rAz")}
    data["dyG"] = (data["dyG"][0], BlockArray.from_array(data["dyG"][1], ((3, 3), (8,))))
    ds2 = Dataset(data, {k: (k, np.asarray(ds[k].values)) for k in ("XC", "XG", "YC", "YG")})
    chunked = Grid(ds2, coords=AXES, metrics=METRICS, padding={"X": "periodic", "Y": "extend"}, autoparse_metadata=False)
    _does_what_the_chain_does(chunked, u, v, fill_value=FILL)
    assert calls.n == 0


def test_a_coefficient_with_dims_the_stage_lacks_runs_the_chain(backend, monkeypatch):
    calls = _Calls(monkeypatch)
    grid, ds, dims = _grid((), 5, 6, np.float64, {"X": "periodic", "Y": "extend"})
    u, v = _fields((), 5, 6, np.float64, dims)
    extra = DataArray(np.arange(3.0) + 1.0, ("member",), name="nu")
    _falls_back(grid, u, v, (extra, extra), fill_value=FILL)
    # a coefficient at the wrong point carries a dim its stage lacks as well
    _does_what_the_chain_does(grid, u, v, (ds["nu_z"], ds["nu_d"]), fill_value=FILL)
    assert calls.n == 0


def test_exactly_one_coefficient_runs_the_chain(backend, monkeypatch):
    calls = _Calls(monkeypatch)
    grid, ds, dims = _grid((2,), 5, 6, np.float64, {"X": "fill", "Y": "extend"})
    u, v = _fields((2,), 5, 6, np.float64, dims)
    _falls_back(grid, u, v, (ds["nu_d"], None), fill_value=FILL)
    _falls_back(grid, u, v, (None, ds["nu_z"]), fill_value=FILL, metric_weighted=False)
    assert calls.n == 0


def test_connected_faces_run_the_chain(backend, monkeypatch):
    from test_topology import COORDS, X_TO_X

    calls = _Calls(monkeypatch)
    ds = Dataset(coords={"x": np.arange(4), "xl": np.arange(4) - 0.5, "y": np.arange(4), "yl": np.arange(4) - 0.5,
                         "face": np.arange(2)})
    grid = Grid(ds, coords=COORDS, face_connections=X_TO_X, padding={"X": "fill", "Y": "extend"}, autoparse_metadata=False)
    f = lambda seed, dims: DataArray(R.synthetic_field((2, 4, 4), seed), dims)  # noqa: E731
    u, v = f(82, ("face", "y", "xl")), f(83, ("face", "yl", "x"))
    _falls_back(grid, u, v, (f(84, ("face", "y", "x")), f(85, ("face", "yl", "xl"))), metric_weighted=False)
    assert calls.n == 0


def test_a_missing_metric_raises_the_chains_error(backend, monkeypatch):
    calls = _Calls(monkeypatch)
    grid, ds, dims = _grid((), 5, 6, np.float64, {"X": "periodic", "Y": "extend"}, metrics={("X",): ["dxC", "dxG"]})
    u, v = _fields((), 5, 6, np.float64, dims)
    with pytest.raises(Exception) as fused_err:
        grid.horizontal_viscosity(u, v)
    with pytest.raises(Exception) as chain_err:
        _chain(grid, u, v)
    assert type(fused_err.value) is type(chain_err.value) and str(fused_err.value) == str(chain_err.value)
    assert calls.n == 0


def test_misplaced_inputs_raise(backend):
    grid, ds, dims = _grid((), 5, 6, np.float64, {"X": "periodic", "Y": "extend"})
    u, v = _fields((), 5, 6, np.float64, dims)
    with pytest.raises(NotImplementedError, match="X:left"):
        grid.horizontal_viscosity(v, u)
    with pytest.raises(NotImplementedError):
        grid.horizontal_viscosity(u, u)


def test_missing_boundary_raises_the_chains_error(backend, monkeypatch):
    calls = _Calls(monkeypatch)
    grid, ds, dims = _grid((), 5, 6, np.float64, {"X": "periodic", "Y": "extend"})
    u, v = _fields((), 5, 6, np.float64, dims)
    for padding in ({"X": "periodic"}, {"Y": "extend"}):
        bare = Grid(ds, coords=AXES, padding=padding, autoparse_metadata=False)
        with pytest.raises(Exception) as fused_err:
            bare.horizontal_viscosity(u, v, metric_weighted=False)
        with pytest.raises(Exception) as chain_err:
            _chain(bare, u, v, metric_weighted=False)
        assert type(fused_err.value) is type(chain_err.value) and str(fused_err.value) == str(chain_err.value)
    assert calls.n == 0
