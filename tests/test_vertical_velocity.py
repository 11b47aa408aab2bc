"""Vertical velocity from continuity, `Grid.vertical_velocity`, on CPU.

The one-pass path runs through the `host_abi` fixture (the product's `xgcm_amd.device` over libxgcm_host.so) and is
compared bit for bit with the oracle composing the chain the operator replaces:

    [u = R.binary("mul", u, face area of u);  v likewise]
    d = R.divergence(u, v, 1.0, bcx, bcy, fx, fy)                  (`R.divergence` always divides: area = 1.0 is exact)
    w = -R.grid_cumsum(d, Z, "center", "left", bcz, fz, reverse=rev)
    [w = R.binary("div", w, area)]

The fallbacks only call existing device functions and run under the `backend` double."""

import itertools

import numpy as np
import pytest

from oracle import refimpl as R
from xgcm_amd import DataArray, Dataset, Grid
from xgcm_amd.chunked import BlockArray

BCS = ["periodic", "extend", "fill"]
ZBCS = ["fill", "extend"]
FILL = {"X": 1.75, "Y": -0.625, "Z": 0.375}
AXES = {"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"}, "Z": {"center": "ZC", "left": "ZL"}}


def _grid(lead, nz, ny, nx, dtype, padding, faces="factors", area="plane"):
    """C-grid with a Z axis.  Face areas: dyG(YC, XG) * drF(ZC) and dxG(YG, XC) * drF(ZC) formed by the grid (`factors`) or
    registered (Z, Y, X) arrays (`registered`); the area of the result: rA(YC, XC) (`plane`) or a (ZL, YC, XC) array (`full`)"""
    dims = ("time",)[:len(lead)]
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0),
              "YC": ("YC", np.arange(ny) + 0.5), "YG": ("YG", np.arange(ny) * 1.0),
              "ZC": ("ZC", -np.arange(nz) - 0.5), "ZL": ("ZL", -np.arange(nz) * 1.0)}
    for d, n in zip(dims, lead):
        coords[d] = (d, np.arange(n) * 2.0)
    m = lambda shape, seed: R.synthetic_metric(shape, seed).astype(dtype)  # noqa: E731
    data = {"dyG": (("YC", "XG"), m((ny, nx), 61)), "dxG": (("YG", "XC"), m((ny, nx), 62)), "drF": (("ZC",), m((nz,), 63))}
    metrics = {("X",): ["dxG"], ("Y",): ["dyG"], ("Z",): ["drF"]}
    if area == "plane":
        data["rA"] = (("YC", "XC"), m((ny, nx), 64))
        metrics[("X", "Y")] = ["rA"]
    else:
        data["rA3"] = (("ZL", "YC", "XC"), m((nz, ny, nx), 65))
        metrics[("X", "Y")] = ["rA3"]
    if faces == "registered":
        data["yzA"] = (("ZC", "YC", "XG"), m((nz, ny, nx), 66))
        data["xzA"] = (("ZC", "YG", "XC"), m((nz, ny, nx), 67))
        metrics[("Y", "Z")] = ["yzA"]
        metrics[("X", "Z")] = ["xzA"]
    ds = Dataset(data, coords)
    grid = Grid(ds, coords=AXES, metrics=metrics, padding=padding, autoparse_metadata=False)
    return grid, ds, dims


def _fields(lead, nz, ny, nx, dtype, dims, nan=False):
    shape = tuple(lead) + (nz, ny, nx)
    f = lambda seed: R.synthetic_field(shape, seed).astype(dtype)  # noqa: E731
    u, v = f(72), f(73)
    if nan:
        u.reshape(-1)[3::11] = np.nan
        v.reshape(-1)[5::13] = np.nan
    return DataArray(u, dims + ("ZC", "YC", "XG"), name="u"), DataArray(v, dims + ("ZC", "YG", "XC"), name="v")


def _face_areas(ds, faces):
    if faces == "registered":
        return np.asarray(ds["yzA"].values), np.asarray(ds["xzA"].values)
    drf = np.asarray(ds["drF"].values)[:, None, None]
    return (R.binary("mul", np.asarray(ds["dyG"].values)[None], drf), R.binary("mul", np.asarray(ds["dxG"].values)[None], drf))


def _area(ds, area):
    return np.asarray(ds["rA"].values) if area == "plane" else np.asarray(ds["rA3"].values)


def _want(u, v, px, py, pz, rev, faces=None, area=None, fill=FILL):
    zax = u.ndim - 3
    if faces is not None:
        u, v = R.binary("mul", u, faces[0]), R.binary("mul", v, faces[1])
    d = R.divergence(u, v, 1.0, px, py, fill["X"], fill["Y"])
    w = -R.grid_cumsum(d, zax, "center", "left", pz, fill["Z"], reverse=rev)
    return w if area is None else R.binary("div", w, area)


def _same(got, want):
    got = np.asarray(got.values if hasattr(got, "values") else got)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got, want, equal_nan=True)


# (lead, nz, ny, nx): odd nx, nx below one 16-byte vector, ny not a multiple of the 2-row segment, nz / ny / nx of 1, a lead dim
SHAPES = [((), 4, 6, 8), ((), 3, 7, 5), ((), 5, 1, 6), ((), 4, 6, 1), ((2,), 3, 5, 4), ((2,), 2, 3, 7), ((), 7, 4, 3)]
PADS = list(itertools.product(BCS, BCS, ZBCS, [False, True]))


@pytest.mark.parametrize("px,py,pz,rev", PADS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("weighted", [True, False])
def test_equals_the_oracle_chain(host_abi, px, py, pz, rev, dtype, weighted):
    for lead, nz, ny, nx in SHAPES:
        grid, ds, dims = _grid(lead, nz, ny, nx, dtype, {"X": px, "Y": py, "Z": pz})
        u, v = _fields(lead, nz, ny, nx, dtype, dims)
        got = grid.vertical_velocity(u, v, fill_value=FILL, reverse=rev, metric_weighted=weighted)
        _same(got, _want(u.values, v.values, px, py, pz, rev, area=_area(ds, "plane") if weighted else None))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_single_level(host_abi, dtype):
    """nz = 1: upward with `fill` the result is the pad alone, downward it is the level's own divergence"""
    for lead, ny, nx in [((), 5, 9), ((), 1, 1), ((2,), 3, 4)]:
        for px, py, rev in [("periodic", "fill", False), ("extend", "periodic", True), ("fill", "extend", True)]:
            grid, ds, dims = _grid(lead, 1, ny, nx, dtype, {"X": px, "Y": py, "Z": "fill"})
            u, v = _fields(lead, 1, ny, nx, dtype, dims)
            got = grid.vertical_velocity(u, v, fill_value=FILL, reverse=rev)
            _same(got, _want(u.values, v.values, px, py, "fill", rev, area=_area(ds, "plane")))


@pytest.mark.parametrize("faces", ["factors", "registered"])
@pytest.mark.parametrize("area", ["plane", "full", None])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_face_weights_and_area_in_both_forms(host_abi, faces, area, dtype):
    for lead, nz, ny, nx in [((), 4, 6, 8), ((2,), 3, 5, 7), ((), 1, 1, 1), ((), 5, 3, 4)]:
        for px, py, pz, rev in [("periodic", "fill", "extend", False), ("extend", "periodic", "fill", True),
                                ("fill", "extend", "fill", False), ("periodic", "periodic", "extend", True)]:
            if nz == 1 and pz == "extend" and not rev:
                continue  # (numpy cannot extend an empty cumulative field: no oracle)
            grid, ds, dims = _grid(lead, nz, ny, nx, dtype, {"X": px, "Y": py, "Z": pz}, faces=faces, area=area or "plane")
            u, v = _fields(lead, nz, ny, nx, dtype, dims)
            got = grid.vertical_velocity(u, v, fill_value=FILL, reverse=rev, face_weighted=True, metric_weighted=area is not None)
            _same(got, _want(u.values, v.values, px, py, pz, rev, faces=_face_areas(ds, faces),
                             area=_area(ds, area) if area else None))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("face_weighted", [False, True])
def test_nan_divergence_counts_as_zero(host_abi, dtype, face_weighted):
    for px, py, pz, rev in PADS:
        grid, ds, dims = _grid((2,), 5, 7, 9, dtype, {"X": px, "Y": py, "Z": pz})
        u, v = _fields((2,), 5, 7, 9, dtype, dims, nan=True)
        got = grid.vertical_velocity(u, v, fill_value=FILL, reverse=rev, face_weighted=face_weighted)
        want = _want(u.values, v.values, px, py, pz, rev, faces=_face_areas(ds, "factors") if face_weighted else None,
                     area=_area(ds, "plane"))
        _same(got, want)
        assert not np.isnan(got.values).any()  # the sum never stays NaN (the areas hold none)


@pytest.mark.parametrize("dtype,bits", [(np.float64, np.int64), (np.float32, np.int32)])
@pytest.mark.parametrize("rev", [False, True])
def test_signed_zeros_are_the_chains(host_abi, dtype, bits, rev):
    """u = +0.0 at even i and -0.0 at odd i (v likewise along j), periodic: the divergence of a cell at even (j, i) is
    (-0.0 - +0.0) + (-0.0 - +0.0) = -0.0 on every level, +0.0 elsewhere.  The first sum is d itself, not 0 + d, so the sign
    bits of such columns tell the two apart; the Z pad is -0.0 as well."""
    fill = {"X": 0.0, "Y": 0.0, "Z": -0.0}
    for nz, ny, nx in [(4, 2, 2), (3, 4, 6), (5, 2, 4), (1, 2, 2)]:
        for pz in ZBCS:
            if nz == 1 and pz == "extend" and not rev:
                continue  # (numpy cannot extend an empty cumulative field: no oracle)
            grid, ds, dims = _grid((), nz, ny, nx, dtype, {"X": "periodic", "Y": "periodic", "Z": pz})
            uu, vv = np.zeros((nz, ny, nx), dtype), np.zeros((nz, ny, nx), dtype)
            uu[:, :, 1::2] = -0.0
            vv[:, 1::2, :] = -0.0
            u, v = DataArray(uu, ("ZC", "YC", "XG")), DataArray(vv, ("ZC", "YG", "XC"))
            d = R.divergence(uu, vv, 1.0, "periodic", "periodic", 0.0, 0.0)
            assert np.signbit(d[:, ::2, ::2]).all() and not np.signbit(d[:, 1::2, :]).any()
            got = grid.vertical_velocity(u, v, fill_value=fill, reverse=rev, metric_weighted=False).values
            want = _want(uu, vv, "periodic", "periodic", pz, rev, fill=fill)
            assert got.dtype == want.dtype and np.array_equal(got.view(bits), want.view(bits))
            assert nz == 1 or (np.signbit(want).any() and not np.signbit(want).all())


def _chain(grid, u, v, x_axis="X", y_axis="Y", z_axis="Z", padding=None, fill_value=None, reverse=False,
           face_weighted=False, metric_weighted=True):
    kw = dict(padding=padding, fill_value=fill_value)
    if face_weighted:
        u = u * grid.get_metric(u, (y_axis, z_axis))
        v = v * grid.get_metric(v, (x_axis, z_axis))
    d = grid.divergence(u, v, x_axis, y_axis, metric_weighted=False, **kw)
    w = -grid.cumsum(d, z_axis, to="left", reverse=reverse, **kw)
    if metric_weighted:
        w = w / grid.get_metric(w, (x_axis, y_axis))
    return w


def _same_labelled(got, want):
    assert tuple(got.dims) == tuple(want.dims) and got.shape == want.shape and got.name == want.name
    assert list(got.coords) == list(want.coords)
    assert dict(got.attrs) == dict(want.attrs)
    for k in want.coords:
        assert got.coords[k].dims == want.coords[k].dims
        assert np.array_equal(np.asarray(got.coords[k].values), np.asarray(want.coords[k].values))
    g, w = np.asarray(got.values), np.asarray(want.values)
    assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=True)


@pytest.mark.parametrize("face_weighted", [True, False])
@pytest.mark.parametrize("metric_weighted", [True, False])
@pytest.mark.parametrize("faces", ["factors", "registered"])
@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("same_names", [True, False])
def test_dims_coords_and_name_are_the_chains(host_abi, monkeypatch, face_weighted, metric_weighted, faces, rev, same_names):
    """fused through the host ABI first, then the chain itself through Grid over the oracle double (installed after the
    fused call has run): same values, dims, coords, name and attrs"""
    from oracle import fake_device

    grid, ds, dims = _grid((2,), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"}, faces=faces)
    u, v = _fields((2,), 3, 5, 6, np.float64, dims)
    if same_names:
        u, v = (a._replace(name="q") for a in (u, v))
    u = u.assign_coords({"lon_u": (("YC", "XG"), np.ones((5, 6))), "tu": (("time",), np.arange(2) + 7.0),
                         "depth": (("ZC",), np.arange(3) * 10.0)})
    v = v.assign_coords({"tv": (("time",), np.arange(2) - 1.0), "hFacS": (("ZC", "YG", "XC"), np.ones((3, 5, 6)))})
    kw = dict(fill_value=FILL, reverse=rev, face_weighted=face_weighted, metric_weighted=metric_weighted)
    got = grid.vertical_velocity(u, v, **kw)
    fake_device.install(monkeypatch)
    _same_labelled(got, _chain(grid, u, v, **kw))


def test_xarray_in_xarray_out(host_abi, monkeypatch):
    import xarray_standin
    from oracle import fake_device

    xarray_standin.install(monkeypatch)
    import xarray as xr

    grid, ds, dims = _grid((), 3, 4, 6, np.float64, {"X": "periodic", "Y": "fill", "Z": "extend"})
    u, v = _fields((), 3, 4, 6, np.float64, dims)
    xs = [xr.DataArray(a.values, dims=a.dims, name=a.name) for a in (u, v)]
    got = grid.vertical_velocity(*xs, fill_value=FILL)
    assert type(got).__module__.split(".")[0] == "xarray"
    fake_device.install(monkeypatch)
    want = _chain(grid, u, v, fill_value=FILL)
    assert tuple(got.dims) == tuple(want.dims) and got.name == want.name
    assert np.array_equal(np.asarray(got.values), np.asarray(want.values))


def test_the_fused_entry_runs_alone(host_abi, monkeypatch):
    """one call of the fused device entry and none of the chain's operators"""
    import xgcm_amd.device as D

    grid, ds, dims = _grid((2,), 3, 5, 6, np.float64, {"X": "periodic", "Y": "fill", "Z": "extend"})
    u, v = _fields((2,), 3, 5, 6, np.float64, dims)
    calls = {"fused": 0, "chain": 0}

    def counted(fn, key):
        def wrapped(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(D, "vertical_velocity", counted(D.vertical_velocity, "fused"))
    for name in ("divergence", "binary", "stencil1d", "cumsum1d"):
        monkeypatch.setattr(D, name, counted(getattr(D, name), "chain"))
    for rev in (False, True):
        got = grid.vertical_velocity(u, v, fill_value=FILL, reverse=rev, face_weighted=True)
        _same(got, _want(u.values, v.values, "periodic", "fill", "extend", rev, faces=_face_areas(ds, "factors"),
                         area=_area(ds, "plane")))
    assert calls == {"fused": 2, "chain": 0}


def test_closes_continuity_with_flux_divergence_3d(host_abi):
    """forward mode, Z `fill` 0, transports: with a tracer of ones, flux_divergence_3d(u, v, w, 1) = d[k] + (w[k+1] - w[k]) is
    zero to rounding on levels 0 .. nz-2 (on the last one that operator pads w beyond the column).  Bound: three roundings
    (the sum that formed w[k+1], the difference w[k+1] - w[k], the final sum), each at most half an ulp of a magnitude
    <= 2 max|w| of the column, i.e. 3 * eps * max|w|."""
    nz, ny, nx = 12, 9, 16
    eps = np.finfo(np.float64).eps
    for seed in range(20):
        grid, ds, dims = _grid((), nz, ny, nx, np.float64, {"X": "periodic", "Y": "periodic", "Z": "fill"})
        u = DataArray(R.synthetic_field((nz, ny, nx), 100 + 2 * seed), ("ZC", "YC", "XG"))
        v = DataArray(R.synthetic_field((nz, ny, nx), 101 + 2 * seed), ("ZC", "YG", "XC"))
        w = grid.vertical_velocity(u, v, fill_value=0.0, metric_weighted=False)
        assert w.dims == ("ZL", "YC", "XC")
        ones = DataArray(np.ones((nz, ny, nx)), ("ZC", "YC", "XC"))
        res = np.asarray(grid.flux_divergence_3d(u, v, w, ones, fill_value=0.0, metric_weighted=False).values)
        wmax = np.abs(np.asarray(w.values)).max(axis=0)
        ratio = (np.abs(res[:-1]) / (eps * wmax)).max()
        print(f"seed {seed}: max |residual| / (eps * max|w|) = {ratio:.3f}")
        assert (np.abs(res[:-1]) <= 3 * eps * wmax).all()


# ---- fallbacks: the chain itself (existing device functions only) ------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int64, np.int32, np.float16])
def test_integer_and_half_fields_run_the_chain(backend, dtype):
    grid, ds, dims = _grid((), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    vals = lambda seed: (R.synthetic_field((3, 5, 6), seed) * 100).astype(dtype)  # noqa: E731
    u, v = DataArray(vals(1), ("ZC", "YC", "XG")), DataArray(vals(2), ("ZC", "YG", "XC"))
    for kw in (dict(), dict(metric_weighted=False), dict(reverse=True, face_weighted=True)):
        _same_labelled(grid.vertical_velocity(u, v, **kw), _chain(grid, u, v, **kw))


def test_mixed_dtypes_run_the_chain(backend):
    pad = {"X": "fill", "Y": "periodic", "Z": "extend"}
    grid, ds, dims = _grid((), 3, 5, 6, np.float64, pad)
    u, v = _fields((), 3, 5, 6, np.float64, dims)
    v32 = DataArray(v.values.astype(np.float32), v.dims)
    _same_labelled(grid.vertical_velocity(u, v32, fill_value=FILL), _chain(grid, u, v32, fill_value=FILL))
    # float32 fields over float64 metrics
    u32, v32 = _fields((), 3, 5, 6, np.float32, dims)
    for kw in (dict(), dict(face_weighted=True, reverse=True)):
        _same_labelled(grid.vertical_velocity(u32, v32, fill_value=FILL, **kw), _chain(grid, u32, v32, fill_value=FILL, **kw))


def test_z_not_third_last_runs_the_chain(backend):
    grid, ds, dims = _grid((2,), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    u, v = _fields((2,), 3, 5, 6, np.float64, dims)
    u, v = (a.transpose(a.dims[1], a.dims[0], *a.dims[2:]) for a in (u, v))
    _same_labelled(grid.vertical_velocity(u, v, fill_value=FILL), _chain(grid, u, v, fill_value=FILL))


def test_chunked_input_runs_the_chain(backend):
    grid, ds, dims = _grid((4,), 3, 6, 8, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    u, v = _fields((4,), 3, 6, 8, np.float64, dims)
    chunks = ((2, 2), (3,), (6,), (8,))
    cu = DataArray(BlockArray.from_array(u.values, chunks), u.dims, name="u")
    cv = DataArray(BlockArray.from_array(v.values, chunks), v.dims, name="v")
    got = grid.vertical_velocity(cu, cv, fill_value=FILL, metric_weighted=False)
    want = _chain(grid, cu, cv, fill_value=FILL, metric_weighted=False)
    assert got.dims == want.dims and got.name == want.name
    assert np.array_equal(np.asarray(got.values), np.asarray(want.values))
    assert np.array_equal(np.asarray(got.values), _want(u.values, v.values, "periodic", "extend", "fill", False))


def test_periodic_z_runs_the_chain(backend):
    """summed upward with periodic Z the pad is the column total: the chain; summed downward there is no pad: one pass"""
    grid, ds, dims = _grid((2,), 4, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "periodic"})
    u, v = _fields((2,), 4, 5, 6, np.float64, dims)
    got = grid.vertical_velocity(u, v, fill_value=FILL)
    _same_labelled(got, _chain(grid, u, v, fill_value=FILL))
    _same(got, _want(u.values, v.values, "periodic", "extend", "periodic", False, area=_area(ds, "plane")))


def test_periodic_z_reverse_is_one_pass(host_abi):
    grid, ds, dims = _grid((2,), 4, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "periodic"})
    u, v = _fields((2,), 4, 5, 6, np.float64, dims)
    _same(grid.vertical_velocity(u, v, fill_value=FILL, reverse=True),
          _want(u.values, v.values, "periodic", "extend", "periodic", True, area=_area(ds, "plane")))


def test_connected_faces_run_the_chain(backend):
    from test_topology import COORDS, X_TO_X

    ds = Dataset(coords={"x": np.arange(4), "xl": np.arange(4) - 0.5, "y": np.arange(4), "yl": np.arange(4) - 0.5,
                         "face": np.arange(2), "zc": np.arange(3) + 0.5, "zl": np.arange(3) * 1.0})
    grid = Grid(ds, coords=dict(COORDS, Z={"center": "zc", "left": "zl"}), face_connections=X_TO_X,
                padding={"X": "fill", "Y": "extend", "Z": "fill"}, autoparse_metadata=False)
    f = lambda seed, dims: DataArray(R.synthetic_field((2, 3, 4, 4), seed), dims)  # noqa: E731
    u, v = f(82, ("face", "zc", "y", "xl")), f(83, ("face", "zc", "yl", "x"))
    for rev in (False, True):
        _same_labelled(grid.vertical_velocity(u, v, reverse=rev, metric_weighted=False),
                       _chain(grid, u, v, reverse=rev, metric_weighted=False))


def test_misplaced_inputs_raise(backend):
    grid, ds, dims = _grid((), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    u, v = _fields((), 3, 5, 6, np.float64, dims)
    w = DataArray(u.values, ("ZL", "YC", "XG"))
    with pytest.raises(NotImplementedError, match="X:left"):
        grid.vertical_velocity(v, u)
    with pytest.raises(NotImplementedError, match="Z:center"):
        grid.vertical_velocity(w, v)
    with pytest.raises(NotImplementedError):
        grid.vertical_velocity(u, u)


def test_missing_z_boundary_raises_the_chains_error(backend):
    grid, ds, dims = _grid((), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    u, v = _fields((), 3, 5, 6, np.float64, dims)
    bare = Grid(ds, coords=AXES, padding={"X": "periodic", "Y": "extend"}, autoparse_metadata=False)
    with pytest.raises(Exception) as fused_err:
        bare.vertical_velocity(u, v, metric_weighted=False)
    with pytest.raises(Exception) as chain_err:
        _chain(bare, u, v, metric_weighted=False)
    assert type(fused_err.value) is type(chain_err.value) and str(fused_err.value) == str(chain_err.value)


def test_one_level_extended_upward_raises_the_chains_error(host_abi):
    """nz = 1 summed upward: the cumulative field is empty after the trim and `extend` has nothing to repeat"""
    grid, ds, dims = _grid((), 1, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "extend"})
    u, v = _fields((), 1, 5, 6, np.float64, dims)
    with pytest.raises(ValueError) as fused_err:
        grid.vertical_velocity(u, v, metric_weighted=False)
    with pytest.raises(ValueError) as chain_err:
        _chain(grid, u, v, metric_weighted=False)
    assert str(fused_err.value) == str(chain_err.value)
