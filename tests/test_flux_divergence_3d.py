"""Fused 3-D tracer flux divergence `Grid.flux_divergence_3d` on CPU.

The one-pass path runs through the `host_abi` fixture (the product's `xgcm_amd.device` over libxgcm_host.so) and is
compared bit for bit with the oracle composing the chain the operator replaces:

    fx, fy = R.flux(u, v, T);  fz = R.binary("mul", w, R.stencil1d("interp", T, Z, 1, 0))
    out = R.divergence(fx, fy, area=1.0) + R.stencil1d("diff", fz, Z, 0, 1)  [/ vol]

(`R.divergence` always divides: area = 1.0 is exact.)  The chain pads twice on every axis -- the tracer center -> left,
then the fluxes left -> center -- and that is what the boundary matrix exercises.  The fallbacks only call existing
device functions and run under the `backend` double."""

import itertools
import warnings

import numpy as np
import pytest

from oracle import refimpl as R
from xgcm_amd import DataArray, Dataset, Grid

BCS = ["periodic", "extend", "fill"]
FILL = {"X": 1.75, "Y": -0.625, "Z": 0.375}
AXES = {"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"}, "Z": {"center": "ZC", "left": "ZL"}}


def _grid(lead, nz, ny, nx, dtype, padding, volume="product"):
    """C-grid with a Z axis; the volume is rA(Y, X) * drF(Z) formed by the grid, or a registered (Z, Y, X) `vol`"""
    dims = ("time",)[:len(lead)]
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0),
              "YC": ("YC", np.arange(ny) + 0.5), "YG": ("YG", np.arange(ny) * 1.0),
              "ZC": ("ZC", -np.arange(nz) - 0.5), "ZL": ("ZL", -np.arange(nz) * 1.0)}
    for d, n in zip(dims, lead):
        coords[d] = (d, np.arange(n) * 2.0)
    data = {"rA": (("YC", "XC"), R.synthetic_metric((ny, nx), 65).astype(dtype)),
            "drF": (("ZC",), R.synthetic_metric((nz,), 66).astype(dtype))}
    metrics = {("X", "Y"): ["rA"], ("Z",): ["drF"]}
    if volume == "registered":
        data["vol"] = (("ZC", "YC", "XC"), R.synthetic_metric((nz, ny, nx), 67).astype(dtype))
        metrics[("X", "Y", "Z")] = ["vol"]
    ds = Dataset(data, coords)
    grid = Grid(ds, coords=AXES, metrics=metrics, padding=padding, autoparse_metadata=False)
    return grid, ds, dims


def _fields(lead, nz, ny, nx, dtype, dims, nan=False):
    shape = tuple(lead) + (nz, ny, nx)
    f = lambda seed: R.synthetic_field(shape, seed).astype(dtype)  # noqa: E731
    t, u, v, w = f(71), f(72), f(73), f(74)
    if nan:
        t.reshape(-1)[::7] = np.nan
        u.reshape(-1)[3::11] = np.nan
        w.reshape(-1)[5::13] = np.nan
    return (DataArray(u, dims + ("ZC", "YC", "XG"), name="u"), DataArray(v, dims + ("ZC", "YG", "XC"), name="v"),
            DataArray(w, dims + ("ZL", "YC", "XC"), name="w"), DataArray(t, dims + ("ZC", "YC", "XC"), name="T"))


def _volume(ds, volume):
    """the volume as get_metric forms it, broadcast against (Z, Y, X)"""
    if volume == "registered":
        return np.asarray(ds["vol"].values)
    return R.binary("mul", np.asarray(ds["rA"].values)[None], np.asarray(ds["drF"].values)[:, None, None])


def _want(u, v, w, t, px, py, pz, vol, fill=FILL):
    zax = t.ndim - 3
    fx, fy = R.flux(u, v, t, px, py, fill["X"], fill["Y"])
    fz = R.binary("mul", w, R.stencil1d("interp", t, zax, 1, 0, pz, fill["Z"]))
    out = R.divergence(fx, fy, 1.0, px, py, fill["X"], fill["Y"]) + R.stencil1d("diff", fz, zax, 0, 1, pz, fill["Z"])
    return out if vol is None else out / vol


def _same(got, want):
    got = np.asarray(got.values if hasattr(got, "values") else got)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got, want, equal_nan=True)


def _values(*arrays):
    return tuple(a.values for a in arrays)


# (lead, nz, ny, nx): odd nx, ny not a multiple of the 2-row segment, nz / ny / nx of 1, a 4-D lead dim
SHAPES = [((), 4, 6, 8), ((), 3, 7, 5), ((), 1, 5, 9), ((), 5, 1, 6), ((), 4, 6, 1), ((2,), 3, 5, 4), ((), 1, 1, 1),
          ((2,), 2, 3, 7)]
PADS = list(itertools.product(BCS, BCS, BCS))


@pytest.mark.parametrize("px,py,pz", PADS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("weighted", [True, False])
def test_equals_the_oracle_chain(host_abi, px, py, pz, dtype, weighted):
    for lead, nz, ny, nx in SHAPES:
        grid, ds, dims = _grid(lead, nz, ny, nx, dtype, {"X": px, "Y": py, "Z": pz})
        u, v, w, t = _fields(lead, nz, ny, nx, dtype, dims)
        got = grid.flux_divergence_3d(u, v, w, t, fill_value=FILL, metric_weighted=weighted)
        _same(got, _want(*_values(u, v, w, t), px, py, pz, _volume(ds, "product") if weighted else None))


@pytest.mark.parametrize("volume", ["product", "registered"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_volume_registered_or_formed_from_area_and_thickness(host_abi, volume, dtype):
    for lead, nz, ny, nx in [((), 4, 6, 8), ((2,), 3, 5, 7), ((), 1, 1, 1)]:
        for px, py, pz in [("periodic", "fill", "extend"), ("extend", "periodic", "fill"), ("fill", "extend", "periodic")]:
            grid, ds, dims = _grid(lead, nz, ny, nx, dtype, {"X": px, "Y": py, "Z": pz}, volume=volume)
            u, v, w, t = _fields(lead, nz, ny, nx, dtype, dims)
            got = grid.flux_divergence_3d(u, v, w, t, fill_value=FILL)
            _same(got, _want(*_values(u, v, w, t), px, py, pz, _volume(ds, volume)))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_nan_cells_propagate_as_in_the_chain(host_abi, dtype):
    for px, py, pz in PADS:
        grid, ds, dims = _grid((2,), 3, 7, 9, dtype, {"X": px, "Y": py, "Z": pz})
        u, v, w, t = _fields((2,), 3, 7, 9, dtype, dims, nan=True)
        _same(grid.flux_divergence_3d(u, v, w, t, fill_value=FILL),
              _want(*_values(u, v, w, t), px, py, pz, _volume(ds, "product")))


def test_z_fill_value_reaches_both_stages(host_abi):
    """fill along Z: the tracer above level 0 AND the vertical flux below the last level take the fill value itself"""
    grid, ds, dims = _grid((), 3, 4, 6, np.float64, {"X": "periodic", "Y": "periodic", "Z": "fill"})
    u, v, w, t = _fields((), 3, 4, 6, np.float64, dims)
    zu, zv = DataArray(np.zeros(u.shape), u.dims), DataArray(np.zeros(v.shape), v.dims)
    got = grid.flux_divergence_3d(zu, zv, w, t, fill_value=FILL, metric_weighted=False).values
    above = np.concatenate([np.full((1, 4, 6), FILL["Z"]), t.values[:-1]])
    fz = w.values * ((above + t.values) * 0.5)
    assert np.array_equal(got[-1], 0.0 + (FILL["Z"] - fz[-1]))
    assert np.array_equal(got[0], 0.0 + (fz[1] - fz[0]))


def test_negated_w_is_exact(host_abi):
    """a Z index growing downward with w positive upward: passing -w is the chain on -w, bit for bit"""
    grid, ds, dims = _grid((), 4, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    u, v, w, t = _fields((), 4, 5, 6, np.float64, dims)
    nw = DataArray(-w.values, w.dims)
    _same(grid.flux_divergence_3d(u, v, nw, t, fill_value=FILL),
          _want(u.values, v.values, -w.values, t.values, "periodic", "extend", "fill", _volume(ds, "product")))


def _chain(grid, u, v, w, t, x_axis="X", y_axis="Y", z_axis="Z", padding=None, fill_value=None, metric_weighted=True):
    kw = dict(padding=padding, fill_value=fill_value)
    fx, fy = grid.flux(u, v, t, x_axis, y_axis, **kw)
    fz = w * grid.interp(t, z_axis, **kw)
    h = grid.divergence(fx, fy, x_axis, y_axis, metric_weighted=False, **kw)
    out = h + grid.diff(fz, z_axis, **kw)
    if metric_weighted:
        out = out / grid.get_metric(out, (x_axis, y_axis, z_axis))
    return out


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
@pytest.mark.parametrize("volume", ["product", "registered"])
@pytest.mark.parametrize("same_names", [True, False])
def test_dims_coords_and_name_are_the_chains(host_abi, monkeypatch, weighted, volume, same_names):
    """fused through the host ABI first, then the chain itself through Grid over the oracle double (installed after the
    fused call has run): same values, dims, coords, name and attrs"""
    from oracle import fake_device

    grid, ds, dims = _grid((2,), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"}, volume=volume)
    u, v, w, t = _fields((2,), 3, 5, 6, np.float64, dims)
    if same_names:
        u, v, w, t = (a._replace(name="T") for a in (u, v, w, t))
    u = u.assign_coords({"lon_u": (("YC", "XG"), np.ones((5, 6))), "tu": (("time",), np.arange(2) + 7.0)})
    w = w.assign_coords({"depth_w": (("ZL",), np.arange(3) * 10.0)})
    t = t.assign_coords({"tt": (("time",), np.arange(2) - 1.0), "hFacC": (("ZC", "YC", "XC"), np.ones((3, 5, 6)))})
    got = grid.flux_divergence_3d(u, v, w, t, fill_value=FILL, metric_weighted=weighted)
    fake_device.install(monkeypatch)
    _same_labelled(got, _chain(grid, u, v, w, t, fill_value=FILL, metric_weighted=weighted))


def test_xarray_in_xarray_out(host_abi, monkeypatch):
    import xarray_standin
    from oracle import fake_device

    xarray_standin.install(monkeypatch)
    import xarray as xr

    grid, ds, dims = _grid((), 3, 4, 6, np.float64, {"X": "periodic", "Y": "fill", "Z": "extend"})
    u, v, w, t = _fields((), 3, 4, 6, np.float64, dims)
    xs = [xr.DataArray(a.values, dims=a.dims, name=a.name) for a in (u, v, w, t)]
    got = grid.flux_divergence_3d(*xs, fill_value=FILL)
    assert type(got).__module__.split(".")[0] == "xarray"
    fake_device.install(monkeypatch)
    want = _chain(grid, u, v, w, t, fill_value=FILL)
    assert tuple(got.dims) == tuple(want.dims) and got.name == want.name
    assert np.array_equal(np.asarray(got.values), np.asarray(want.values))


def test_the_fused_entry_runs_alone(host_abi, monkeypatch):
    """one call of the fused device entry and none of the chain's operators"""
    import xgcm_amd.device as D

    grid, ds, dims = _grid((2,), 3, 5, 6, np.float64, {"X": "periodic", "Y": "fill", "Z": "periodic"})
    u, v, w, t = _fields((2,), 3, 5, 6, np.float64, dims)
    want = _want(*_values(u, v, w, t), "periodic", "fill", "periodic", _volume(ds, "product"))
    calls = {"fused": 0, "chain": 0}

    def counted(fn, key):
        def wrapped(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(D, "flux_divergence_3d", counted(D.flux_divergence_3d, "fused"))
    for name in ("flux", "divergence", "binary", "stencil1d", "flux_divergence"):
        monkeypatch.setattr(D, name, counted(getattr(D, name), "chain"))
    _same(grid.flux_divergence_3d(u, v, w, t, fill_value=FILL), want)
    assert calls == {"fused": 1, "chain": 0}


# ---- fallbacks: the chain itself (existing device functions only) ------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int64, np.int32])
def test_integer_fields_run_the_chain(backend, dtype):
    grid, ds, dims = _grid((), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    ints = lambda seed: (R.synthetic_field((3, 5, 6), seed) * 100).astype(dtype)  # noqa: E731
    u = DataArray(ints(1), ("ZC", "YC", "XG"))
    v = DataArray(ints(2), ("ZC", "YG", "XC"))
    w = DataArray(ints(3), ("ZL", "YC", "XC"))
    t = DataArray(ints(4), ("ZC", "YC", "XC"))
    for mw in (True, False):
        _same_labelled(grid.flux_divergence_3d(u, v, w, t, metric_weighted=mw), _chain(grid, u, v, w, t, metric_weighted=mw))


def test_mixed_dtypes_run_the_chain(backend):
    pad = {"X": "fill", "Y": "periodic", "Z": "extend"}
    grid, ds, dims = _grid((), 3, 5, 6, np.float64, pad)
    u, v, w, t = _fields((), 3, 5, 6, np.float64, dims)
    w32 = DataArray(w.values.astype(np.float32), w.dims)
    _same_labelled(grid.flux_divergence_3d(u, v, w32, t, fill_value=FILL), _chain(grid, u, v, w32, t, fill_value=FILL))
    # float32 fields over float64 metrics
    u32, v32, w32, t32 = _fields((), 3, 5, 6, np.float32, dims)
    _same_labelled(grid.flux_divergence_3d(u32, v32, w32, t32, fill_value=FILL),
                   _chain(grid, u32, v32, w32, t32, fill_value=FILL))


def test_z_not_third_last_runs_the_chain(backend):
    grid, ds, dims = _grid((2,), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    u, v, w, t = _fields((2,), 3, 5, 6, np.float64, dims)
    u, v, w, t = (a.transpose(a.dims[1], a.dims[0], *a.dims[2:]) for a in (u, v, w, t))
    _same_labelled(grid.flux_divergence_3d(u, v, w, t, fill_value=FILL), _chain(grid, u, v, w, t, fill_value=FILL))


def test_connected_faces_run_the_chain(backend):
    from test_topology import COORDS, X_TO_X

    ds = Dataset(coords={"x": np.arange(4), "xl": np.arange(4) - 0.5, "y": np.arange(4), "yl": np.arange(4) - 0.5,
                         "face": np.arange(2), "zc": np.arange(3) + 0.5, "zl": np.arange(3) * 1.0})
    grid = Grid(ds, coords=dict(COORDS, Z={"center": "zc", "left": "zl"}), face_connections=X_TO_X,
                padding={"X": "fill", "Y": "extend", "Z": "periodic"}, autoparse_metadata=False)
    f = lambda seed, dims: DataArray(R.synthetic_field((2, 3, 4, 4), seed), dims)  # noqa: E731
    t = f(80, ("face", "zc", "y", "x"))
    u, v, w = f(82, ("face", "zc", "y", "xl")), f(83, ("face", "zc", "yl", "x")), f(84, ("face", "zl", "y", "x"))
    _same_labelled(grid.flux_divergence_3d(u, v, w, t, metric_weighted=False),
                   _chain(grid, u, v, w, t, metric_weighted=False))


def test_fold_grid_runs_the_chain(backend):
    from test_topology import Nx, Ny

    ds = Dataset(coords={"xh": np.arange(Nx), "xl": np.arange(Nx), "yh": np.arange(Ny), "yl": np.arange(Ny),
                         "zc": np.arange(2) + 0.5, "zl": np.arange(2) * 1.0})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        grid = Grid(ds, coords={"X": {"center": "xh", "left": "xl"}, "Y": {"center": "yh", "left": "yl"},
                                "Z": {"center": "zc", "left": "zl"}},
                    padding={"X": "periodic", "Y": {"fold": "corner"}, "Z": "extend"}, autoparse_metadata=False)
    f = lambda seed, dims: DataArray(R.synthetic_field((2, Ny, Nx), seed), dims)  # noqa: E731
    t = f(91, ("zc", "yh", "xh"))
    u, v, w = f(92, ("zc", "yh", "xl")), f(93, ("zc", "yl", "xh")), f(94, ("zl", "yh", "xh"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        _same_labelled(grid.flux_divergence_3d(u, v, w, t, metric_weighted=False),
                       _chain(grid, u, v, w, t, metric_weighted=False))


def test_misplaced_inputs_raise(backend):
    grid, ds, dims = _grid((), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    u, v, w, t = _fields((), 3, 5, 6, np.float64, dims)
    with pytest.raises(NotImplementedError):
        grid.flux_divergence_3d(v, u, w, t)
    with pytest.raises(NotImplementedError):
        grid.flux_divergence_3d(u, v, t, t)
    with pytest.raises(NotImplementedError):
        grid.flux_divergence_3d(u, v, w, w)


def test_missing_z_boundary_raises_the_chains_error(backend):
    grid, ds, dims = _grid((), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    u, v, w, t = _fields((), 3, 5, 6, np.float64, dims)
    bare = Grid(ds, coords=AXES, padding={"X": "periodic", "Y": "extend"}, autoparse_metadata=False)
    with pytest.raises(Exception) as fused_err:
        bare.flux_divergence_3d(u, v, w, t, metric_weighted=False)
    with pytest.raises(Exception) as chain_err:
        _chain(bare, u, v, w, t, metric_weighted=False)
    assert type(fused_err.value) is type(chain_err.value) and str(fused_err.value) == str(chain_err.value)
