"""Fused second-order operators `Grid.flux_divergence` / `Grid.laplacian` on CPU.

The one-pass path runs through the `host_abi` fixture (the product's `xgcm_amd.device` over libxgcm_host.so) and is
compared bit for bit with the oracle composing the chain the operator replaces:

    flux_divergence:  R.divergence(*R.flux(u, v, T), area)
    laplacian:        R.gradient(a, mx=dxC, my=dyC) -> R.binary("mul", ., dyG / dxG) -> R.divergence(., rA)

(`R.divergence` always divides: the unweighted forms pass area = 1.0, which is exact.)  The chain's two boundaries --
the field padded center -> left, the intermediate left -> center -- are what the matrix below exercises.  The fallbacks
(integers, connected faces, a fold) only call existing device functions and run under the `backend` double."""

import itertools
import warnings

import numpy as np
import pytest

from oracle import refimpl as R
from xgcm_amd import DataArray, Dataset, Grid

BCS = ["periodic", "extend", "fill"]
FILL = {"X": 1.75, "Y": -0.625}
LEAD_NAMES = ("Z", "face")


def _grid(lead, ny, nx, dtype, padding, met_lead=()):
    """C-grid with the metrics of both operators: dxC / dyG at (YC, XG), dyC / dxG at (YG, XC), rA at the centre; the
    metrics carry the leading dims `met_lead` (a subset of the field's, broadcast over the others)"""
    dims = LEAD_NAMES[:len(lead)]
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0),
              "YC": ("YC", np.arange(ny) + 0.5), "YG": ("YG", np.arange(ny) * 1.0)}
    for d, n in zip(dims, lead):
        coords[d] = (d, np.arange(n) * 2.0)
    mdims = tuple(d for d in dims if d in met_lead)
    mshape = tuple(n for d, n in zip(dims, lead) if d in met_lead) + (ny, nx)
    m = lambda seed: R.synthetic_metric(mshape, seed).astype(dtype)  # noqa: E731
    ds = Dataset({"dxC": (mdims + ("YC", "XG"), m(61)), "dyG": (mdims + ("YC", "XG"), m(62)),
                  "dyC": (mdims + ("YG", "XC"), m(63)), "dxG": (mdims + ("YG", "XC"), m(64)),
                  "rA": (mdims + ("YC", "XC"), m(65))}, coords)
    grid = Grid(ds, coords={"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"}},
                metrics={("X",): ["dxC", "dxG"], ("Y",): ["dyC", "dyG"], ("X", "Y"): ["rA"]},
                padding=padding, autoparse_metadata=False)
    return grid, ds, dims


def _fields(lead, ny, nx, dtype, dims, nan=False):
    shape = tuple(lead) + (ny, nx)
    f = lambda seed: R.synthetic_field(shape, seed).astype(dtype)  # noqa: E731
    t, u, v = f(71), f(72), f(73)
    if nan:
        t.reshape(-1)[::7] = np.nan
        u.reshape(-1)[3::11] = np.nan
    return (DataArray(u, dims + ("YC", "XG"), name="u"), DataArray(v, dims + ("YG", "XC"), name="v"),
            DataArray(t, dims + ("YC", "XC"), name="T"))


def _want_flux_div(u, v, t, px, py, area, fill=FILL):
    fx, fy = R.flux(u, v, t, px, py, fill["X"], fill["Y"])
    return R.divergence(fx, fy, area, px, py, fill["X"], fill["Y"])


def _want_laplacian(a, px, py, met, fill=FILL):
    if met is None:
        gx, gy = R.gradient(a, px, py, fill["X"], fill["Y"])
        return R.divergence(gx, gy, 1.0, px, py, fill["X"], fill["Y"])
    gx, gy = R.gradient(a, px, py, fill["X"], fill["Y"], mx=met["dxC"], my=met["dyC"])
    gx, gy = R.binary("mul", gx, met["dyG"]), R.binary("mul", gy, met["dxG"])
    return R.divergence(gx, gy, met["rA"], px, py, fill["X"], fill["Y"])


def _metric_arrays(ds, dims, met_lead):
    """the metrics as numpy arrays that broadcast against (*lead, Y, X) fields"""
    out = {}
    for k in ("dxC", "dyG", "dyC", "dxG", "rA"):
        a = np.asarray(ds[k].values)
        idx = tuple(slice(None) if d in met_lead else np.newaxis for d in dims)
        out[k] = a[idx] if idx else a
    return out


def _same(got, want):
    got = np.asarray(got.values if hasattr(got, "values") else got)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got, want, equal_nan=True)


# shapes: odd nx, ny not a multiple of the 2-row segment, nx or ny equal to 1; 2-D, 3-D and 4-D
SHAPES = [((), 6, 8), ((), 7, 5), ((3,), 5, 9), ((2,), 1, 6), ((2,), 6, 1), ((2, 3), 5, 4), ((1,), 1, 1)]
PADS = [(px, py) for px in BCS for py in BCS]


@pytest.mark.parametrize("px,py", PADS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("weighted", [True, False])
def test_flux_divergence_equals_the_oracle_chain(host_abi, px, py, dtype, weighted):
    for lead, ny, nx in SHAPES:
        grid, ds, dims = _grid(lead, ny, nx, dtype, {"X": px, "Y": py})
        u, v, t = _fields(lead, ny, nx, dtype, dims)
        got = grid.flux_divergence(u, v, t, fill_value=FILL, metric_weighted=weighted)
        area = _metric_arrays(ds, dims, ())["rA"] if weighted else 1.0
        _same(got, _want_flux_div(u.values, v.values, t.values, px, py, area))


@pytest.mark.parametrize("px,py", PADS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("weighted", [True, False])
def test_laplacian_equals_the_oracle_chain(host_abi, px, py, dtype, weighted):
    for lead, ny, nx in SHAPES:
        grid, ds, dims = _grid(lead, ny, nx, dtype, {"X": px, "Y": py})
        _, _, a = _fields(lead, ny, nx, dtype, dims)
        got = grid.laplacian(a, padding={"X": px, "Y": py}, fill_value=FILL, metric_weighted=weighted)
        _same(got, _want_laplacian(a.values, px, py, _metric_arrays(ds, dims, ()) if weighted else None))


@pytest.mark.parametrize("met_lead", [(), ("face",), ("Z", "face")])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_4d_fields_with_metrics_broadcast_over_leading_dims(host_abi, met_lead, dtype):
    lead, ny, nx = (3, 2), 5, 6
    for px, py in [("periodic", "fill"), ("extend", "periodic"), ("fill", "extend")]:
        grid, ds, dims = _grid(lead, ny, nx, dtype, {"X": px, "Y": py}, met_lead=met_lead)
        u, v, t = _fields(lead, ny, nx, dtype, dims)
        met = _metric_arrays(ds, dims, met_lead)
        _same(grid.flux_divergence(u, v, t, fill_value=FILL),
              _want_flux_div(u.values, v.values, t.values, px, py, met["rA"]))
        _same(grid.laplacian(t, fill_value=FILL), _want_laplacian(t.values, px, py, met))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_nan_cells_propagate_as_in_the_chain(host_abi, dtype):
    lead, ny, nx = (2,), 7, 9
    for px, py in itertools.product(BCS, BCS):
        grid, ds, dims = _grid(lead, ny, nx, dtype, {"X": px, "Y": py})
        u, v, t = _fields(lead, ny, nx, dtype, dims, nan=True)
        met = _metric_arrays(ds, dims, ())
        _same(grid.flux_divergence(u, v, t, fill_value=FILL), _want_flux_div(u.values, v.values, t.values, px, py, met["rA"]))
        _same(grid.laplacian(t, fill_value=FILL), _want_laplacian(t.values, px, py, met))


def test_per_axis_fill_values_reach_both_stages(host_abi):
    """fill on both axes with different values: the tracer's halo AND the intermediate's halo take them"""
    grid, ds, dims = _grid((2,), 4, 6, np.float64, {"X": "fill", "Y": "fill"})
    u, v, t = _fields((2,), 4, 6, np.float64, dims)
    got = grid.flux_divergence(u, v, t, fill_value=FILL, metric_weighted=False)
    fx, fy = R.flux(u.values, v.values, t.values, "fill", "fill", FILL["X"], FILL["Y"])
    # right / top edges of the divergence read the fill value itself, not a flux formed from filled T
    want = R.divergence(fx, fy, 1.0, "fill", "fill", FILL["X"], FILL["Y"])
    assert np.array_equal(got.values, want)
    assert np.array_equal(got.values[..., -1], (FILL["X"] - fx[..., -1]) + R.stencil1d("diff", fy, 1, 0, 1, "fill", FILL["Y"])[..., -1])


def _chain_flux_divergence(grid, u, v, t, **kw):
    mw = kw.pop("metric_weighted", True)
    fx, fy = grid.flux(u, v, t, **kw)
    return grid.divergence(fx, fy, metric_weighted=mw, **kw)


def _chain_laplacian(grid, a, **kw):
    mw = kw.pop("metric_weighted", True)
    gx, gy = grid.gradient(a, metric_weighted=mw, **kw)
    if mw:
        gx = gx * grid.get_metric(gx, ("Y",))
        gy = gy * grid.get_metric(gy, ("X",))
    return grid.divergence(gx, gy, metric_weighted=mw, **kw)


def _same_labelled(got, want):
    assert tuple(got.dims) == tuple(want.dims) and got.shape == want.shape and got.name == want.name
    assert list(got.coords) == list(want.coords)
    for k in want.coords:
        assert got.coords[k].dims == want.coords[k].dims
        assert np.array_equal(np.asarray(got.coords[k].values), np.asarray(want.coords[k].values))
    g, w = np.asarray(got.values), np.asarray(want.values)
    assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=True)


@pytest.mark.parametrize("weighted", [True, False])
def test_dims_coords_and_name_are_the_chains(host_abi, monkeypatch, weighted):
    """fused through the host ABI first, then the chain itself through Grid over the oracle double (installed after the
    fused calls have run): same values, dims, coords and name"""
    from oracle import fake_device

    grid, ds, dims = _grid((3,), 5, 6, np.float64, {"X": "periodic", "Y": "extend"})
    u, v, t = _fields((3,), 5, 6, np.float64, dims)
    u = u.assign_coords({"lon_u": (("YC", "XG"), np.ones((5, 6))), "Zu": (("Z",), np.arange(3) + 7.0)})
    t = t.assign_coords({"Zt": (("Z",), np.arange(3) - 1.0)})
    got_fd = grid.flux_divergence(u, v, t, metric_weighted=weighted)
    got_lap = grid.laplacian(t, metric_weighted=weighted)
    fake_device.install(monkeypatch)
    _same_labelled(got_fd, _chain_flux_divergence(grid, u, v, t, metric_weighted=weighted))
    _same_labelled(got_lap, _chain_laplacian(grid, t, metric_weighted=weighted))
    assert got_lap.name is None and got_fd.dims == t.dims


def test_xarray_in_xarray_out(host_abi, monkeypatch):
    import xarray_standin
    from oracle import fake_device

    xarray_standin.install(monkeypatch)
    import xarray as xr

    grid, ds, dims = _grid((2,), 4, 6, np.float64, {"X": "periodic", "Y": "fill"})
    u, v, t = _fields((2,), 4, 6, np.float64, dims)
    xu, xv, xt = (xr.DataArray(a.values, dims=a.dims, name=a.name) for a in (u, v, t))
    got_fd = grid.flux_divergence(xu, xv, xt, fill_value=FILL)
    got_lap = grid.laplacian(xt, fill_value=FILL)
    assert type(got_fd).__name__ == "DataArray" and type(got_fd).__module__.split(".")[0] == "xarray"
    fake_device.install(monkeypatch)
    # (the stand-in has no arithmetic: the laplacian's chain runs on the labelled arrays of this package)
    for got, want in ((got_fd, _chain_flux_divergence(grid, xu, xv, xt, fill_value=FILL)),
                      (got_lap, _chain_laplacian(grid, t, fill_value=FILL))):
        assert type(got).__module__.split(".")[0] == "xarray"
        assert tuple(got.dims) == tuple(want.dims) and got.name == want.name
        assert list(got.coords) == list(want.coords)
        assert np.array_equal(np.asarray(got.values), np.asarray(want.values))


# ---- fallbacks: the chain itself (existing device functions only) ------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int64, np.int32])
def test_integer_fields_run_the_chain(backend, dtype):
    grid, ds, dims = _grid((2,), 5, 6, np.float64, {"X": "periodic", "Y": "extend"})
    shape = (2, 5, 6)
    ints = lambda seed: (R.synthetic_field(shape, seed) * 100).astype(dtype)  # noqa: E731
    u = DataArray(ints(1), dims + ("YC", "XG"))
    v = DataArray(ints(2), dims + ("YG", "XC"))
    t = DataArray(ints(3), dims + ("YC", "XC"))
    for mw in (True, False):
        _same_labelled(grid.flux_divergence(u, v, t, metric_weighted=mw), _chain_flux_divergence(grid, u, v, t, metric_weighted=mw))
        _same_labelled(grid.laplacian(t, metric_weighted=mw), _chain_laplacian(grid, t, metric_weighted=mw))


def test_mixed_dtypes_run_the_chain(backend):
    grid, ds, dims = _grid((2,), 5, 6, np.float64, {"X": "fill", "Y": "periodic"})
    u, v, t = _fields((2,), 5, 6, np.float64, dims)
    t32 = DataArray(t.values.astype(np.float32), t.dims)
    _same_labelled(grid.flux_divergence(u, v, t32, fill_value=FILL), _chain_flux_divergence(grid, u, v, t32, fill_value=FILL))
    _same_labelled(grid.laplacian(t32, fill_value=FILL), _chain_laplacian(grid, t32, fill_value=FILL))


def test_connected_faces_run_the_chain(backend):
    from test_topology import COORDS, X_TO_X, _faces_ds

    ds = _faces_ds(2, 4, seed=81)
    grid = Grid(ds, coords=COORDS, face_connections=X_TO_X, padding={"X": "fill", "Y": "extend"}, autoparse_metadata=False)
    t = ds.data_c
    u = DataArray(R.synthetic_field((2, 4, 4), 82), ("face", "y", "xl"))
    v = DataArray(R.synthetic_field((2, 4, 4), 83), ("face", "yl", "x"))
    _same_labelled(grid.flux_divergence(u, v, t, metric_weighted=False),
                   _chain_flux_divergence(grid, u, v, t, metric_weighted=False))
    _same_labelled(grid.laplacian(t, metric_weighted=False), _chain_laplacian(grid, t, metric_weighted=False))


def test_fold_grid_runs_the_chain(backend):
    from test_topology import Nx, Ny, _fold_ds, _fold_grid

    grid = _fold_grid(_fold_ds(), "corner")
    t = DataArray(R.synthetic_field((2, Ny, Nx), 91), ("z", "yh", "xh"))
    u = DataArray(R.synthetic_field((2, Ny, Nx), 92), ("z", "yh", "xl"))
    v = DataArray(R.synthetic_field((2, Ny, Nx), 93), ("z", "yl", "xh"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        _same_labelled(grid.flux_divergence(u, v, t, metric_weighted=False),
                       _chain_flux_divergence(grid, u, v, t, metric_weighted=False))
        _same_labelled(grid.laplacian(t, metric_weighted=False), _chain_laplacian(grid, t, metric_weighted=False))


def test_misplaced_inputs_raise(backend):
    grid, ds, dims = _grid((2,), 5, 6, np.float64, {"X": "periodic", "Y": "extend"})
    u, v, t = _fields((2,), 5, 6, np.float64, dims)
    with pytest.raises(NotImplementedError):
        grid.flux_divergence(v, u, t)
    with pytest.raises(NotImplementedError):
        grid.flux_divergence(u, v, u)
    with pytest.raises(NotImplementedError):
        grid.laplacian(u)
    with pytest.raises(NotImplementedError):
        grid.divergence(v, u)  # (the operator the message follows)
