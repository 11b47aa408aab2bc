"""Hydrostatic pressure gradient, `Grid.hydrostatic_pressure_gradient`, on CPU.

The one-pass path runs through the `host_abi` fixture (the product's `xgcm_amd.device` over libxgcm_host.so); the chain it
replaces

    p = grid.cumint(b, Z, to="outer");  pc = grid.interp(p, Z);  gx, gy = grid.gradient(pc, X, Y, metric_weighted=...)

runs through the same Grid over the oracle double, installed AFTER the one-pass calls of a test have run (the double
replaces `asdevice`, which the one-pass entry needs as the product's own).  Values are compared bit for bit (NaN = NaN), with
dims, coords and names.  The fallbacks only call existing device functions and run under the `backend` double.  The
direct-ABI cases (`abi_layout_cases`) are shared with the GPU suite."""

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
ZBCS = ["fill", "extend"]
FILL = {"X": 1.75, "Y": -0.625, "Z": 0.375}
FILLS = [FILL, {"X": -0.0, "Y": float("nan"), "Z": -0.0}, {"X": float("nan"), "Y": -0.0, "Z": float("nan")}]
AXES = {"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"}, "Z": {"center": "ZC", "outer": "ZP1"}}
_same_labelled = TV._same_labelled


def _grid(lead, nz, ny, nx, dtype, padding, weight="drF", planes="plane", axes=AXES, mdtype=None):
    """C-grid with a Z axis that has an outer position.  Z weight: drF(ZC) or a registered (ZC, YC, XC) thickness; dxC / dyC:
    (Y, X) planes or (`lead`) with the first leading dim in front"""
    dims = ("time", "member")[:len(lead)]
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0),
              "YC": ("YC", np.arange(ny) + 0.5), "YG": ("YG", np.arange(ny) * 1.0),
              "ZC": ("ZC", np.arange(nz) + 0.5), "ZP1": ("ZP1", np.arange(nz + 1) * 1.0)}
    for d, n in zip(dims, lead):
        coords[d] = (d, np.arange(n) * 2.0)
    m = lambda shape, seed: R.synthetic_metric(shape, seed).astype(mdtype or dtype)  # noqa: E731
    pl, pd = ((lead[0],), dims[:1]) if planes == "lead" else ((), ())
    data = {"dxC": (pd + ("YC", "XG"), m(pl + (ny, nx), 61)), "dyC": (pd + ("YG", "XC"), m(pl + (ny, nx), 62))}
    if weight == "drF":
        data["drF"] = (("ZC",), m((nz,), 63))
    else:
        data["drF"] = (("ZC", "YC", "XC"), m((nz, ny, nx), 64))
    ds = Dataset(data, coords)
    grid = Grid(ds, coords=axes, metrics={("X",): ["dxC"], ("Y",): ["dyC"], ("Z",): ["drF"]}, padding=padding,
                autoparse_metadata=False)
    return grid, ds, dims


def _field(lead, nz, ny, nx, dtype, dims, nan=False, seed=71):
    b = R.synthetic_field(tuple(lead) + (nz, ny, nx), seed).astype(dtype)
    if nan:
        b.reshape(-1)[3::11] = np.nan
        b[..., :, ny // 2, nx // 2] = np.nan   # a column that is all NaN
        b[..., 0, 0, 0] = np.nan               # a NaN in level 0
        b[..., 0, ny - 1, nx - 1] = np.nan
    return DataArray(b, dims + ("ZC", "YC", "XC"), name="b")


def _chain(grid, b, x_axis="X", y_axis="Y", z_axis="Z", padding=None, fill_value=None, metric_weighted=True):
    kw = dict(padding=padding, fill_value=fill_value)
    p = grid.cumint(b, z_axis, to="outer", **kw)
    pc = grid.interp(p, z_axis, **kw)
    return grid.gradient(pc, x_axis, y_axis, metric_weighted=metric_weighted, **kw)


def _want(b, w, px, py, pz, fill=FILL, mx=None, my=None):
    """the chain over plain numpy arrays (the weight and the metrics broadcast against b)"""
    zax = b.ndim - 3
    p = R.cumsum1d(b, zax, 0, 0, 1, 0, pz, fill["Z"], False, True, w, None)
    pc = R.stencil1d("interp", p, zax, 0, 0, None, 0.0)
    return R.gradient(pc, px, py, fill["X"], fill["Y"], mx, my)


def _compare_with_chain(monkeypatch, cases):
    """cases: (grid, b, kwargs); every one-pass call first, then the chain over the oracle double"""
    from oracle import fake_device

    got = [grid.hydrostatic_pressure_gradient(b, **kw) for grid, b, kw in cases]
    fake_device.install(monkeypatch)
    for (grid, b, kw), g in zip(cases, got):
        want = _chain(grid, b, **kw)
        assert len(g) == 2
        for a, w in zip(g, want):
            _same_labelled(a, w)


# ---- 1. the one-pass result equals the chain ------------------------------------------------------------------------------
@pytest.mark.parametrize("px,py,pz", list(itertools.product(BCS, BCS, ZBCS)))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("weighted", [True, False])
def test_equals_the_chain(host_abi, monkeypatch, px, py, pz, dtype, weighted):
    pad = {"X": px, "Y": py, "Z": pz}
    cases = []
    for n, (lead, nz, ny, nx, weight, planes) in enumerate([((), 4, 5, 8, "drF", "plane"), ((2,), 3, 5, 6, "full", "plane"),
                                                           ((2, 2), 3, 4, 5, "drF", "lead"), ((3,), 5, 3, 12, "full", "lead")]):
        grid, ds, dims = _grid(lead, nz, ny, nx, dtype, pad, weight=weight, planes=planes)
        for nan in (False, True):
            b = _field(lead, nz, ny, nx, dtype, dims, nan=nan)
            cases.append((grid, b, dict(fill_value=FILLS[(n + nan) % 3], metric_weighted=weighted)))
    _compare_with_chain(monkeypatch, cases)


def test_all_nan_column_and_level_zero_nan_stay_finite_where_the_chain_is(host_abi):
    """a NaN product counts as 0: with finite fills the result holds no NaN at all, and equals the numpy chain"""
    grid, ds, dims = _grid((2,), 5, 7, 9, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    b = _field((2,), 5, 7, 9, np.float64, dims, nan=True)
    assert np.isnan(b.values[:, :, 3, 4]).all() and np.isnan(b.values[:, 0, 0, 0]).all()
    gx, gy = grid.hydrostatic_pressure_gradient(b, fill_value=FILL)
    wx, wy = _want(b.values, ds["drF"].values[:, None, None], "periodic", "extend", "fill", mx=ds["dxC"].values,
                   my=ds["dyC"].values)
    assert np.array_equal(gx.values, wx) and np.array_equal(gy.values, wy)
    assert not np.isnan(gx.values).any() and not np.isnan(gy.values).any()


def test_xarray_in_xarray_out(host_abi, monkeypatch):
    import xarray_standin
    from oracle import fake_device

    xarray_standin.install(monkeypatch)
    import xarray as xr

    grid, ds, dims = _grid((), 3, 4, 6, np.float64, {"X": "periodic", "Y": "fill", "Z": "extend"})
    b = _field((), 3, 4, 6, np.float64, dims)
    got = grid.hydrostatic_pressure_gradient(xr.DataArray(b.values, dims=b.dims, name=b.name), fill_value=FILL)
    assert all(type(g).__module__.split(".")[0] == "xarray" for g in got)
    fake_device.install(monkeypatch)
    for g, w in zip(got, _chain(grid, b, fill_value=FILL)):
        assert tuple(g.dims) == tuple(w.dims) and g.name == w.name
        assert np.array_equal(np.asarray(g.values), np.asarray(w.values))


def test_coords_and_names_follow_the_chain(host_abi, monkeypatch):
    cases = []
    for name in ("b", "drF", None):   # (a field named as the weight keeps its name through the product)
        grid, ds, dims = _grid((2,), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
        b = _field((2,), 3, 5, 6, np.float64, dims)._replace(name=name)
        b = b.assign_coords({"lon": (("YC", "XC"), np.ones((5, 6))), "t2": (("time",), np.arange(2) + 7.0),
                             "depth": (("ZC",), np.arange(3) * 10.0), "hFacC": (("ZC", "YC", "XC"), np.ones((3, 5, 6)))})
        cases += [(grid, b, dict(fill_value=FILL, metric_weighted=mw)) for mw in (True, False)]
    _compare_with_chain(monkeypatch, cases)


def test_the_fused_entry_runs_alone(host_abi, monkeypatch):
    """one call of the one-pass device entry and none of the chain's operators"""
    import xgcm_amd.device as D

    grid, ds, dims = _grid((2,), 3, 5, 6, np.float64, {"X": "periodic", "Y": "fill", "Z": "extend"})
    b = _field((2,), 3, 5, 6, np.float64, dims)
    calls = {"fused": 0, "chain": 0}

    def counted(fn, key):
        def wrapped(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(D, "hydrostatic_pressure_gradient", counted(D.hydrostatic_pressure_gradient, "fused"))
    for name in ("gradient", "binary", "stencil1d", "cumsum1d"):
        monkeypatch.setattr(D, name, counted(getattr(D, name), "chain"))
    gx, gy = grid.hydrostatic_pressure_gradient(b, fill_value=FILL)
    wx, wy = _want(b.values, ds["drF"].values[:, None, None], "periodic", "fill", "extend", mx=ds["dxC"].values,
                   my=ds["dyC"].values)
    assert np.array_equal(gx.values, wx) and np.array_equal(gy.values, wy)
    assert gx.dims == ("time", "ZC", "YC", "XG") and gy.dims == ("time", "ZC", "YG", "XC")
    assert calls == {"fused": 1, "chain": 0}


# ---- 2. the smallest shapes at which it can go wrong ----------------------------------------------------------------------
NZS, NYS, NXS = [1, 2, 3, 5], [1, 2, 3, 9], [1, 2, 3, 8, 129, 130, 257]
PADS3 = list(itertools.product(BCS, BCS, ZBCS))


def shape_table(nx):
    """(nz, ny, nx, (px, py, pz), dtype, weight form, metric_weighted): every nz and ny with this nx, the boundaries, the dtype
    and the metric forms rotating so that the table as a whole meets every combination several times"""
    out = []
    for n, (nz, ny) in enumerate(itertools.product(NZS, NYS)):
        k = n + 3 * NXS.index(nx)
        out.append((nz, ny, nx, PADS3[k % len(PADS3)], (np.float64, np.float32)[(k // 2) % 2], ("drF", "full")[k % 2],
                    bool((k // 3) % 2)))
    return out


@pytest.mark.parametrize("nx", NXS)
def test_small_shapes(host_abi, monkeypatch, nx):
    import xgcm_amd.device as D

    calls = []
    real = D.hydrostatic_pressure_gradient
    monkeypatch.setattr(D, "hydrostatic_pressure_gradient", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    cases, single = [], []
    for nz, ny, nx_, (px, py, pz), dtype, weight, mw in shape_table(nx):
        grid, ds, dims = _grid((), nz, ny, nx_, dtype, {"X": px, "Y": py, "Z": pz}, weight=weight)
        b = _field((), nz, ny, nx_, dtype, dims, nan=(nz + ny) % 2 == 0)
        (single if ny * nx_ == 1 else cases).append((grid, b, dict(fill_value=FILL, metric_weighted=mw)))
    _compare_with_chain(monkeypatch, cases)
    assert len(calls) == len(cases) and len(single) == (len(NZS) if nx == 1 else 0)
    # a single column (ny * nx == 1) takes the chain (the oracle double is installed by now) and still agrees
    for grid, b, kw in single:
        for g, w in zip(grid.hydrostatic_pressure_gradient(b, **kw), _chain(grid, b, **kw)):
            _same_labelled(g, w)
    assert len(calls) == len(cases)


# ---- 3. every fallback of the docstring takes the chain -------------------------------------------------------------------
def _no_fused(monkeypatch):
    import xgcm_amd.device as D

    calls = []
    monkeypatch.setattr(D, "hydrostatic_pressure_gradient", lambda *a, **k: calls.append(1) or pytest.fail("one-pass entry called"))
    return calls


def _fallback_equals_chain(grid, b, **kw):
    got, want = grid.hydrostatic_pressure_gradient(b, **kw), _chain(grid, b, **kw)
    for g, w in zip(got, want):
        _same_labelled(g, w)


@pytest.mark.parametrize("dtype", [np.int64, np.int32, np.float16])
def test_integer_and_half_fields_run_the_chain(backend, monkeypatch, dtype):
    _no_fused(monkeypatch)
    grid, ds, dims = _grid((), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    b = DataArray((R.synthetic_field((3, 5, 6), 1) * 100).astype(dtype), ("ZC", "YC", "XC"), name="b")
    for kw in (dict(), dict(metric_weighted=False, fill_value=FILL)):
        _fallback_equals_chain(grid, b, **kw)


def test_float32_field_over_float64_metrics_runs_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, dims = _grid((), 3, 5, 6, np.float32, {"X": "fill", "Y": "periodic", "Z": "extend"}, mdtype=np.float64)
    b = _field((), 3, 5, 6, np.float32, dims)
    for mw in (True, False):
        _fallback_equals_chain(grid, b, fill_value=FILL, metric_weighted=mw)


def test_permuted_dims_run_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, dims = _grid((2,), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    b = _field((2,), 3, 5, 6, np.float64, dims)
    _fallback_equals_chain(grid, b.transpose("ZC", "time", "YC", "XC"), fill_value=FILL)
    _fallback_equals_chain(grid, b.transpose("time", "YC", "ZC", "XC"), fill_value=FILL, metric_weighted=False)


def test_chunked_input_runs_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, dims = _grid((4,), 3, 6, 8, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    b = _field((4,), 3, 6, 8, np.float64, dims)
    cb = DataArray(BlockArray.from_array(b.values, ((2, 2), (3,), (6,), (8,))), b.dims, name="b")
    got = grid.hydrostatic_pressure_gradient(cb, fill_value=FILL)
    want = _chain(grid, cb, fill_value=FILL)
    plain = _want(b.values, ds["drF"].values[:, None, None], "periodic", "extend", "fill", mx=ds["dxC"].values, my=ds["dyC"].values)
    for g, w, pw in zip(got, want, plain):
        assert g.dims == w.dims and g.name == w.name
        assert np.array_equal(np.asarray(g.values), np.asarray(w.values)) and np.array_equal(np.asarray(g.values), pw)


def test_periodic_z_runs_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, dims = _grid((2,), 4, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "periodic"})
    _fallback_equals_chain(grid, _field((2,), 4, 5, 6, np.float64, dims), fill_value=FILL)


def test_missing_z_boundary_raises_the_chains_error(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, dims = _grid((), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    b = _field((), 3, 5, 6, np.float64, dims)
    bare = Grid(ds, coords=AXES, metrics={("X",): ["dxC"], ("Y",): ["dyC"], ("Z",): ["drF"]},
                padding={"X": "periodic", "Y": "extend"}, autoparse_metadata=False)
    with pytest.raises(Exception) as fused_err:
        bare.hydrostatic_pressure_gradient(b)
    with pytest.raises(Exception) as chain_err:
        _chain(bare, b)
    assert type(fused_err.value) is type(chain_err.value) and str(fused_err.value) == str(chain_err.value)


def test_a_weight_with_an_extra_dim_runs_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, dims = _grid((), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    data = {k: (ds[k].dims, ds[k].values) for k in ("dxC", "dyC")}
    data["drF"] = (("ZC", "time"), R.synthetic_metric((3, 2), 65))
    coords = {k: (k, np.asarray(ds.coords[k].values)) for k in ("XC", "XG", "YC", "YG", "ZC", "ZP1")}
    coords["time"] = ("time", np.arange(2) * 2.0)
    ds2 = Dataset(data, coords)
    g2 = Grid(ds2, coords=AXES, metrics={("X",): ["dxC"], ("Y",): ["dyC"], ("Z",): ["drF"]},
              padding={"X": "periodic", "Y": "extend", "Z": "fill"}, autoparse_metadata=False)
    b = _field((), 3, 5, 6, np.float64, ())
    got, want = g2.hydrostatic_pressure_gradient(b, fill_value=FILL), _chain(g2, b, fill_value=FILL)
    for g, w in zip(got, want):
        assert "time" in g.dims
        _same_labelled(g, w)


def test_connected_faces_run_the_chain(backend, monkeypatch):
    from test_topology import COORDS, X_TO_X

    _no_fused(monkeypatch)
    ds = Dataset({"drF": (("zc",), R.synthetic_metric((3,), 63))},
                 coords={"x": np.arange(4), "xl": np.arange(4) - 0.5, "y": np.arange(4), "yl": np.arange(4) - 0.5,
                         "face": np.arange(2), "zc": np.arange(3) + 0.5, "zp1": np.arange(4) * 1.0})
    grid = Grid(ds, coords=dict(COORDS, Z={"center": "zc", "outer": "zp1"}), face_connections=X_TO_X,
                metrics={("Z",): ["drF"]}, padding={"X": "fill", "Y": "extend", "Z": "fill"}, autoparse_metadata=False)
    b = DataArray(R.synthetic_field((2, 3, 4, 4), 82), ("face", "zc", "y", "x"), name="b")
    _fallback_equals_chain(grid, b, metric_weighted=False)


def test_no_outer_position_and_misplaced_fields_raise(backend):
    axes = dict(AXES, Z={"center": "ZC", "left": "ZP1"})
    grid, ds, dims = _grid((), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    b = _field((), 3, 5, 6, np.float64, dims)
    coords = {k: (k, np.asarray(ds.coords[k].values)) for k in ("XC", "XG", "YC", "YG", "ZC")}
    coords["ZP1"] = ("ZP1", np.arange(3) * 1.0)
    left = Grid(Dataset({k: (ds[k].dims, ds[k].values) for k in ("dxC", "dyC", "drF")}, coords), coords=axes,
                metrics={("Z",): ["drF"]}, padding={"X": "periodic", "Y": "extend", "Z": "fill"}, autoparse_metadata=False)
    with pytest.raises(NotImplementedError, match="outer"):
        left.hydrostatic_pressure_gradient(b)
    with pytest.raises(NotImplementedError, match="X:center"):
        grid.hydrostatic_pressure_gradient(DataArray(b.values, ("ZC", "YC", "XG")))
    with pytest.raises(NotImplementedError, match="Z:center"):
        grid.hydrostatic_pressure_gradient(DataArray(np.zeros((4, 5, 6)), ("ZP1", "YC", "XC")))


# ---- 4. physics, at a tolerance ------------------------------------------------------------------------------------------
def test_a_horizontally_uniform_buoyancy_exerts_no_force(host_abi):
    """b constant along X and Y: every column holds the same sums, so both differences are exactly 0 under periodic boundaries"""
    for dtype in (np.float64, np.float32):
        grid, ds, dims = _grid((2,), 6, 5, 8, dtype, {"X": "periodic", "Y": "periodic", "Z": "fill"})
        col = R.synthetic_field((2, 6, 1, 1), 5).astype(dtype)
        b = DataArray(np.ascontiguousarray(np.broadcast_to(col, (2, 6, 5, 8))), dims + ("ZC", "YC", "XC"))
        for mw in (True, False):
            gx, gy = grid.hydrostatic_pressure_gradient(b, fill_value=0.0, metric_weighted=mw)
            assert (gx.values == 0).all() and (gy.values == 0).all()


def test_unit_buoyancy_gives_the_depth_of_the_cell_centre(host_abi):
    """b = i (linear in X, constant along Y and Z), w = drF, Z fill 0: pc[k, j, i] = i * zc[k] with zc the depth of the centre
    of level k, so the plain difference along X is zc[k] from column 1 on.  Bound: pc[k, j, i] carries k + 1 products and
    sums and one mean, each within half an ulp -- a relative error below (k + 3) * eps -- and the difference of two of them
    one rounding more: |gx - zc[k]| <= 2 * (nz + 3) * eps * nx * depth."""
    nz, ny, nx = 9, 4, 12
    grid, ds, dims = _grid((), nz, ny, nx, np.float64, {"X": "extend", "Y": "extend", "Z": "fill"})
    drf = ds["drF"].values
    zc = np.concatenate([[0.0], np.cumsum(drf)[:-1]]) + drf / 2
    b = DataArray(np.ascontiguousarray(np.broadcast_to(np.arange(nx, dtype=np.float64), (nz, ny, nx))), ("ZC", "YC", "XC"))
    gx, gy = grid.hydrostatic_pressure_gradient(b, fill_value=0.0, metric_weighted=False)
    bound = 2 * (nz + 3) * np.finfo(np.float64).eps * nx * drf.sum()
    err = np.abs(gx.values[:, :, 1:] - zc[:, None, None]).max()
    print(f"max |gx - zc| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert (gy.values == 0).all() and (gx.values[:, :, 0] == 0).all()   # extend: pc - pc at row 0 / column 0


# ---- 5. the entry of the C ABI called directly, with views ----------------------------------------------------------------
NVS = {np.float64: 2, np.float32: 4}
SFX = {np.float64: "f64", np.float32: "f32"}
TORCH = {np.float64: torch.float64, np.float32: torch.float32}
ABI_NX = {np.float64: 132, np.float32: 264}   # one full 64-lane tile and a partial one
ABI_PADS = [("periodic", "extend", "fill"), ("fill", "periodic", "extend"), ("extend", "fill", "fill")]


def _abi_call(D, dtype, shape, b, planes, k):
    """one call of xg_hydrostatic_pressure_gradient: `b` a contiguous view, `planes` {w, dxC, dyC} views or None"""
    px, py, pz = ABI_PADS[k]
    args = [b.data_ptr()]
    for name in ("w", "dxC", "dyC"):
        v = planes.get(name)
        if v is None:
            args += [None, None]
        else:
            assert all(m in (1, s) for m, s in zip(v.shape, shape))
            args += [v.data_ptr(), _hip.i64([0 if m == 1 else v.stride(d) for d, m in enumerate(v.shape)])]
    junk = [torch.full(shape, float("nan"), dtype=TORCH[dtype], device=D._MEM.device) for _ in range(2)]
    del junk
    outs = [D._empty(shape, TORCH[dtype], D._MEM.device) for _ in range(2)]
    args += [o.data_ptr() for o in outs] + [_hip.i64(shape), len(shape), _hip.BC[px], FILL["X"], _hip.BC[py], FILL["Y"],
                                             _hip.BC[pz], FILL["Z"]]
    D._check(getattr(D._MEM.lib(), "xg_hydrostatic_pressure_gradient_" + SFX[dtype])(*args, D._stream()))
    return tuple(o.cpu().numpy() for o in outs)


def abi_layout_cases(dtype):
    """Runs the direct-ABI table on whatever library `xgcm_amd.device._MEM` serves.  Every view lives in a NaN-filled
    allocation, so a read outside it shows in the result; the contiguous, aligned control of each set of planes is compared
    with the numpy chain, every other layout with that control."""
    import xgcm_amd.device as D

    nv = NVS[dtype]
    shape = [2, 5, 7, ABI_NX[dtype]]
    lead, nz, ny, nx = shape
    bv = R.synthetic_field(tuple(shape), 101).astype(dtype)
    bv.reshape(-1)[5::17] = np.nan
    vals = {"w": R.synthetic_metric((1, nz, 1, 1), 102).astype(dtype), "w3": R.synthetic_metric((1, nz, ny, nx), 103).astype(dtype),
            "wl": R.synthetic_metric((lead, nz, ny, nx), 106).astype(dtype),
            "dxC": R.synthetic_metric((1, 1, ny, nx), 104).astype(dtype), "dyC": R.synthetic_metric((1, 1, ny, nx), 105).astype(dtype)}
    put = lambda a, st=None, off=ALIGNED: _strided(D, a, st or _contig(a.shape), off)  # noqa: E731
    for k in range(len(ABI_PADS)):
        px, py, pz = ABI_PADS[k]
        b = put(bv)
        assert b.is_contiguous() and b.data_ptr() % 16 == 0
        # each metric alone, all together (the weight in its three forms), none
        for present in (("w",), ("w3",), ("wl",), ("dxC",), ("dyC",), ("w", "dxC", "dyC"), ("w3", "dxC", "dyC"), ()):
            pv = {("w" if n.startswith("w") else n): vals[n] for n in present}
            control = _abi_call(D, dtype, shape, b, {n: put(a) for n, a in pv.items()}, k)
            want = _want(bv, pv.get("w"), px, py, pz, mx=pv.get("dxC"), my=pv.get("dyC"))
            for g, w in zip(control, want):
                assert g.dtype == w.dtype == np.dtype(dtype) and np.array_equal(g, w, equal_nan=True), (k, present)
            views = []
            # a misaligned base: the field one element into its allocation (the narrow form over an even nx)
            off = put(bv, off=1)
            assert off.data_ptr() % 16 == bv.dtype.itemsize
            views.append((off, {n: put(a) for n, a in pv.items()}))
            # the planes one element in; with an odd row pitch; with an odd level pitch (3-D weights)
            views.append((b, {n: put(a, off=1) for n, a in pv.items()}))
            pitched = {}
            for n, a in pv.items():
                s = list(a.shape)
                st = _contig(s[:-1] + [s[-1] + 1]) if s[-1] > 1 else _contig(s)
                pitched[n] = put(a, st)
                assert s[-1] == 1 or (pitched[n].stride(-2) == nx + 1 and pitched[n].stride(-1) == 1)
            views.append((b, pitched))
            if present and present[0] in ("w3", "wl"):
                a = pv["w"]
                st = [(nz * (ny * nx + 1)) * (a.shape[0] > 1), ny * nx + 1, nx, 1]
                lev = put(a, [s or 1 for s in st])
                assert lev.stride(1) == ny * nx + 1
                views.append((b, dict({n: put(x) for n, x in pv.items()}, w=lev)))
            if present and present[0] == "w":
                # the Z-only weight three elements apart
                views.append((b, dict({n: put(x) for n, x in pv.items()}, w=put(pv["w"], [3 * nz, 3, 1, 1], 1))))
            for fb, planes in views:
                got = _abi_call(D, dtype, shape, fb, planes, k)
                for g, c in zip(got, control):
                    assert np.array_equal(g, c, equal_nan=True), (k, present)
        # a stride-0 weight along X and Y: one value per level, expanded over the whole volume, equals the Z-only weight
        flat = put(vals["w"]).expand(1, nz, ny, nx)
        assert flat.stride(-1) == 0 and flat.stride(-2) == 0
        full = put(np.ascontiguousarray(np.broadcast_to(vals["w"], (1, nz, ny, nx))))
        a = _abi_call(D, dtype, shape, b, {"w": flat}, k)
        c = _abi_call(D, dtype, shape, b, {"w": full}, k)
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

    def call(b=t, ndim=3, bcx=_hip.BC["periodic"], bcy=_hip.BC["extend"], bcz=_hip.BC["fill"], w=None, ws=None):
        return lib.xg_hydrostatic_pressure_gradient_f64(b.data_ptr() if b is not None else None, w, ws, None, None, None, None,
                                                        o1.data_ptr(), o2.data_ptr(), _hip.i64(shape), ndim, bcx, 0.0, bcy, 0.0,
                                                        bcz, 0.0, None)

    assert call() == 0
    assert call(b=None) == -1                                  # NULL array: XG_ERR_INVALID
    assert call(bcx=7) == -1 and call(bcz=9) == -1             # unknown boundary codes
    assert call(w=t.data_ptr(), ws=None) == -1                 # a metric without strides
    assert call(ndim=2) < 0 and call(ndim=2) != -1             # XG_ERR_UNSUPPORTED
    assert call(bcz=_hip.BC["periodic"]) < 0 and call(bcz=_hip.BC["periodic"]) != -1
