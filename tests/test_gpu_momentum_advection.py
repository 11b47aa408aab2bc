"""Kinetic energy and vector-invariant momentum advection on the GPU: `Grid.kinetic_energy` (K7g) and
`Grid.momentum_advection` (K7h), one HIP pass each, against the HIP chains they replace -- six and twenty launches of the
existing operators -- bit for bit, over the CPU suite's matrix plus shapes that span several wave tiles, a seeded fuzz,
the full 4320 x 4320 x 90 size, a float32 field of more than 2^31 cells and one case under `graphs.capture`."""

import itertools

import numpy as np
import pytest

from oracle import refimpl as R

pytestmark = pytest.mark.gpu

BCS = ["periodic", "extend", "fill"]
AXES = {"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"}}
FILL = {"X": 1.75, "Y": -0.625}


def _coords(lead, ny, nx):
    dims = ("time",)[:len(lead)]
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0),
              "YC": ("YC", np.arange(ny) + 0.5), "YG": ("YG", np.arange(ny) * 1.0)}
    for d, n in zip(dims, lead):
        coords[d] = (d, np.arange(n) * 2.0)
    return dims, coords


def _grid(lead, ny, nx, dtype, padding, seed=0):
    from xgcm_amd import Dataset, Grid

    dims, coords = _coords(lead, ny, nx)
    m = lambda k: R.synthetic_metric((ny, nx), seed + k).astype(dtype)  # noqa: E731
    data = {"dxC": (("YC", "XG"), m(61)), "dyC": (("YG", "XC"), m(62)), "rAz": (("YG", "XG"), m(63)),
            "f": (("YG", "XG"), (R.synthetic_field((ny, nx), seed + 65) * 3.0).astype(dtype))}
    ds = Dataset(data, coords)
    grid = Grid(ds, coords=AXES, metrics={("X",): ["dxC"], ("Y",): ["dyC"], ("X", "Y"): ["rAz"]}, padding=padding,
                autoparse_metadata=False)
    return grid, ds, dims


def _fields(lead, ny, nx, dtype, dims, hbm, seed=0, nan=0):
    """`nan`: every nan-th element is a NaN (0: none)"""
    import torch

    from xgcm_amd import DataArray

    shape = tuple(lead) + (ny, nx)
    out = []
    for k, pos in enumerate((("YC", "XG"), ("YG", "XC"))):
        a = R.synthetic_field(shape, seed + 72 + k).astype(dtype)
        if nan:
            a.reshape(-1)[k + 2::nan] = np.nan
        out.append(DataArray(torch.from_numpy(a).cuda() if hbm else a, dims + pos, name="uv"[k]))
    return out


def _resident(da, hbm):
    import torch

    return da._replace(data=torch.from_numpy(np.asarray(da.values)).cuda()) if hbm else da


def _chain_ke(grid, u, v, padding=None, fill_value=None):
    kw = dict(padding=padding, fill_value=fill_value)
    return 0.5 * (grid.interp(u * u, "X", **kw) + grid.interp(v * v, "Y", **kw))


def _chain(grid, u, v, coriolis=None, padding=None, fill_value=None, metric_weighted=True):
    kw = dict(padding=padding, fill_value=fill_value)
    zeta = grid.vorticity(u, v, "X", "Y", metric_weighted=metric_weighted, **kw)
    if coriolis is not None:
        zeta = zeta + coriolis
    ke = 0.5 * (grid.interp(u * u, "X", **kw) + grid.interp(v * v, "Y", **kw))
    vbar = grid.interp(grid.interp(v, "X", **kw), "Y", **kw)
    ubar = grid.interp(grid.interp(u, "Y", **kw), "X", **kw)
    gx, gy = grid.gradient(ke, "X", "Y", metric_weighted=metric_weighted, **kw)
    gu = grid.interp(zeta, "Y", **kw) * vbar - gx
    gv = -(grid.interp(zeta, "X", **kw) * ubar) - gy
    return gu, gv


def _same(got, want):
    import torch

    assert tuple(got.dims) == tuple(want.dims) and got.name == want.name and list(got.coords) == list(want.coords)
    assert type(got.data) is type(want.data)
    if isinstance(want.data, torch.Tensor):
        assert got.data.is_cuda and want.data.is_cuda and got.data.dtype == want.data.dtype
        g, w = got.data, want.data
        # bit patterns, NaN masks apart: -0.0 is not +0.0
        nan = torch.isnan(w)
        assert torch.equal(torch.isnan(g), nan)
        as_int = {4: torch.int32, 8: torch.int64}[g.element_size()]
        zero = torch.zeros((), dtype=g.dtype, device=g.device)
        assert torch.equal(torch.where(nan, zero, g).contiguous().view(as_int), torch.where(nan, zero, w).contiguous().view(as_int))
    else:
        assert got.data.dtype == want.data.dtype and got.data.shape == want.data.shape
        nan = np.isnan(want.data)
        assert np.array_equal(np.isnan(got.data), nan)
        bits, zero = {4: np.uint32, 8: np.uint64}[got.data.dtype.itemsize], got.data.dtype.type(0)
        assert np.array_equal(np.where(nan, zero, got.data).view(bits), np.where(nan, zero, want.data).view(bits))


def _check(grid, u, v, f=None, **kw):
    ke_kw = {k: x for k, x in kw.items() if k != "metric_weighted"}
    _same(grid.kinetic_energy(u, v, **ke_kw), _chain_ke(grid, u, v, **ke_kw))
    gu, gv = grid.momentum_advection(u, v, f, **kw)
    wu, wv = _chain(grid, u, v, f, **kw)
    _same(gu, wu)
    _same(gv, wv)


class _Calls:
    def __init__(self, monkeypatch):
        import xgcm_amd.device as D

        self.n = {"kinetic_energy": 0, "momentum_advection": 0}
        for name in self.n:
            monkeypatch.setattr(D, name, self._counted(getattr(D, name), name))

    def _counted(self, fn, name):
        def wrapped(*a, **k):
            self.n[name] += 1
            return fn(*a, **k)
        return wrapped


# the CPU suite's shapes, then several wave tiles and the lane-63 seam (V = 2: 128 columns per wave, V = 1: 64)
SHAPES = [((), 6, 8), ((), 7, 5), ((), 1, 6), ((), 6, 1), ((2,), 5, 4), ((2,), 3, 7), ((), 4, 3), ((), 1, 1), ((3,), 2, 2),
          ((), 9, 260), ((2,), 13, 129), ((), 4, 513), ((3,), 5, 256), ((), 3, 1024)]


@pytest.mark.parametrize("px,py", list(itertools.product(BCS, BCS)))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fused_equals_the_hip_chain(monkeypatch, px, py, dtype):
    calls = _Calls(monkeypatch)
    n = 0
    for lead, ny, nx in SHAPES:
        grid, ds, dims = _grid(lead, ny, nx, dtype, {"X": px, "Y": py})
        u, v = _fields(lead, ny, nx, dtype, dims, hbm=True)
        f = _resident(ds["f"], True)
        for weighted, cor in itertools.product((True, False), (f, None)):
            _check(grid, u, v, cor, fill_value=FILL, metric_weighted=weighted)
            n += 1
    assert calls.n == {"kinetic_energy": n, "momentum_advection": n}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_nans_and_host_inputs(monkeypatch, dtype):
    calls = _Calls(monkeypatch)
    n = 0
    for (px, py), hbm in itertools.product(itertools.product(BCS, BCS), (True, False)):
        grid, ds, dims = _grid((2,), 7, 136, dtype, {"X": px, "Y": py})
        u, v = _fields((2,), 7, 136, dtype, dims, hbm=hbm, nan=7)
        _check(grid, u, v, _resident(ds["f"], hbm), fill_value={"X": -3.5, "Y": 0.25})
        n += 1
    assert calls.n == {"kinetic_energy": n, "momentum_advection": n}


N_FUZZ = 300


def test_seeded_fuzz(monkeypatch):
    """300 seeded cases over shape, lead dims, dtype, boundaries, fills, metrics on / off, coriolis on / off (as a plane,
    or as f(YG) alone), NaN density, HBM-resident and host inputs; every case is counted on the one-pass entries"""
    calls = _Calls(monkeypatch)
    rng = np.random.default_rng(20261116)
    for case in range(N_FUZZ):
        lead = (int(rng.integers(1, 4)),) if rng.random() < 0.3 else ()
        ny = int(rng.choice([1, 2, 3, 5, 8, 17]))
        nx = int(rng.choice([1, 2, 3, 4, 7, 64, 127, 128, 130, 256, 301, 516]))
        dtype = [np.float64, np.float32][int(rng.integers(0, 2))]
        pad = {ax: BCS[int(rng.integers(0, 3))] for ax in ("X", "Y")}
        fill = {ax: float(rng.normal()) for ax in ("X", "Y")}
        weighted, cor = bool(rng.random() < 0.6), int(rng.integers(0, 3))
        hbm = bool(rng.random() < 0.7)
        nan = int(rng.choice([0, 0, 3, 7, 31]))
        grid, ds, dims = _grid(lead, ny, nx, dtype, pad, seed=case)
        u, v = _fields(lead, ny, nx, dtype, dims, hbm=hbm, seed=case, nan=nan)
        f = None
        if cor == 1:
            f = _resident(ds["f"], hbm)
        elif cor == 2:
            from xgcm_amd import DataArray

            f = _resident(DataArray((R.synthetic_field((ny,), case + 66) * 2.0).astype(dtype), ("YG",)), hbm)
        try:
            _check(grid, u, v, f, fill_value=fill, metric_weighted=weighted)
        except AssertionError as err:
            raise AssertionError(f"fuzz case {case}: lead {lead} {ny}x{nx} {np.dtype(dtype)} {pad} {fill} weighted={weighted} "
                                 f"coriolis={cor} hbm={hbm} nan={nan}") from err
    assert calls.n == {"kinetic_energy": N_FUZZ, "momentum_advection": N_FUZZ}


def test_the_fused_path_is_taken(monkeypatch):
    import xgcm_amd.device as D

    grid, ds, dims = _grid((2,), 6, 130, np.float64, {"X": "periodic", "Y": "fill"})
    u, v = _fields((2,), 6, 130, np.float64, dims, hbm=True)
    f = _resident(ds["f"], True)
    want_ke = _chain_ke(grid, u, v)
    wants = [_chain(grid, u, v, f), _chain(grid, u, v, None, metric_weighted=False)]
    calls = _Calls(monkeypatch)

    def refuse(*a, **k):
        raise AssertionError("the chain ran")

    for name in ("vorticity", "gradient", "binary", "stencil1d"):
        monkeypatch.setattr(D, name, refuse)
    _same(grid.kinetic_energy(u, v), want_ke)
    for got, want in zip(grid.momentum_advection(u, v, f), wants[0]):
        _same(got, want)
    for got, want in zip(grid.momentum_advection(u, v, metric_weighted=False), wants[1]):
        _same(got, want)
    assert calls.n == {"kinetic_energy": 1, "momentum_advection": 2}


def test_under_graph_capture():
    """both operators captured once and replayed on new values in the same storage"""
    import torch

    from xgcm_amd import graphs

    grid, ds, dims = _grid((3,), 40, 256, np.float64, {"X": "periodic", "Y": "extend"})
    u, v = _fields((3,), 40, 256, np.float64, dims, hbm=True)
    f = _resident(ds["f"], True)
    step = graphs.capture(lambda: (grid.kinetic_energy(u, v), grid.momentum_advection(u, v, f)))
    u2, v2 = _fields((3,), 40, 256, np.float64, dims, hbm=True, seed=40)
    u.data.copy_(u2.data)
    v.data.copy_(v2.data)
    ke, (gu, gv) = step()
    torch.cuda.synchronize()
    got = [x._replace(data=x.data.clone()) for x in (ke, gu, gv)]
    wu, wv = _chain(grid, u2, v2, f)
    for g, w in zip(got, (_chain_ke(grid, u2, v2), wu, wv)):
        assert torch.equal(g.data, w.data)


def _big_grid(nz, ny, nx, dtype, padding):
    from xgcm_amd import DataArray, Dataset, Grid
    from xgcm_amd import device as D

    dims, coords = _coords((), ny, nx)
    coords["Z"] = ("Z", np.arange(nz) + 0.5)  # (the fields' leading dim: a label, no grid axis)
    m = lambda seed, d: DataArray(D.synthetic((ny, nx), seed, 0, 1000.0, 1000.0, dtype=dtype), d)  # noqa: E731
    ds = Dataset({"dxC": m(61, ("YC", "XG")), "dyC": m(62, ("YG", "XC")), "rAz": m(63, ("YG", "XG"))}, coords)
    grid = Grid(ds, coords=AXES, metrics={("X",): ["dxC"], ("Y",): ["dyC"], ("X", "Y"): ["rAz"]}, padding=padding,
                autoparse_metadata=False)
    f = DataArray(D.synthetic((ny, nx), 65, 0, 1.0e-4, 0.0, dtype=dtype), ("YG", "XG"))
    return grid, f


def test_full_size():
    """BASELINE config 5's 4320 x 4320 x 90 float64, periodic / extend, metrics and coriolis on: fused against the chain,
    the whole field of both tendencies and of the kinetic energy"""
    import torch

    from xgcm_amd import DataArray
    from xgcm_amd import device as D

    nz, ny, nx = 90, 4320, 4320
    grid, f = _big_grid(nz, ny, nx, torch.float64, {"X": "periodic", "Y": "extend"})
    u = DataArray(D.synthetic((nz, ny, nx), 72), ("Z", "YC", "XG"))
    v = DataArray(D.synthetic((nz, ny, nx), 73), ("Z", "YG", "XC"))
    ke = grid.kinetic_energy(u, v).data
    assert torch.equal(ke, _chain_ke(grid, u, v).data)
    del ke
    gu, gv = (x.data for x in grid.momentum_advection(u, v, f))
    wu, wv = (x.data for x in _chain(grid, u, v, f))
    assert torch.equal(gu, wu) and torch.equal(gv, wv)


def test_float32_beyond_2_31_cells():
    """(nz, ny, nx) = (130, 4096, 4096) float32, 2.18e9 cells: the levels are independent, so the chain runs on slices of
    the first, a middle and the last levels (the last ones lie past 2^31 elements)"""
    import torch

    from xgcm_amd import DataArray
    from xgcm_amd import device as D

    nz, ny, nx = 130, 4096, 4096
    assert nz * ny * nx > 2 ** 31
    grid, f = _big_grid(nz, ny, nx, torch.float32, {"X": "extend", "Y": "periodic"})
    u = DataArray(D.synthetic((nz, ny, nx), 82, dtype=torch.float32), ("Z", "YC", "XG"))
    v = DataArray(D.synthetic((nz, ny, nx), 83, dtype=torch.float32), ("Z", "YG", "XC"))
    ke = grid.kinetic_energy(u, v).data
    gu, gv = (x.data for x in grid.momentum_advection(u, v, f))
    grid2, f2 = _big_grid(2, ny, nx, torch.float32, {"X": "extend", "Y": "periodic"})  # the same metrics over two levels
    assert torch.equal(f2.data, f.data)
    for k0 in (0, 63, 127, nz - 2):
        us = DataArray(u.data[k0:k0 + 2].clone(), u.dims)
        vs = DataArray(v.data[k0:k0 + 2].clone(), v.dims)
        assert torch.equal(ke[k0:k0 + 2], _chain_ke(grid2, us, vs).data), f"levels {k0}, {k0 + 1}"
        wu, wv = _chain(grid2, us, vs, f2)
        assert torch.equal(gu[k0:k0 + 2], wu.data) and torch.equal(gv[k0:k0 + 2], wv.data), f"levels {k0}, {k0 + 1}"
