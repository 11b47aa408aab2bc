"""The vector-invariant harmonic viscosity on the GPU: `Grid.horizontal_viscosity` (K7k), one HIP pass, against the HIP chain
it replaces -- seven launches of the existing operators, nine with the coefficients -- bit for bit, over the CPU suite's
matrix plus shapes that span several wave tiles, NaNs, host inputs, a seeded fuzz and one case under `graphs.capture`.
(The full-size comparison is `tools/bench_configs.py --configs 5hv`.)"""

import itertools

import numpy as np
import pytest

from oracle import refimpl as R

pytestmark = pytest.mark.gpu

BCS = ["periodic", "extend", "fill"]
AXES = {"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"}}
METRICS = {("X",): ["dxC", "dxG"], ("Y",): ["dyC", "dyG"], ("X", "Y"): ["rA", "rAz"]}
FILL = {"X": 1.75, "Y": -0.625}


def _grid(lead, ny, nx, dtype, padding, seed=0):
    from xgcm_amd import Dataset, Grid

    dims = ("time",)[:len(lead)]
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0),
              "YC": ("YC", np.arange(ny) + 0.5), "YG": ("YG", np.arange(ny) * 1.0)}
    for d, n in zip(dims, lead):
        coords[d] = (d, np.arange(n) * 2.0)
    m = lambda k: R.synthetic_metric((ny, nx), seed + k).astype(dtype)  # noqa: E731
    data = {"dxC": (("YC", "XG"), m(61)), "dyC": (("YG", "XC"), m(62)), "rAz": (("YG", "XG"), m(63)), "rA": (("YC", "XC"), m(64)),
            "dyG": (("YC", "XG"), m(65)), "dxG": (("YG", "XC"), m(66)),
            "nu_d": (("YC", "XC"), (R.synthetic_field((ny, nx), seed + 67) * 3.0).astype(dtype)),
            "nu_z": (("YG", "XG"), (R.synthetic_field((ny, nx), seed + 68) * 3.0).astype(dtype))}
    ds = Dataset(data, coords)
    grid = Grid(ds, coords=AXES, metrics=METRICS, padding=padding, autoparse_metadata=False)
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


def _coefficients(form, lead, ny, nx, dtype, dims, ds, hbm, seed=0):
    from xgcm_amd import DataArray

    if form == "none":
        return None, None
    if form == "planes":
        return _resident(ds["nu_d"], hbm), _resident(ds["nu_z"], hbm)
    if form == "rows":
        a, b = ((R.synthetic_field((ny,), seed + k) * 2.0).astype(dtype) for k in (69, 70))
        return _resident(DataArray(a, ("YC",), name="nu_d"), hbm), _resident(DataArray(b, ("YG",), name="nu_z"), hbm)
    assert form == "full"
    shape = tuple(lead) + (ny, nx)
    a, b = ((R.synthetic_field(shape, seed + k) * 2.0).astype(dtype) for k in (76, 77))
    return (_resident(DataArray(a, dims + ("YC", "XC"), name="nu_d"), hbm),
            _resident(DataArray(b, dims + ("YG", "XG"), name="nu_z"), hbm))


def _chain(grid, u, v, viscosity_d=None, viscosity_z=None, padding=None, fill_value=None, metric_weighted=True):
    kw = dict(padding=padding, fill_value=fill_value)
    div = grid.divergence(u, v, "X", "Y", metric_weighted=metric_weighted, **kw)
    zeta = grid.vorticity(u, v, "X", "Y", metric_weighted=metric_weighted, **kw)
    if viscosity_d is not None:
        div = div * viscosity_d
    if viscosity_z is not None:
        zeta = zeta * viscosity_z
    dx, dy = grid.gradient(div, "X", "Y", metric_weighted=metric_weighted, **kw)
    op = grid.derivative if metric_weighted else grid.diff
    zy = op(zeta, "Y", **kw)
    zx = op(zeta, "X", **kw)
    gu = dx - zy
    gv = dy + zx
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


def _check(grid, u, v, nu=(None, None), **kw):
    gu, gv = grid.horizontal_viscosity(u, v, *nu, **kw)
    wu, wv = _chain(grid, u, v, *nu, **kw)
    _same(gu, wu)
    _same(gv, wv)


class _Calls:
    def __init__(self, monkeypatch):
        import xgcm_amd.device as D

        self.n = 0
        fn = D.horizontal_viscosity

        def wrapped(*a, **k):
            self.n += 1
            return fn(*a, **k)

        monkeypatch.setattr(D, "horizontal_viscosity", wrapped)


# the CPU suite's shapes, then several wave tiles and the lane-63 seam for every vector width (a wave covers 64 * V columns,
# V up to 2 in float64 and 4 in float32)
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
        both = _coefficients("planes", lead, ny, nx, dtype, dims, ds, True)
        for weighted, nu in itertools.product((True, False), (both, (None, None))):
            _check(grid, u, v, nu, fill_value=FILL, metric_weighted=weighted)
            n += 1
    assert calls.n == n


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_nans_and_host_inputs(monkeypatch, dtype):
    calls = _Calls(monkeypatch)
    n = 0
    for (px, py), hbm in itertools.product(itertools.product(BCS, BCS), (True, False)):
        grid, ds, dims = _grid((2,), 7, 136, dtype, {"X": px, "Y": py})
        u, v = _fields((2,), 7, 136, dtype, dims, hbm=hbm, nan=7)
        _check(grid, u, v, _coefficients("planes", (2,), 7, 136, dtype, dims, ds, hbm), fill_value={"X": -3.5, "Y": 0.25})
        n += 1
    assert calls.n == n


N_FUZZ = 300


def test_seeded_fuzz(monkeypatch):
    """300 seeded cases over shape, lead dims, dtype, boundaries, fills (-0.0 included), metrics on / off, the coefficients'
    form (none, planes, f(YC) / f(YG) alone, full fields), NaN density, HBM-resident and host inputs; every case is counted
    on the one-pass entry"""
    calls = _Calls(monkeypatch)
    rng = np.random.default_rng(20261018)
    for case in range(N_FUZZ):
        lead = (int(rng.integers(1, 4)),) if rng.random() < 0.3 else ()
        ny = int(rng.choice([1, 2, 3, 5, 8, 17]))
        nx = int(rng.choice([1, 2, 3, 4, 7, 64, 127, 128, 130, 256, 301, 516]))
        dtype = [np.float64, np.float32][int(rng.integers(0, 2))]
        pad = {ax: BCS[int(rng.integers(0, 3))] for ax in ("X", "Y")}
        fill = {ax: [float(rng.normal()), -0.0, 0.0][int(rng.choice([0, 0, 1, 2]))] for ax in ("X", "Y")}
        weighted = bool(rng.random() < 0.6)
        form = ["none", "planes", "rows", "full"][int(rng.integers(0, 4))]
        hbm = bool(rng.random() < 0.7)
        nan = int(rng.choice([0, 0, 3, 7, 31]))
        grid, ds, dims = _grid(lead, ny, nx, dtype, pad, seed=case)
        u, v = _fields(lead, ny, nx, dtype, dims, hbm=hbm, seed=case, nan=nan)
        nu = _coefficients(form, lead, ny, nx, dtype, dims, ds, hbm, seed=case)
        try:
            _check(grid, u, v, nu, fill_value=fill, metric_weighted=weighted)
        except AssertionError as err:
            raise AssertionError(f"fuzz case {case}: lead {lead} {ny}x{nx} {np.dtype(dtype)} {pad} {fill} weighted={weighted} "
                                 f"coefficients={form} hbm={hbm} nan={nan}") from err
    assert calls.n == N_FUZZ


def test_a_negative_zero_fill_on_zero_fields(monkeypatch):
    """all-zero fields of mixed sign under fill_value = -0.0: the sign bits are the chain's"""
    import torch

    from xgcm_amd import DataArray

    calls = _Calls(monkeypatch)
    n = 0
    for (px, py), dtype in itertools.product(itertools.product(BCS, BCS), (np.float64, np.float32)):
        grid, ds, dims = _grid((2,), 5, 130, dtype, {"X": px, "Y": py})
        a = np.zeros((2, 5, 130), dtype=dtype)
        b = np.zeros((2, 5, 130), dtype=dtype)
        a.reshape(-1)[::2] = -0.0
        b.reshape(-1)[1::3] = -0.0
        u = DataArray(torch.from_numpy(a).cuda(), dims + ("YC", "XG"), name="u")
        v = DataArray(torch.from_numpy(b).cuda(), dims + ("YG", "XC"), name="v")
        for weighted in (True, False):
            _check(grid, u, v, fill_value={"X": -0.0, "Y": -0.0}, metric_weighted=weighted)
            n += 1
    assert calls.n == n


def test_the_fused_path_is_taken(monkeypatch):
    import xgcm_amd.device as D

    grid, ds, dims = _grid((2,), 6, 130, np.float64, {"X": "periodic", "Y": "fill"})
    u, v = _fields((2,), 6, 130, np.float64, dims, hbm=True)
    nu = _coefficients("planes", (2,), 6, 130, np.float64, dims, ds, True)
    wants = [_chain(grid, u, v, *nu), _chain(grid, u, v, metric_weighted=False)]
    calls = _Calls(monkeypatch)

    def refuse(*a, **k):
        raise AssertionError("the chain ran")

    for name in ("vorticity", "divergence", "gradient", "binary", "stencil1d"):
        monkeypatch.setattr(D, name, refuse)
    for got, want in zip(grid.horizontal_viscosity(u, v, *nu), wants[0]):
        _same(got, want)
    for got, want in zip(grid.horizontal_viscosity(u, v, metric_weighted=False), wants[1]):
        _same(got, want)
    assert calls.n == 2


def test_under_graph_capture():
    """the operator captured once and replayed on new values in the same storage"""
    import torch

    from xgcm_amd import graphs

    grid, ds, dims = _grid((3,), 40, 256, np.float64, {"X": "periodic", "Y": "extend"})
    u, v = _fields((3,), 40, 256, np.float64, dims, hbm=True)
    nu = _coefficients("planes", (3,), 40, 256, np.float64, dims, ds, True)
    step = graphs.capture(lambda: grid.horizontal_viscosity(u, v, *nu))
    u2, v2 = _fields((3,), 40, 256, np.float64, dims, hbm=True, seed=40)
    u.data.copy_(u2.data)
    v.data.copy_(v2.data)
    gu, gv = step()
    torch.cuda.synchronize()
    got = [x._replace(data=x.data.clone()) for x in (gu, gv)]
    for g, w in zip(got, _chain(grid, u2, v2, *nu)):
        assert torch.equal(g.data, w.data)
