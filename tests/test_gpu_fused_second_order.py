"""Fused second-order operators on the GPU: `Grid.flux_divergence` / `Grid.laplacian` (one HIP pass, K7d) against the
HIP chains they replace -- flux then divergence; gradient, the two face-length products, then divergence -- bit for bit,
over the CPU suite's matrix, a seeded fuzz of shapes / boundaries / fill values, and BASELINE's full size."""

import numpy as np
import pytest

from oracle import refimpl as R

pytestmark = pytest.mark.gpu

BCS = ["periodic", "extend", "fill"]


def _grid(lead, ny, nx, dtype, padding, met_lead=(), seed=0):
    from xgcm_amd import Dataset, Grid

    dims = ("Z", "face")[:len(lead)]
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0),
              "YC": ("YC", np.arange(ny) + 0.5), "YG": ("YG", np.arange(ny) * 1.0)}
    for d, n in zip(dims, lead):
        coords[d] = (d, np.arange(n) * 2.0)
    mdims = tuple(d for d in dims if d in met_lead)
    mshape = tuple(n for d, n in zip(dims, lead) if d in met_lead) + (ny, nx)
    m = lambda s: R.synthetic_metric(mshape, seed + s).astype(dtype)  # noqa: E731
    ds = Dataset({"dxC": (mdims + ("YC", "XG"), m(61)), "dyG": (mdims + ("YC", "XG"), m(62)),
                  "dyC": (mdims + ("YG", "XC"), m(63)), "dxG": (mdims + ("YG", "XC"), m(64)),
                  "rA": (mdims + ("YC", "XC"), m(65))}, coords)
    grid = Grid(ds, coords={"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"}},
                metrics={("X",): ["dxC", "dxG"], ("Y",): ["dyC", "dyG"], ("X", "Y"): ["rA"]},
                padding=padding, autoparse_metadata=False)
    return grid, dims


def _fields(lead, ny, nx, dtype, dims, hbm, seed=0, nan=False):
    import torch

    from xgcm_amd import DataArray

    shape = tuple(lead) + (ny, nx)
    out = []
    for k, pos in enumerate((("YC", "XG"), ("YG", "XC"), ("YC", "XC"))):
        a = R.synthetic_field(shape, seed + 71 + k).astype(dtype)
        if nan:
            a.reshape(-1)[k::7] = np.nan
        out.append(DataArray(torch.from_numpy(a).cuda() if hbm else a, dims + pos))
    return out


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


def _check(grid, u, v, t, **kw):
    _same(grid.flux_divergence(u, v, t, **kw), _chain_flux_divergence(grid, u, v, t, **kw))
    _same(grid.laplacian(t, **kw), _chain_laplacian(grid, t, **kw))


SHAPES = [((), 6, 8), ((), 7, 5), ((3,), 5, 9), ((2,), 1, 6), ((2,), 6, 1), ((2, 3), 5, 4), ((1,), 1, 1),
          ((2,), 9, 260), ((3,), 13, 129), ((2,), 4, 513)]   # (several wave tiles: lanes 0 / 63 at tile seams)


@pytest.mark.parametrize("px", BCS)
@pytest.mark.parametrize("py", BCS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("weighted", [True, False])
def test_fused_equals_the_hip_chain(px, py, dtype, weighted):
    fill = {"X": 1.75, "Y": -0.625}
    for lead, ny, nx in SHAPES:
        grid, dims = _grid(lead, ny, nx, dtype, {"X": px, "Y": py})
        u, v, t = _fields(lead, ny, nx, dtype, dims, hbm=True)
        _check(grid, u, v, t, fill_value=fill, metric_weighted=weighted)


@pytest.mark.parametrize("met_lead", [(), ("face",), ("Z", "face")])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_4d_with_metrics_broadcast_and_nan(met_lead, dtype):
    for px, py in [("periodic", "fill"), ("extend", "periodic"), ("fill", "extend"), ("periodic", "periodic")]:
        grid, dims = _grid((3, 2), 7, 136, dtype, {"X": px, "Y": py}, met_lead=met_lead)
        u, v, t = _fields((3, 2), 7, 136, dtype, dims, hbm=True, nan=True)
        _check(grid, u, v, t, fill_value={"X": -3.5, "Y": 0.25})


def test_seeded_fuzz():
    """240 seeded cases: shapes (1 - 3 leading dims, odd / even / single extents, several wave tiles), boundary mode and
    fill value per axis, dtype, metric weighting, numpy or HBM residency"""
    rng = np.random.default_rng(20261016)
    for case in range(240):
        nlead = int(rng.integers(0, 3))
        lead = tuple(int(n) for n in rng.integers(1, 4, nlead))
        ny = int(rng.choice([1, 2, 3, 5, 8, 17, 33]))
        nx = int(rng.choice([1, 2, 3, 7, 64, 127, 128, 130, 256, 301]))
        dtype = [np.float64, np.float32][int(rng.integers(0, 2))]
        pad = {"X": BCS[int(rng.integers(0, 3))], "Y": BCS[int(rng.integers(0, 3))]}
        fill = {"X": float(rng.normal()), "Y": float(rng.normal())}
        met_lead = ("Z",) if (nlead and rng.random() < 0.3) else ()
        grid, dims = _grid(lead, ny, nx, dtype, pad, met_lead=met_lead, seed=case)
        u, v, t = _fields(lead, ny, nx, dtype, dims, hbm=bool(rng.random() < 0.7), seed=case, nan=bool(rng.random() < 0.2))
        try:
            _check(grid, u, v, t, fill_value=fill, metric_weighted=bool(rng.random() < 0.7))
        except AssertionError as err:
            raise AssertionError(f"fuzz case {case}: lead {lead} ny {ny} nx {nx} {np.dtype(dtype)} {pad} {fill}") from err


def test_the_fused_path_is_taken(monkeypatch):
    import xgcm_amd.device as D

    grid, dims = _grid((2,), 6, 130, np.float64, {"X": "periodic", "Y": "fill"})
    u, v, t = _fields((2,), 6, 130, np.float64, dims, hbm=True)
    want_fd = _chain_flux_divergence(grid, u, v, t)
    want_lap = _chain_laplacian(grid, t)
    want_plain = _chain_laplacian(grid, t, metric_weighted=False)

    def refuse(*a, **k):
        raise AssertionError("the chain ran")

    for name in ("flux", "gradient", "divergence", "binary"):
        monkeypatch.setattr(D, name, refuse)
    _same(grid.flux_divergence(u, v, t), want_fd)
    _same(grid.laplacian(t), want_lap)
    _same(grid.laplacian(t, metric_weighted=False), want_plain)


def test_residency():
    import torch

    grid, dims = _grid((2,), 5, 8, np.float64, {"X": "extend", "Y": "periodic"})
    for hbm in (False, True):
        u, v, t = _fields((2,), 5, 8, np.float64, dims, hbm=hbm)
        for res in (grid.flux_divergence(u, v, t), grid.laplacian(t)):
            assert isinstance(res.data, torch.Tensor) == hbm
            if hbm:
                assert res.data.is_cuda
            else:
                assert isinstance(res.data, np.ndarray)


@pytest.mark.parametrize("pad", [{"X": "periodic", "Y": "extend"}, {"X": "extend", "Y": "periodic"}])
def test_full_size(pad):
    """BASELINE's 75 x 2400 x 3600 float64: one case per operator and boundary pair, torch.equal with the chain"""
    import torch

    from xgcm_amd import DataArray, Dataset, Grid
    from xgcm_amd import device as D

    nz, ny, nx = 75, 2400, 3600
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0),
              "YC": ("YC", np.arange(ny) + 0.5), "YG": ("YG", np.arange(ny) * 1.0), "Z": ("Z", np.arange(nz) * 1.0)}
    m = lambda s, dims: DataArray(D.synthetic((ny, nx), s, 0, 1.0, 0.5), dims)  # noqa: E731
    ds = Dataset({"dxC": m(61, ("YC", "XG")), "dyG": m(62, ("YC", "XG")), "dyC": m(63, ("YG", "XC")),
                  "dxG": m(64, ("YG", "XC")), "rA": m(65, ("YC", "XC"))}, coords)
    grid = Grid(ds, coords={"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"}},
                metrics={("X",): ["dxC", "dxG"], ("Y",): ["dyC", "dyG"], ("X", "Y"): ["rA"]}, padding=pad,
                autoparse_metadata=False)
    t = DataArray(D.synthetic((nz, ny, nx), 71), ("Z", "YC", "XC"))
    lap = grid.laplacian(t)
    assert torch.equal(lap.data, _chain_laplacian(grid, t).data)
    del lap
    u = DataArray(D.synthetic((nz, ny, nx), 72), ("Z", "YC", "XG"))
    v = DataArray(D.synthetic((nz, ny, nx), 73), ("Z", "YG", "XC"))
    fd = grid.flux_divergence(u, v, t)
    assert torch.equal(fd.data, _chain_flux_divergence(grid, u, v, t).data)
