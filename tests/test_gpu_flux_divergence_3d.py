"""Fused 3-D tracer flux divergence on the GPU: `Grid.flux_divergence_3d` (one HIP pass, K7e) against the HIP chain it
replaces -- flux, interp along Z, the product with w, divergence, diff along Z, the sum, the quotient by the volume -- bit
for bit, over the CPU suite's matrix, a seeded fuzz, the full 4320 x 4320 x 90 size and a float32 field of more than 2^31
cells (checked on spot slabs against the oracle)."""

import itertools

import numpy as np
import pytest

from oracle import refimpl as R

pytestmark = pytest.mark.gpu

BCS = ["periodic", "extend", "fill"]
AXES = {"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"}, "Z": {"center": "ZC", "left": "ZL"}}


def _grid(lead, nz, ny, nx, dtype, padding, volume="product", seed=0):
    from xgcm_amd import Dataset, Grid

    dims = ("time",)[:len(lead)]
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0),
              "YC": ("YC", np.arange(ny) + 0.5), "YG": ("YG", np.arange(ny) * 1.0),
              "ZC": ("ZC", -np.arange(nz) - 0.5), "ZL": ("ZL", -np.arange(nz) * 1.0)}
    for d, n in zip(dims, lead):
        coords[d] = (d, np.arange(n) * 2.0)
    data = {"rA": (("YC", "XC"), R.synthetic_metric((ny, nx), seed + 65).astype(dtype)),
            "drF": (("ZC",), R.synthetic_metric((nz,), seed + 66).astype(dtype))}
    metrics = {("X", "Y"): ["rA"], ("Z",): ["drF"]}
    if volume == "registered":
        data["vol"] = (("ZC", "YC", "XC"), R.synthetic_metric((nz, ny, nx), seed + 67).astype(dtype))
        metrics[("X", "Y", "Z")] = ["vol"]
    grid = Grid(Dataset(data, coords), coords=AXES, metrics=metrics, padding=padding, autoparse_metadata=False)
    return grid, dims


def _fields(lead, nz, ny, nx, dtype, dims, hbm, seed=0, nan=False):
    import torch

    from xgcm_amd import DataArray

    shape = tuple(lead) + (nz, ny, nx)
    out = []
    for k, pos in enumerate((("ZC", "YC", "XG"), ("ZC", "YG", "XC"), ("ZL", "YC", "XC"), ("ZC", "YC", "XC"))):
        a = R.synthetic_field(shape, seed + 71 + k).astype(dtype)
        if nan:
            a.reshape(-1)[k::7] = np.nan
        out.append(DataArray(torch.from_numpy(a).cuda() if hbm else a, dims + pos))
    return out


def _chain(grid, u, v, w, t, padding=None, fill_value=None, metric_weighted=True):
    kw = dict(padding=padding, fill_value=fill_value)
    fx, fy = grid.flux(u, v, t, "X", "Y", **kw)
    fz = w * grid.interp(t, "Z", **kw)
    h = grid.divergence(fx, fy, "X", "Y", metric_weighted=False, **kw)
    out = h + grid.diff(fz, "Z", **kw)
    if metric_weighted:
        out = out / grid.get_metric(out, ("X", "Y", "Z"))
    return out


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


def _check(grid, u, v, w, t, **kw):
    _same(grid.flux_divergence_3d(u, v, w, t, **kw), _chain(grid, u, v, w, t, **kw))


SHAPES = [((), 4, 6, 8), ((), 3, 7, 5), ((), 1, 5, 9), ((), 5, 1, 6), ((), 4, 6, 1), ((2,), 3, 5, 4), ((), 1, 1, 1),
          ((2,), 2, 3, 7), ((), 3, 9, 260), ((2,), 2, 13, 129), ((), 2, 4, 513)]   # (several wave tiles: lane 0 / 63 seams)
FILL = {"X": 1.75, "Y": -0.625, "Z": 0.375}


@pytest.mark.parametrize("px,py,pz", list(itertools.product(BCS, BCS, BCS)))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("weighted", [True, False])
def test_fused_equals_the_hip_chain(px, py, pz, dtype, weighted):
    for lead, nz, ny, nx in SHAPES:
        grid, dims = _grid(lead, nz, ny, nx, dtype, {"X": px, "Y": py, "Z": pz})
        u, v, w, t = _fields(lead, nz, ny, nx, dtype, dims, hbm=True)
        _check(grid, u, v, w, t, fill_value=FILL, metric_weighted=weighted)


@pytest.mark.parametrize("volume", ["product", "registered"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_volume_and_nan(volume, dtype):
    for px, py, pz in [("periodic", "fill", "extend"), ("extend", "periodic", "fill"), ("fill", "extend", "periodic")]:
        grid, dims = _grid((2,), 3, 7, 136, dtype, {"X": px, "Y": py, "Z": pz}, volume=volume)
        u, v, w, t = _fields((2,), 3, 7, 136, dtype, dims, hbm=True, nan=True)
        _check(grid, u, v, w, t, fill_value={"X": -3.5, "Y": 0.25, "Z": 2.0})


def test_seeded_fuzz():
    """240 seeded cases: shapes (0 - 1 lead dims, odd / even / single extents, several wave tiles), boundary mode and fill
    value per axis, dtype, volume product or registered, weighting, numpy or HBM residency, NaN cells"""
    rng = np.random.default_rng(20261017)
    for case in range(240):
        lead = (int(rng.integers(1, 3)),) if rng.random() < 0.3 else ()
        nz = int(rng.choice([1, 2, 3, 5, 9]))
        ny = int(rng.choice([1, 2, 3, 5, 8, 17]))
        nx = int(rng.choice([1, 2, 3, 7, 64, 127, 128, 130, 256, 301]))
        dtype = [np.float64, np.float32][int(rng.integers(0, 2))]
        pad = {ax: BCS[int(rng.integers(0, 3))] for ax in ("X", "Y", "Z")}
        fill = {ax: float(rng.normal()) for ax in ("X", "Y", "Z")}
        volume = "registered" if rng.random() < 0.3 else "product"
        grid, dims = _grid(lead, nz, ny, nx, dtype, pad, volume=volume, seed=case)
        u, v, w, t = _fields(lead, nz, ny, nx, dtype, dims, hbm=bool(rng.random() < 0.7), seed=case,
                             nan=bool(rng.random() < 0.2))
        try:
            _check(grid, u, v, w, t, fill_value=fill, metric_weighted=bool(rng.random() < 0.7))
        except AssertionError as err:
            raise AssertionError(f"fuzz case {case}: lead {lead} {nz}x{ny}x{nx} {np.dtype(dtype)} {pad} {fill} {volume}") from err


def test_the_fused_path_is_taken(monkeypatch):
    import xgcm_amd.device as D

    grid, dims = _grid((2,), 4, 6, 130, np.float64, {"X": "periodic", "Y": "fill", "Z": "extend"})
    u, v, w, t = _fields((2,), 4, 6, 130, np.float64, dims, hbm=True)
    want = _chain(grid, u, v, w, t)
    want_plain = _chain(grid, u, v, w, t, metric_weighted=False)
    calls = []
    fused = D.flux_divergence_3d

    def count(*a, **k):
        calls.append(1)
        return fused(*a, **k)

    def refuse(*a, **k):
        raise AssertionError("the chain ran")

    monkeypatch.setattr(D, "flux_divergence_3d", count)
    for name in ("flux", "divergence", "binary", "stencil1d", "flux_divergence"):
        monkeypatch.setattr(D, name, refuse)
    _same(grid.flux_divergence_3d(u, v, w, t), want)
    _same(grid.flux_divergence_3d(u, v, w, t, metric_weighted=False), want_plain)
    assert len(calls) == 2


def test_full_size():
    """BASELINE config 5's 4320 x 4320 x 90 float64, the volume rA * drF: torch.equal with the chain"""
    import torch

    from xgcm_amd import DataArray, Dataset, Grid
    from xgcm_amd import device as D

    nz, ny, nx = 90, 4320, 4320
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0),
              "YC": ("YC", np.arange(ny) + 0.5), "YG": ("YG", np.arange(ny) * 1.0),
              "ZC": ("ZC", np.arange(nz) + 0.5), "ZL": ("ZL", np.arange(nz) * 1.0)}
    ds = Dataset({"rA": DataArray(D.synthetic((ny, nx), 65, 0, 1.0, 0.5), ("YC", "XC")),
                  "drF": DataArray(D.synthetic((nz,), 66, 0, 1.0, 0.5), ("ZC",))}, coords)
    grid = Grid(ds, coords=AXES, metrics={("X", "Y"): ["rA"], ("Z",): ["drF"]},
                padding={"X": "periodic", "Y": "extend", "Z": "fill"}, autoparse_metadata=False)
    t = DataArray(D.synthetic((nz, ny, nx), 71), ("ZC", "YC", "XC"))
    u = DataArray(D.synthetic((nz, ny, nx), 72), ("ZC", "YC", "XG"))
    v = DataArray(D.synthetic((nz, ny, nx), 73), ("ZC", "YG", "XC"))
    w = DataArray(D.synthetic((nz, ny, nx), 74), ("ZL", "YC", "XC"))
    got = grid.flux_divergence_3d(u, v, w, t)
    assert torch.equal(got.data, _chain(grid, u, v, w, t).data)


def test_float32_beyond_2_31_cells_on_spot_slabs():
    """(nz, ny, nx) = (130, 4096, 4096) float32, 2.18e9 cells: levels at the start, the middle, past 2^31 and the last one
    against the oracle, each formed from the slabs around it"""
    import torch

    from xgcm_amd import DataArray, Dataset, Grid
    from xgcm_amd import device as D

    nz, ny, nx = 130, 4096, 4096
    assert nz * ny * nx > 2 ** 31
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0),
              "YC": ("YC", np.arange(ny) + 0.5), "YG": ("YG", np.arange(ny) * 1.0),
              "ZC": ("ZC", np.arange(nz) + 0.5), "ZL": ("ZL", np.arange(nz) * 1.0)}
    grid = Grid(Dataset({}, coords), coords=AXES, padding={"X": "extend", "Y": "periodic", "Z": "extend"},
                autoparse_metadata=False)
    f = lambda seed, dims: DataArray(D.synthetic((nz, ny, nx), seed, dtype=torch.float32), dims)  # noqa: E731
    t, u, v, w = f(81, ("ZC", "YC", "XC")), f(82, ("ZC", "YC", "XG")), f(83, ("ZC", "YG", "XC")), f(84, ("ZL", "YC", "XC"))
    got = grid.flux_divergence_3d(u, v, w, t, metric_weighted=False).data
    for k in (0, 64, 128, nz - 1):
        sl = lambda a, j: a.data[j].cpu().numpy()  # noqa: E731
        tk = sl(t, k)
        fx, fy = R.flux(sl(u, k), sl(v, k), tk, "extend", "periodic")
        h = R.divergence(fx, fy, np.float32(1.0), "extend", "periodic")
        fz = w.data[k].cpu().numpy() * ((sl(t, max(k - 1, 0)) + tk) * np.float32(0.5))
        fz1 = sl(w, k + 1) * ((tk + sl(t, k + 1)) * np.float32(0.5)) if k + 1 < nz else fz
        want = h + (fz1 - fz)
        assert want.dtype == np.float32
        assert np.array_equal(got[k].cpu().numpy(), want, equal_nan=True), f"level {k}"
