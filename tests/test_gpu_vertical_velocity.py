"""Vertical velocity from continuity on the GPU: `Grid.vertical_velocity` (one HIP pass, K7f) against the HIP chain it
replaces -- the products with the face areas, divergence, cumsum along Z, the negation, the quotient by the area -- bit for
bit, over the CPU suite's matrix, a seeded fuzz, the full 4320 x 4320 x 90 size and a float32 field of more than 2^31 cells
(spot columns against numpy's nancumsum of the chain's divergence)."""

import itertools

import numpy as np
import pytest

from oracle import refimpl as R

pytestmark = pytest.mark.gpu

BCS = ["periodic", "extend", "fill"]
ZBCS = ["fill", "extend"]
AXES = {"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"}, "Z": {"center": "ZC", "left": "ZL"}}
FILL = {"X": 1.75, "Y": -0.625, "Z": 0.375}


def _grid(lead, nz, ny, nx, dtype, padding, faces="factors", area="plane", seed=0):
    from xgcm_amd import Dataset, Grid

    dims = ("time",)[:len(lead)]
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0),
              "YC": ("YC", np.arange(ny) + 0.5), "YG": ("YG", np.arange(ny) * 1.0),
              "ZC": ("ZC", -np.arange(nz) - 0.5), "ZL": ("ZL", -np.arange(nz) * 1.0)}
    for d, n in zip(dims, lead):
        coords[d] = (d, np.arange(n) * 2.0)
    m = lambda shape, k: R.synthetic_metric(shape, seed + k).astype(dtype)  # noqa: E731
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
    grid = Grid(Dataset(data, coords), coords=AXES, metrics=metrics, padding=padding, autoparse_metadata=False)
    return grid, dims


def _fields(lead, nz, ny, nx, dtype, dims, hbm, seed=0, nan=False):
    import torch

    from xgcm_amd import DataArray

    shape = tuple(lead) + (nz, ny, nx)
    out = []
    for k, pos in enumerate((("ZC", "YC", "XG"), ("ZC", "YG", "XC"))):
        a = R.synthetic_field(shape, seed + 72 + k).astype(dtype)
        if nan:
            a.reshape(-1)[k + 2::7] = np.nan
        out.append(DataArray(torch.from_numpy(a).cuda() if hbm else a, dims + pos, name="uv"[k]))
    return out


def _chain(grid, u, v, padding=None, fill_value=None, reverse=False, face_weighted=False, metric_weighted=True):
    kw = dict(padding=padding, fill_value=fill_value)
    if face_weighted:
        u = u * grid.get_metric(u, ("Y", "Z"))
        v = v * grid.get_metric(v, ("X", "Z"))
    d = grid.divergence(u, v, "X", "Y", metric_weighted=False, **kw)
    w = -grid.cumsum(d, "Z", to="left", reverse=reverse, **kw)
    if metric_weighted:
        w = w / grid.get_metric(w, ("X", "Y"))
    return w


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


def _check(grid, u, v, **kw):
    try:
        want = _chain(grid, u, v, **kw)
    except ValueError as err:  # one level summed upward with `extend`: the chain refuses, and so must the operator
        assert "extend empty axis" in str(err)
        with pytest.raises(ValueError, match="extend empty axis"):
            grid.vertical_velocity(u, v, **kw)
        return
    _same(grid.vertical_velocity(u, v, **kw), want)


SHAPES = [((), 4, 6, 8), ((), 3, 7, 5), ((), 5, 1, 6), ((), 4, 6, 1), ((2,), 3, 5, 4), ((2,), 2, 3, 7), ((), 7, 4, 3),
          ((), 1, 5, 9), ((), 9, 9, 260), ((2,), 8, 13, 129), ((), 12, 4, 513)]   # (several wave tiles: the lane 63 seam)


@pytest.mark.parametrize("px,py,pz,rev", list(itertools.product(BCS, BCS, ZBCS, [False, True])))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fused_equals_the_hip_chain(px, py, pz, rev, dtype):
    for lead, nz, ny, nx in SHAPES:
        grid, dims = _grid(lead, nz, ny, nx, dtype, {"X": px, "Y": py, "Z": pz})
        u, v = _fields(lead, nz, ny, nx, dtype, dims, hbm=True)
        _check(grid, u, v, fill_value=FILL, reverse=rev)
        _check(grid, u, v, fill_value=FILL, reverse=rev, metric_weighted=False)


@pytest.mark.parametrize("faces", ["factors", "registered"])
@pytest.mark.parametrize("area", ["plane", "full"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_face_weights_area_forms_and_nan(faces, area, dtype):
    for px, py, pz, rev in [("periodic", "fill", "extend", False), ("extend", "periodic", "fill", True),
                            ("fill", "extend", "fill", False), ("periodic", "periodic", "extend", True)]:
        grid, dims = _grid((2,), 7, 7, 136, dtype, {"X": px, "Y": py, "Z": pz}, faces=faces, area=area)
        u, v = _fields((2,), 7, 7, 136, dtype, dims, hbm=True, nan=True)
        _check(grid, u, v, fill_value={"X": -3.5, "Y": 0.25, "Z": 2.0}, reverse=rev, face_weighted=True)


def _fuzz_case(rng, case):
    lead = (int(rng.integers(1, 3)),) if rng.random() < 0.3 else ()
    nz = int(rng.choice([1, 2, 3, 5, 9, 14]))
    ny = int(rng.choice([1, 2, 3, 5, 8, 17]))
    nx = int(rng.choice([1, 2, 3, 7, 64, 127, 128, 130, 256, 301]))
    dtype = [np.float64, np.float32][int(rng.integers(0, 2))]
    pad = {ax: BCS[int(rng.integers(0, 3))] for ax in ("X", "Y")}
    pad["Z"] = str(rng.choice(["fill", "extend", "periodic"], p=[0.45, 0.4, 0.15]))  # periodic Z, forward: the chain itself
    fill = {ax: float(rng.normal()) for ax in ("X", "Y", "Z")}
    kw = dict(reverse=bool(rng.random() < 0.5), face_weighted=bool(rng.random() < 0.5), metric_weighted=bool(rng.random() < 0.7))
    faces = "registered" if rng.random() < 0.4 else "factors"
    area = "full" if rng.random() < 0.4 else "plane"
    hbm, nan = bool(rng.random() < 0.7), bool(rng.random() < 0.3)
    return lead, nz, ny, nx, dtype, pad, fill, kw, faces, area, hbm, nan


N_FUZZ = 240


def test_seeded_fuzz(monkeypatch):
    """240 seeded cases: shape, lead dims, dtype, paddings, fills, `reverse`, the two weighting flags, the metric forms, numpy
    or HBM residency and planted NaNs.  No case is skipped; the cases that route to the chain by design (summed forward with
    periodic Z, drawn with probability 0.15 * 0.5, or with one level and `extend`, 1/6 * 0.4 * 0.5, where the chain raises, or a single column, 1/60) are
    counted and are at most a quarter; every other case is counted on the one-pass entry."""
    import xgcm_amd.device as D

    fused_calls = []
    fused = D.vertical_velocity

    def count(*a, **k):
        fused_calls.append(1)
        return fused(*a, **k)

    monkeypatch.setattr(D, "vertical_velocity", count)
    rng = np.random.default_rng(20261101)
    chained = 0
    for case in range(N_FUZZ):
        lead, nz, ny, nx, dtype, pad, fill, kw, faces, area, hbm, nan = _fuzz_case(rng, case)
        grid, dims = _grid(lead, nz, ny, nx, dtype, pad, faces=faces, area=area, seed=case)
        u, v = _fields(lead, nz, ny, nx, dtype, dims, hbm=hbm, seed=case, nan=nan)
        to_chain = (not kw["reverse"] and (pad["Z"] == "periodic" or (pad["Z"] == "extend" and nz == 1))) or ny * nx == 1
        chained += to_chain
        before = len(fused_calls)
        try:
            _check(grid, u, v, fill_value=fill, **kw)
        except AssertionError as err:
            raise AssertionError(f"fuzz case {case}: lead {lead} {nz}x{ny}x{nx} {np.dtype(dtype)} {pad} {fill} {kw} {faces} "
                                 f"{area}") from err
        assert len(fused_calls) - before == (0 if to_chain else 1), f"fuzz case {case}: wrong route"
    assert chained * 4 <= N_FUZZ, f"{chained} of {N_FUZZ} cases ran the chain"
    assert len(fused_calls) == N_FUZZ - chained


def test_the_fused_path_is_taken(monkeypatch):
    import xgcm_amd.device as D

    grid, dims = _grid((2,), 4, 6, 130, np.float64, {"X": "periodic", "Y": "fill", "Z": "extend"})
    u, v = _fields((2,), 4, 6, 130, np.float64, dims, hbm=True)
    wants = [_chain(grid, u, v, **kw) for kw in (dict(), dict(metric_weighted=False), dict(reverse=True, face_weighted=True))]
    calls = []
    fused = D.vertical_velocity

    def count(*a, **k):
        calls.append(1)
        return fused(*a, **k)

    def refuse(*a, **k):
        raise AssertionError("the chain ran")

    monkeypatch.setattr(D, "vertical_velocity", count)
    for name in ("divergence", "binary", "stencil1d", "cumsum1d"):
        monkeypatch.setattr(D, name, refuse)
    _same(grid.vertical_velocity(u, v), wants[0])
    _same(grid.vertical_velocity(u, v, metric_weighted=False), wants[1])
    _same(grid.vertical_velocity(u, v, reverse=True, face_weighted=True), wants[2])
    assert len(calls) == 3


def test_full_size():
    """BASELINE config 5's 4320 x 4320 x 90 float64, transports in, the area rA: fused against the chain on spot slabs (the
    first, a middle and the last level), forward and reverse"""
    import torch

    from xgcm_amd import DataArray, Dataset, Grid
    from xgcm_amd import device as D

    nz, ny, nx = 90, 4320, 4320
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0),
              "YC": ("YC", np.arange(ny) + 0.5), "YG": ("YG", np.arange(ny) * 1.0),
              "ZC": ("ZC", np.arange(nz) + 0.5), "ZL": ("ZL", np.arange(nz) * 1.0)}
    ds = Dataset({"rA": DataArray(D.synthetic((ny, nx), 65, 0, 1.0, 0.5), ("YC", "XC"))}, coords)
    grid = Grid(ds, coords=AXES, metrics={("X", "Y"): ["rA"]},
                padding={"X": "periodic", "Y": "extend", "Z": "fill"}, autoparse_metadata=False)
    u = DataArray(D.synthetic((nz, ny, nx), 72), ("ZC", "YC", "XG"))
    v = DataArray(D.synthetic((nz, ny, nx), 73), ("ZC", "YG", "XC"))
    for rev in (False, True):
        got = grid.vertical_velocity(u, v, reverse=rev).data
        slabs = {k: got[k].clone() for k in (0, 1, nz // 2, nz - 1)}
        del got
        want = _chain(grid, u, v, reverse=rev).data
        for k, slab in slabs.items():
            assert torch.equal(slab, want[k]), f"reverse={rev}, level {k}"
        del want


def test_float32_beyond_2_31_cells_on_spot_columns():
    """(nz, ny, nx) = (130, 4096, 4096) float32, 2.18e9 cells: columns of the first, a middle and the last rows (levels up to
    the last one lie past 2^31 elements) against numpy's nancumsum of the chain's divergence, added in sequence"""
    import torch

    from xgcm_amd import DataArray, Dataset, Grid
    from xgcm_amd import device as D

    nz, ny, nx = 130, 4096, 4096
    assert nz * ny * nx > 2 ** 31
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0),
              "YC": ("YC", np.arange(ny) + 0.5), "YG": ("YG", np.arange(ny) * 1.0),
              "ZC": ("ZC", np.arange(nz) + 0.5), "ZL": ("ZL", np.arange(nz) * 1.0)}
    grid = Grid(Dataset({}, coords), coords=AXES, padding={"X": "extend", "Y": "periodic", "Z": "fill"},
                autoparse_metadata=False)
    f = lambda seed, dims: DataArray(D.synthetic((nz, ny, nx), seed, dtype=torch.float32), dims)  # noqa: E731
    u, v = f(82, ("ZC", "YC", "XG")), f(83, ("ZC", "YG", "XC"))
    d = grid.divergence(u, v, metric_weighted=False).data
    rows = (0, 1, 2047, ny - 1)
    dcols = {j: d[:, j, :].cpu().numpy() for j in rows}   # (nz, nx) columns of the chain's divergence
    del d
    for rev in (False, True):
        got = grid.vertical_velocity(u, v, fill_value={"Z": 0.5}, reverse=rev, metric_weighted=False).data
        for j in rows:
            dj = dcols[j]
            assert dj.dtype == np.float32
            if rev:
                want = -np.flip(np.nancumsum(np.flip(dj, 0), axis=0, dtype=np.float32), 0)
            else:
                want = -np.concatenate([np.full((1, nx), 0.5, np.float32), np.nancumsum(dj, axis=0, dtype=np.float32)[:-1]])
            assert want.dtype == np.float32
            assert np.array_equal(got[:, j, :].cpu().numpy(), want), f"reverse={rev}, row {j}"
        del got
