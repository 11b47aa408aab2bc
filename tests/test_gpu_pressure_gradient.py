"""Hydrostatic pressure gradient on the GPU: `Grid.hydrostatic_pressure_gradient` (K7i, one launch) against the chain of three
launches it replaces -- cumint (center -> outer), interp, gradient -- both through libxgcm_hip.so, bit for bit."""

import itertools

import numpy as np
import pytest
import torch

import test_pressure_gradient as TP
from oracle import refimpl as R
from test_richardson_number import _same_bits
from xgcm_amd import DataArray

pytestmark = pytest.mark.gpu


def _same(got, want):
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        TP._same_labelled(g, w)
        _same_bits(np.asarray(g.values), np.asarray(w.values))   # bit patterns, NaN masks apart: -0.0 is not +0.0


def _counted(monkeypatch):
    import xgcm_amd.device as D

    calls = []
    real = D.hydrostatic_pressure_gradient
    monkeypatch.setattr(D, "hydrostatic_pressure_gradient", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize("nx", TP.NXS)
def test_small_shapes(monkeypatch, nx):
    calls = _counted(monkeypatch)
    table = TP.shape_table(nx)
    for nz, ny, nx_, (px, py, pz), dtype, weight, mw in table:
        grid, ds, dims = TP._grid((), nz, ny, nx_, dtype, {"X": px, "Y": py, "Z": pz}, weight=weight)
        b = TP._field((), nz, ny, nx_, dtype, dims, nan=(nz + ny) % 2 == 0)
        kw = dict(fill_value=TP.FILL, metric_weighted=mw)
        _same(grid.hydrostatic_pressure_gradient(b, **kw), TP._chain(grid, b, **kw))
    assert len(calls) == sum(1 for nz, ny, nx_, *_ in table if ny * nx_ != 1)


@pytest.mark.parametrize("px,py", list(itertools.product(TP.BCS, TP.BCS)))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_equals_the_chain(monkeypatch, px, py, dtype):
    calls = _counted(monkeypatch)
    n = 0
    for k, (lead, nz, ny, nx, weight, planes) in enumerate([((), 4, 5, 8, "drF", "plane"), ((2,), 3, 5, 6, "full", "plane"),
                                                           ((2, 2), 3, 4, 5, "drF", "lead"), ((3,), 5, 3, 12, "full", "lead")]):
        pz = TP.ZBCS[(k + TP.BCS.index(px)) % 2]
        grid, ds, dims = TP._grid(lead, nz, ny, nx, dtype, {"X": px, "Y": py, "Z": pz}, weight=weight, planes=planes)
        b = TP._field(lead, nz, ny, nx, dtype, dims, nan=bool(k % 2))
        for mw in (True, False):
            kw = dict(fill_value=TP.FILLS[(k + mw) % 3], metric_weighted=mw)
            _same(grid.hydrostatic_pressure_gradient(b, **kw), TP._chain(grid, b, **kw))
            n += 1
    assert len(calls) == n


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_abi_layouts(dtype):
    TP.abi_layout_cases(dtype)


def test_seeded_fuzz(monkeypatch):
    """240 cases over the small shapes, the boundaries, the fills, the NaN density, the dtype and the metric forms"""
    calls = _counted(monkeypatch)
    rng = np.random.default_rng(20240607)
    expected = 0
    for case in range(240):
        nz, ny, nx = (int(rng.choice(v)) for v in (TP.NZS, TP.NYS, TP.NXS))
        lead = [(), (2,), (2, 2)][int(rng.integers(3))] if nx < 100 else ()
        px, py, pz = rng.choice(TP.BCS), rng.choice(TP.BCS), rng.choice(TP.ZBCS)
        dtype = (np.float64, np.float32)[int(rng.integers(2))]
        weight = ("drF", "full")[int(rng.integers(2))]
        planes = "lead" if lead and rng.integers(2) else "plane"
        grid, ds, dims = TP._grid(lead, nz, ny, nx, dtype, {"X": str(px), "Y": str(py), "Z": str(pz)}, weight=weight, planes=planes)
        bv = R.synthetic_field(tuple(lead) + (nz, ny, nx), 500 + case).astype(dtype)
        density = (0.0, 0.05, 0.5)[int(rng.integers(3))]
        bv[rng.random(bv.shape) < density] = np.nan
        b = DataArray(bv, dims + ("ZC", "YC", "XC"), name="b")
        kw = dict(fill_value=TP.FILLS[int(rng.integers(3))], metric_weighted=bool(rng.integers(2)))
        try:
            _same(grid.hydrostatic_pressure_gradient(b, **kw), TP._chain(grid, b, **kw))
        except AssertionError as err:
            raise AssertionError(f"fuzz case {case}: {lead} {nz}x{ny}x{nx} {px}/{py}/{pz} {np.dtype(dtype)} {weight} {planes} "
                                 f"{kw}") from err
        expected += ny * nx != 1
    assert len(calls) == expected


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("nx", [515, 516])
def test_mid_size(monkeypatch, dtype, nx):
    """several XCD bands, ragged tiles and a ragged last segment together; nx = 515 takes the narrow form, 516 the vector form"""
    calls = _counted(monkeypatch)
    lead, nz, ny = (2,), 7, 67
    grid, ds, dims = TP._grid(lead, nz, ny, nx, dtype, {"X": "periodic", "Y": "periodic", "Z": "extend"})
    b = TP._field(lead, nz, ny, nx, dtype, dims, nan=True)
    _same(grid.hydrostatic_pressure_gradient(b, fill_value=TP.FILL), TP._chain(grid, b, fill_value=TP.FILL))
    assert len(calls) == 1


def test_hbm_in_hbm_out(monkeypatch):
    calls = _counted(monkeypatch)
    grid, ds, dims = TP._grid((2,), 5, 9, 136, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    host = TP._field((2,), 5, 9, 136, np.float64, dims, nan=True)
    b = DataArray(torch.from_numpy(host.values).cuda(), host.dims, name="b")
    got = grid.hydrostatic_pressure_gradient(b, fill_value=TP.FILL)
    assert len(calls) == 1
    want = TP._chain(grid, b, fill_value=TP.FILL)
    ref = grid.hydrostatic_pressure_gradient(host, fill_value=TP.FILL)
    for g, w, r in zip(got, want, ref):
        assert isinstance(g.data, torch.Tensor) and g.data.is_cuda and g.is_device
        assert tuple(g.dims) == tuple(w.dims) and g.name == w.name
        assert torch.equal(g.data.view(torch.int64), w.data.view(torch.int64))
        assert isinstance(r.data, np.ndarray) and np.array_equal(r.values, g.data.cpu().numpy(), equal_nan=True)


def test_under_graph_capture(monkeypatch):
    """the operator captured once and replayed on new values in the same storage; the Z weight, dxC and dyC have the field's
    own shape (2, 5, 40, 256) and are HBM-resident (the grid uploads them once, in the capture's warm-up)"""
    from xgcm_amd import Dataset, Grid, graphs

    calls = _counted(monkeypatch)
    shape = (2, 5, 40, 256)
    lead, nz, ny, nx = shape
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0), "YC": ("YC", np.arange(ny) + 0.5),
              "YG": ("YG", np.arange(ny) * 1.0), "ZC": ("ZC", np.arange(nz) + 0.5), "ZP1": ("ZP1", np.arange(nz + 1) * 1.0),
              "time": ("time", np.arange(lead) * 2.0)}
    ds = Dataset({"drF": (("time", "ZC", "YC", "XC"), R.synthetic_metric(shape, 64)),
                  "dxC": (("time", "ZC", "YC", "XG"), R.synthetic_metric(shape, 61)),
                  "dyC": (("time", "ZC", "YG", "XC"), R.synthetic_metric(shape, 62))}, coords)
    grid = Grid(ds, coords=TP.AXES, metrics={("X",): ["dxC"], ("Y",): ["dyC"], ("Z",): ["drF"]},
                padding={"X": "periodic", "Y": "extend", "Z": "fill"}, autoparse_metadata=False)
    dims = ("time", "ZC", "YC", "XC")
    resident = lambda seed: DataArray(torch.from_numpy(R.synthetic_field(shape, seed)).cuda(), dims, name="b")  # noqa: E731
    b, b2 = resident(71), resident(111)
    step = graphs.capture(lambda: grid.hydrostatic_pressure_gradient(b, fill_value=TP.FILL))
    b.data.copy_(b2.data)
    gx, gy = step()
    torch.cuda.synchronize()
    assert len(calls) == 3   # two warm-up runs and the capture itself: the one-pass entry, not the chain, is in the graph
    got = [x.data.clone() for x in (gx, gy)]
    for g, w in zip(got, TP._chain(grid, b2, fill_value=TP.FILL)):
        assert g.shape == shape and torch.equal(g.view(torch.int64), w.data.view(torch.int64))
