"""Vertical advection of horizontal momentum on the GPU: `Grid.vertical_momentum_advection` (K7j, one launch) against the chain
of twelve launches it replaces -- two interps of w, two diffs along Z, two products, two interps along Z, two negations, two
divisions -- both through libxgcm_hip.so, bit for bit."""

import itertools

import numpy as np
import pytest
import torch

import test_vertical_momentum_advection as TM
from oracle import refimpl as R
from xgcm_amd import DataArray

pytestmark = pytest.mark.gpu


def _same(got, want):
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        TM._same_labelled(g, w)
        TM._same_bits(np.asarray(g.values), np.asarray(w.values))   # bit patterns, NaN masks apart: -0.0 is not +0.0


def _counted(monkeypatch):
    import xgcm_amd.device as D

    calls = []
    real = D.vertical_momentum_advection
    monkeypatch.setattr(D, "vertical_momentum_advection", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize("nx", TM.NXS)
def test_small_shapes(monkeypatch, nx):
    calls = _counted(monkeypatch)
    table = TM.shape_table(nx)
    for nz, ny, nx_, (px, py, pz), dtype, metric, mw in table:
        grid, ds, dims = TM._grid((), nz, ny, nx_, dtype, {"X": px, "Y": py, "Z": pz}, metric=metric)
        f = TM._fields((), nz, ny, nx_, dtype, dims, nan=(nz + ny) % 2 == 0)
        kw = dict(fill_value=TM.FILL, metric_weighted=mw)
        _same(grid.vertical_momentum_advection(*f, **kw), TM._chain(grid, *f, **kw))
    assert len(calls) == len(table)


@pytest.mark.parametrize("px,py,pz", list(itertools.product(TM.BCS, TM.BCS, TM.BCS)))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_equals_the_chain(monkeypatch, px, py, pz, dtype):
    calls = _counted(monkeypatch)
    n = 0
    for k, (lead, nz, ny, nx, metric) in enumerate(TM.LEAD_CASES):
        grid, ds, dims = TM._grid(lead, nz, ny, nx, dtype, {"X": px, "Y": py, "Z": pz}, metric=metric)
        f = TM._fields(lead, nz, ny, nx, dtype, dims, nan=bool(k % 2))
        for mw in (True, False):
            kw = dict(fill_value=TM.FILLS[(k + mw) % 3], metric_weighted=mw)
            _same(grid.vertical_momentum_advection(*f, **kw), TM._chain(grid, *f, **kw))
            n += 1
    assert len(calls) == n


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_signed_zeros_and_negative_zero_fills_keep_their_sign(monkeypatch, dtype):
    """bit patterns, not values: -0.0 fills and exact zeros of both signs, kernel against chain against numpy"""
    calls = _counted(monkeypatch)
    cases = TM.signed_zero_cases(dtype)
    for grid, f, kw, (px, py, pz) in cases:
        got, want = grid.vertical_momentum_advection(*f, **kw), TM._chain(grid, *f, **kw)
        fill = kw["fill_value"] or {"X": 0.0, "Y": 0.0, "Z": 0.0}
        m = np.asarray(grid._ds["drF"].values)[:, None, None] if kw["metric_weighted"] else None
        plain = TM._want(*(a.values for a in f), px, py, pz, fill=fill, mu=m, mv=m)
        for g, w, pw in zip(got, want, plain):
            TM._same_bits(g.values, w.values)
            TM._same_bits(g.values, pw)
    assert len(calls) == len(cases)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_abi_layouts(dtype):
    TM.abi_layout_cases(dtype)


def test_seeded_fuzz(monkeypatch):
    """240 cases over the small shapes, all 27 boundary triples, the fills, the NaN density, the dtype and the metric forms"""
    calls = _counted(monkeypatch)
    rng = np.random.default_rng(20240611)
    for case in range(240):
        nz, ny, nx = (int(rng.choice(v)) for v in (TM.NZS, TM.NYS, TM.NXS))
        lead = [(), (2,), (2, 2)][int(rng.integers(3))] if nx < 100 else ()
        px, py, pz = TM.PADS3[case % 27] if case < 27 else (str(rng.choice(TM.BCS)) for _ in range(3))
        dtype = (np.float64, np.float32)[int(rng.integers(2))]
        metric = ("drF", "full", "lead")[int(rng.integers(3 if lead else 2))]
        grid, ds, dims = TM._grid(lead, nz, ny, nx, dtype, {"X": px, "Y": py, "Z": pz}, metric=metric)
        density = (0.0, 0.05, 0.5)[int(rng.integers(3))]
        f = []
        for n, (name, fd) in enumerate((("u", ("ZC", "YC", "XG")), ("v", ("ZC", "YG", "XC")), ("w", ("ZL", "YC", "XC")))):
            a = R.synthetic_field(tuple(lead) + (nz, ny, nx), 500 + 3 * case + n).astype(dtype)
            a[rng.random(a.shape) < density] = np.nan
            f.append(DataArray(a, dims + fd, name=name))
        kw = dict(fill_value=TM.FILLS[int(rng.integers(3))], metric_weighted=bool(rng.integers(2)))
        try:
            _same(grid.vertical_momentum_advection(*f, **kw), TM._chain(grid, *f, **kw))
        except AssertionError as err:
            raise AssertionError(f"fuzz case {case}: {lead} {nz}x{ny}x{nx} {px}/{py}/{pz} {np.dtype(dtype)} {metric} "
                                 f"NaN density {density} {kw}") from err
    assert len(calls) == 240


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("nx", [515, 516])
def test_mid_size(monkeypatch, dtype, nx):
    """several XCD bands, ragged tiles and a ragged last segment together; nx = 515 takes the narrow form, 516 the vector form"""
    calls = _counted(monkeypatch)
    lead, nz, ny = (2,), 7, 67
    for pz, metric in (("periodic", "full"), ("fill", "drF")):
        grid, ds, dims = TM._grid(lead, nz, ny, nx, dtype, {"X": "periodic", "Y": "periodic", "Z": pz}, metric=metric)
        f = TM._fields(lead, nz, ny, nx, dtype, dims, nan=True)
        _same(grid.vertical_momentum_advection(*f, fill_value=TM.FILL), TM._chain(grid, *f, fill_value=TM.FILL))
    assert len(calls) == 2


def test_hbm_in_hbm_out(monkeypatch):
    calls = _counted(monkeypatch)
    grid, ds, dims = TM._grid((2,), 5, 9, 136, np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"})
    host = TM._fields((2,), 5, 9, 136, np.float64, dims, nan=True)
    f = tuple(DataArray(torch.from_numpy(a.values).cuda(), a.dims, name=a.name) for a in host)
    got = grid.vertical_momentum_advection(*f, fill_value=TM.FILL)
    assert len(calls) == 1
    want = TM._chain(grid, *f, fill_value=TM.FILL)
    ref = grid.vertical_momentum_advection(*host, fill_value=TM.FILL)
    for g, w, r in zip(got, want, ref):
        assert isinstance(g.data, torch.Tensor) and g.data.is_cuda and g.is_device
        assert tuple(g.dims) == tuple(w.dims) and g.name == w.name
        assert isinstance(w.data, torch.Tensor) and w.data.is_cuda
        assert np.array_equal(g.data.cpu().numpy(), w.data.cpu().numpy(), equal_nan=True)
        assert isinstance(r.data, np.ndarray) and np.array_equal(r.values, g.data.cpu().numpy(), equal_nan=True)


def test_under_graph_capture(monkeypatch):
    """the operator captured once and replayed on new values in the same storage; the two Z metrics have the fields' own shape
    (2, 5, 40, 256) and are HBM-resident (the grid uploads them once, in the capture's warm-up)"""
    from xgcm_amd import graphs

    calls = _counted(monkeypatch)
    shape = (2, 5, 40, 256)
    grid, ds, dims = TM._grid(shape[:1], *shape[1:], np.float64, {"X": "periodic", "Y": "extend", "Z": "fill"}, metric="lead")
    assert ds["hFacW"].shape == shape and ds["hFacS"].shape == shape

    def resident(seed):
        return tuple(DataArray(torch.from_numpy(a.values).cuda(), a.dims, name=a.name)
                     for a in TM._fields(shape[:1], *shape[1:], np.float64, dims, seed=seed))

    f, f2 = resident(71), resident(111)
    step = graphs.capture(lambda: grid.vertical_momentum_advection(*f, fill_value=TM.FILL))
    for a, a2 in zip(f, f2):
        a.data.copy_(a2.data)
    gu, gv = step()
    torch.cuda.synchronize()
    assert len(calls) == 3   # two warm-up runs and the capture itself: the one-pass entry, not the chain, is in the graph
    got = [x.data.clone() for x in (gu, gv)]
    for g, w in zip(got, TM._chain(grid, *f2, fill_value=TM.FILL)):
        assert g.shape == shape and torch.equal(g.view(torch.int64), w.data.view(torch.int64))
