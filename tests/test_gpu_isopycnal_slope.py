"""The isopycnal slopes on the GPU: `Grid.isopycnal_slope` (K7q, one launch) through libxgcm_hip.so against the numpy statement
of the chain it replaces, both results bit for bit (NaN where the other has NaN, -0.0 is not +0.0); the statement is held to
`Case.not_hollow` before the kernel is asked to match it.  The case builders are those of tests/test_isopycnal_slope.py.  The
entry takes its element type as an argument, so the battery of tests/test_gpu_tunables.py (which looks for `_f64` / `_f32`
entries) does not meet it: the sweep over every value of every launch-shape tunable and the guarded table run here."""

import warnings

import numpy as np
import pytest
import torch

import test_gpu_tunables as TT
import test_isopycnal_slope as TI
import test_richardson_number as TR
from xgcm_amd import DataArray

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nx", TI.NXS)
def test_small_shapes(monkeypatch, nx):
    cases = TI.shape_cases(nx)
    assert len(cases) == len(TI.NZS) * len(TI.NYS)
    TI.compare_with_numpy(cases, monkeypatch)


@pytest.mark.parametrize("pz", TI.BCS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_every_boundary_triple(monkeypatch, pz, dtype):
    cases = [c for px in TI.BCS for py in TI.BCS for c in TI.matrix_cases((px, py, pz), dtype)]
    assert TI.compare_with_numpy(cases, monkeypatch) >= 9


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_metric_forms_and_leading_dims(monkeypatch, dtype):
    assert TI.compare_with_numpy(TI.metric_cases(dtype), monkeypatch) > 5


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("nx", [515, 516])
def test_mid_size(monkeypatch, dtype, nx):
    assert TI.compare_with_numpy(TI.mid_size_cases(dtype, nx), monkeypatch) == 2


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_fills_keep_their_bits(monkeypatch, dtype):
    assert TI.compare_with_numpy(TI.fill_cases(dtype), monkeypatch) == 8


@pytest.mark.parametrize("to", TI.TOS)
def test_a_nan_poisons_exactly_what_the_statement_has_as_nan(to):
    for pads in (("periodic", "periodic", "periodic"), ("extend", "fill", "fill"), ("fill", "extend", "extend")):
        TI.check_nan_locality(to, pads)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_zero_over_zero_lands_where_the_statement_has_it(dtype):
    TI.check_zero_over_zero(dtype)


def test_equals_the_chain_with_its_labels(monkeypatch):
    """the chain itself, through the same library: values, dims, coords and names"""
    calls = TI._counted(monkeypatch, bar_chain=False)
    cases = (TI.matrix_cases(("periodic", "extend", "fill"), np.float64) + TI.matrix_cases(("fill", "periodic", "extend"), np.float32)
             + TI.label_cases()[:8])
    for c in cases:
        for got, want in zip(c.one_pass(), c.chain()):
            TR._same_labelled(got, want)
            TR._same_bits(got.values, want.values)
    assert calls["fused"] == len(cases)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_abi_layouts(dtype):
    TI.abi_layout_cases(dtype)


def test_abi_refuses_bad_calls():
    TI.abi_bad_calls()


def test_seeded_fuzz(monkeypatch):
    """120 cases over the small shapes, the boundary triples, both face positions, the fills, the NaNs, the dtype, the metric
    forms, the leading dims and all-zero fields; one call of the one-pass entry each, so that no case passes by falling back"""
    cases = TI.fuzz_cases()
    assert len(cases) == 120 and TI.compare_with_numpy(cases, monkeypatch) >= 10


def _resident(x):
    return DataArray(torch.from_numpy(x.values).cuda(), x.dims, name=x.name)


def test_hbm_in_hbm_out(monkeypatch):
    calls = TI._counted(monkeypatch)
    c = TI.Case((2,), 5, 9, 136, np.float64, ("periodic", "extend", "fill"), "outer", "full", nan=True)
    got = c.grid.isopycnal_slope(_resident(c.b), **c.kw)
    assert calls == {"fused": 1, "chain": 0}
    for g, want in zip(got, c.want()):
        assert isinstance(g.data, torch.Tensor) and g.data.is_cuda and g.is_device
        assert g.dims == ("time", "ZO", "YC", "XC")
        TR._same_bits(g.data.cpu().numpy(), want)
    for g, ref in zip(got, c.one_pass()):
        assert isinstance(ref.data, np.ndarray)
        TR._same_bits(ref.values, g.data.cpu().numpy())


def test_under_graph_capture(monkeypatch):
    """the operator captured once, on one stream with no parallel branch, and replayed on new values in the same storage; the
    metrics are HBM-resident (the grid uploads them once, in the capture's warm-up)"""
    from xgcm_amd import graphs

    calls = TI._counted(monkeypatch)
    c = TI.Case((2,), 5, 40, 256, np.float64, ("periodic", "extend", "fill"), "outer", "lead")
    c2 = TI.Case((2,), 5, 40, 256, np.float64, c.pads, "outer", "lead", seed=111)
    b, b2 = _resident(c.b), _resident(c2.b)
    step = graphs.capture(lambda: c.grid.isopycnal_slope(b, **c.kw))
    b.data.copy_(b2.data)
    out = step()
    torch.cuda.synchronize()
    assert calls == {"fused": 3, "chain": 0}   # two warm-up runs and the capture itself: the one pass is what the graph holds
    assert c2.not_hollow(*c2.want()) == 1
    for g, w in zip(out, c2.want()):
        got = g.data.clone().cpu().numpy()
        assert got.shape == (2, 6, 40, 256)
        TR._same_bits(got, w)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_every_tunable_value_computes_the_same(dtype):
    """`device.isopycnal_slope` under every value of every tunable of the battery's table, on the battery's own shapes: bit
    for bit what the defaults give, and that is the numpy statement's"""
    from xgcm_amd import _hip
    from xgcm_amd import device as D

    calls, references = TI.tunable_calls(D, dtype)
    run = lambda: {k: [D.tohost(x) for x in fn()] for k, fn in calls.items()}  # noqa: E731
    want = run()
    for k, reference in references.items():
        assert all(TT._same_bits(g, w) for g, w in zip(want[k], reference())), f"{k}: the default result is not numpy's"
    bad = []
    for name, values in TT.ALTERNATIVES.items():
        before = _hip.get_tunable(name)
        try:
            for val in values:
                _hip.set_tunable(name, val)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    got = run()
                bad += [(name, val, k) for k in calls if not all(TT._same_bits(g, w) for g, w in zip(got[k], want[k]))]
        finally:
            _hip.set_tunable(name, before)
    torch.cuda.synchronize()
    assert not bad, bad[:20]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_between_guard_bands_on_the_device(monkeypatch, dtype):
    """the same table with both results and every uploaded input between guard bands, the payload 512-byte aligned, 16 bytes
    and one element off"""
    from xgcm_amd import device as D

    for offset in (0, 16, np.dtype(dtype).itemsize):
        assert TI.guarded_table(D, monkeypatch, dtype, offset, TT._same_bits) == 16
    torch.cuda.synchronize()
