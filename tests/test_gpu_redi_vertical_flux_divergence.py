"""The divergence of the off-diagonal vertical isoneutral flux on the GPU: `Grid.redi_vertical_flux_divergence` (K7s, one
launch) through libxgcm_hip.so against the numpy statement of the chain it replaces, bit for bit (NaN where the other has NaN,
-0.0 is not +0.0); the statement is held to its own conditions (every ordinary case finite, at least half of every table's
cells non-zero) before the kernel is asked to match it.  The case builders are those of
tests/test_redi_vertical_flux_divergence.py, every table with both values of `closed`.  The entry takes its element type as
an argument, so the battery of tests/test_gpu_tunables.py (which looks for `_f64` / `_f32` entries) does not meet it: the
sweep over every value of every launch-shape tunable and the guarded table run here."""

import warnings

import numpy as np
import pytest
import torch

import test_gpu_tunables as TT
import test_isopycnal_slope as TI
import test_redi_vertical_flux_divergence as TF
import test_richardson_number as TR
from xgcm_amd import DataArray

pytestmark = pytest.mark.gpu


def test_small_shapes(monkeypatch):
    cases = [c for nx in TI.NXS for c in TF.shape_cases(nx)]
    assert len(cases) == 2 * len(TI.NZS) * len(TI.NYS) * len(TI.NXS)
    TF.compare_with_numpy(cases, monkeypatch)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_one_level(monkeypatch, dtype):
    TF.compare_with_numpy(TF.one_level_cases(dtype), monkeypatch)


@pytest.mark.parametrize("pz", TI.BCS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_every_boundary_triple(monkeypatch, pz, dtype):
    cases = [c for px in TI.BCS for py in TI.BCS for c in TF.matrix_cases((px, py, pz), dtype)]
    assert TF.compare_with_numpy(cases, monkeypatch) >= 18


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_metric_forms_and_leading_dims(monkeypatch, dtype):
    assert TF.compare_with_numpy(TF.metric_cases(dtype), monkeypatch) > 10
    TF.check_each_metric_absent_on_its_own(dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("nx", [515, 516])
def test_mid_size(monkeypatch, dtype, nx):
    assert TF.compare_with_numpy(TF.mid_size_cases(dtype, nx), monkeypatch) == 4


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_fills_keep_their_bits(monkeypatch, dtype):
    assert TF.compare_with_numpy(TF.fill_cases(dtype), monkeypatch) == 16


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_closed_really_is_closed(dtype):
    TF.check_closed_is_closed(dtype)


@pytest.mark.parametrize("closed", [True, False])
@pytest.mark.parametrize("to", TI.TOS)
def test_a_nan_poisons_exactly_what_the_statement_has_as_nan(to, closed):
    for pads in (("periodic", "periodic", "periodic"), ("extend", "fill", "fill"), ("fill", "extend", "extend")):
        TF.check_nan_locality(to, pads, closed)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_on_redi_tensors_own_results(monkeypatch, dtype):
    calls = TF._counted(monkeypatch)
    TF.check_on_redi_tensors_own_results(dtype)
    assert calls == {"fused": 2, "chain": 0}


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_the_flux_of_b_itself_cancels_against_kwz_bz(dtype):
    TF.check_cancellation(dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_a_constant_tracer_gives_zeros_of_the_statements_signs(dtype):
    TF.check_a_constant_tracer(dtype)


def test_equals_the_chain_with_its_labels(monkeypatch):
    """the chain itself, through the same library: values, dims, coords and names"""
    calls = TF._counted(monkeypatch, bar_chain=False)
    cases = (TF.matrix_cases(("periodic", "extend", "fill"), np.float64) + TF.matrix_cases(("fill", "periodic", "extend"), np.float32)
             + TF.label_cases()[:16])
    for c in cases:
        got, want = c.one_pass(), c.chain()
        TR._same_labelled(got, want)
        TR._same_bits(got.values, want.values)
    assert calls["fused"] == len(cases)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_abi_layouts(dtype):
    TF.abi_layout_cases(dtype)


def test_abi_refuses_bad_calls():
    TF.abi_bad_calls()


def test_seeded_fuzz(monkeypatch):
    """120 cases over the small shapes, the boundary triples, both face positions, the fills, the NaNs, the dtype, the metric
    forms, the leading dims and all-zero fields, closed and open in turns; one call of the one-pass entry each, so that no
    case passes by falling back"""
    cases = TF.fuzz_cases()
    assert len(cases) == 120 and TF.compare_with_numpy(cases, monkeypatch) >= 10


def _resident(x):
    return DataArray(torch.from_numpy(x.values).cuda(), x.dims, name=x.name)


@pytest.mark.parametrize("closed", [True, False])
def test_hbm_in_hbm_out(monkeypatch, closed):
    calls = TF._counted(monkeypatch)
    c = TF.Case(TI.Case((2,), 5, 9, 136, np.float64, ("periodic", "extend", "fill"), "outer", "full", nan=True), closed)
    a, kwx, kwy = _resident(c.a), _resident(c.kwx), _resident(c.kwy)
    got = c.grid.redi_vertical_flux_divergence(a, kwx, kwy, **c.kw)
    assert calls == {"fused": 1, "chain": 0}
    assert isinstance(got.data, torch.Tensor) and got.data.is_cuda and got.is_device
    assert got.dims == ("time", "ZC", "YC", "XC")
    TR._same_bits(got.data.cpu().numpy(), c.want())
    assert got.data.data_ptr() not in {x.data.data_ptr() for x in (a, kwx, kwy)}     # one device result of its own
    ref = c.one_pass()
    assert isinstance(ref.data, np.ndarray)
    TR._same_bits(ref.values, got.data.cpu().numpy())


def test_under_graph_capture(monkeypatch):
    """the operator captured once, on one stream with no parallel branch, and replayed on new values in the same storage; the
    metrics are HBM-resident (the grid uploads them once, in the capture's warm-up)"""
    from xgcm_amd import graphs

    calls = TF._counted(monkeypatch)
    c = TF.Case(TI.Case((2,), 5, 40, 256, np.float64, ("periodic", "extend", "fill"), "outer", "lead"), True)
    c2 = TF.Case(TI.Case((2,), 5, 40, 256, np.float64, c.pads, "outer", "lead", seed=111), True, seed=5)
    a, kwx, kwy = _resident(c.a), _resident(c.kwx), _resident(c.kwy)
    step = graphs.capture(lambda: c.grid.redi_vertical_flux_divergence(a, kwx, kwy, **c.kw))
    for dst, src in ((a, c2.a), (kwx, c2.kwx), (kwy, c2.kwy)):
        dst.data.copy_(torch.from_numpy(src.values))
    out = step()
    torch.cuda.synchronize()
    assert calls == {"fused": 3, "chain": 0}   # two warm-up runs and the capture itself: the one pass is what the graph holds
    want = c2.want()
    assert np.isfinite(want).all() and (want != 0).mean() > 0.9 and not TI._bits_equal(want, c.want())
    got = out.data.clone().cpu().numpy()
    assert got.shape == (2, 5, 40, 256)
    TR._same_bits(got, want)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_every_tunable_value_computes_the_same(dtype):
    """`device.redi_vertical_flux_divergence` under every value of every tunable of the battery's table, on the battery's own
    shapes: bit for bit what the defaults give, and that is the numpy statement's"""
    from xgcm_amd import _hip
    from xgcm_amd import device as D

    calls, references = TF.tunable_calls(D, dtype)
    run = lambda: {k: D.tohost(fn()) for k, fn in calls.items()}  # noqa: E731
    want = run()
    for k, reference in references.items():
        assert TT._same_bits(want[k], reference()), f"{k}: the default result is not numpy's"
    bad = []
    for name, values in TT.ALTERNATIVES.items():
        before = _hip.get_tunable(name)
        try:
            for val in values:
                _hip.set_tunable(name, val)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    got = run()
                bad += [(name, val, k) for k in calls if not TT._same_bits(got[k], want[k])]
        finally:
            _hip.set_tunable(name, before)
    torch.cuda.synchronize()
    assert not bad, bad[:20]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_between_guard_bands_on_the_device(monkeypatch, dtype):
    """the same table with the result and all six uploaded inputs between guard bands, the payload 512-byte aligned, 16 bytes
    and one element off"""
    from xgcm_amd import device as D

    for offset in (0, 16, np.dtype(dtype).itemsize):
        assert TF.guarded_table(D, monkeypatch, dtype, offset, TT._same_bits) == 8
    torch.cuda.synchronize()
