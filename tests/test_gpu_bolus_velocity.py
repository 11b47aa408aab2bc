"""The Gent-McWilliams eddy-induced (bolus) velocity on the GPU: `Grid.bolus_velocity` (K7t, one launch) through
libxgcm_hip.so against the numpy statement of the chain it replaces, bit for bit (NaN where the other has NaN, -0.0 is not
+0.0); the statement is held to its own conditions (every ordinary case finite, at least half of the cells of each result
of every table non-zero) before the kernel is asked to match it.  The case builders are those of
tests/test_bolus_velocity.py.  The entry takes its element type as an argument, so the battery of tests/test_gpu_tunables.py
(which looks for `_f64` / `_f32` entries) does not meet it: the sweep over every value of every launch-shape tunable and the
guarded table run here.  Nothing is larger than (2, 5, 40, 516)."""

import warnings

import numpy as np
import pytest
import torch

import test_bolus_velocity as TB
import test_gpu_tunables as TT
import test_richardson_number as TR
from xgcm_amd import DataArray

pytestmark = pytest.mark.gpu


def test_small_shapes(monkeypatch):
    cases = [c for nx in TB.NXS for c in TB.shape_cases(nx)]
    assert len(cases) == 4 * len(TB.NZS) * len(TB.NYS) * len(TB.NXS)
    TB.compare_with_numpy(cases, monkeypatch)


@pytest.mark.parametrize("pz", TB.BCS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_every_boundary_triple(monkeypatch, pz, dtype):
    cases = [c for px in TB.BCS for py in TB.BCS for c in TB.matrix_cases((px, py, pz), dtype)]
    assert TB.compare_with_numpy(cases, monkeypatch) >= 72


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_metric_forms_and_leading_dims(monkeypatch, dtype):
    assert TB.compare_with_numpy(TB.metric_cases(dtype), monkeypatch) > 10
    TB.check_each_metric_absent_on_its_own(dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("nx", [515, 516])
def test_mid_size(monkeypatch, dtype, nx):
    assert TB.compare_with_numpy(TB.mid_size_cases(dtype, nx), monkeypatch) == 4


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_fills_zeros_and_nans_keep_their_bits(monkeypatch, dtype):
    assert TB.compare_with_numpy(TB.fill_cases(dtype), monkeypatch) == 48
    for c in TB.zero_cases(dtype) + TB.nan_cases(dtype):
        for g, w in zip(c.one_pass(), c.want()):
            TR._same_bits(g.values, w)


def test_one_level_closed_at_outer_is_all_minus_zero(monkeypatch):
    c = TB.Case((2,), 1, 3, 8, np.float64, ("periodic", "extend", "fill"), "outer", "planes", True)
    ub, vb, wb = (g.values for g in c.one_pass())
    assert (ub == 0).all() and np.signbit(ub).all() and (vb == 0).all() and np.signbit(vb).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_closed_really_is_closed(dtype):
    TB.check_closed_is_closed(dtype)


@pytest.mark.parametrize("closed", [True, False])
@pytest.mark.parametrize("to", TB.TOS)
def test_a_nan_poisons_exactly_what_the_statement_has_as_nan(to, closed):
    for pads in (("periodic", "periodic", "periodic"), ("extend", "fill", "fill"), ("fill", "extend", "extend")):
        TB.check_nan_locality(to, pads, closed)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_on_redi_tensors_own_results(monkeypatch, dtype):
    calls = TB._counted(monkeypatch, bar_chain=False)
    TB.check_on_redi_tensors_own_results(dtype)
    assert calls["fused"] == 1


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_the_bolus_velocity_is_non_divergent_cell_by_cell(dtype):
    print(f"continuity: worst |residual| / S = {TB.check_continuity(dtype):.3f} eps")


def test_equals_the_chain_with_its_labels(monkeypatch):
    """the chain itself, through the same library: values, dims, coords and names"""
    calls = TB._counted(monkeypatch, bar_chain=False)
    cases = (TB.matrix_cases(("periodic", "extend", "fill"), np.float64) + TB.matrix_cases(("fill", "periodic", "extend"), np.float32)
             + TB.label_cases()[:16])
    for c in cases:
        for g, w in zip(c.one_pass(), c.chain()):
            TR._same_labelled(g, w)
            TR._same_bits(g.values, w.values)
    assert calls["fused"] == len(cases)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_abi_layouts(dtype):
    TB.abi_layout_cases(dtype)


def test_abi_refuses_bad_calls():
    TB.abi_bad_calls()


def test_seeded_fuzz(monkeypatch):
    """120 seeded cases, one call of the one-pass entry each, so that no case passes by falling back"""
    cases = TB.fuzz_cases()
    assert len(cases) == 120 and TB.compare_with_numpy(cases, monkeypatch) >= 40


def _resident(x):
    return DataArray(torch.from_numpy(x.values).cuda(), x.dims, name=x.name)


@pytest.mark.parametrize("closed", [True, False])
def test_hbm_in_hbm_out(monkeypatch, closed):
    calls = TB._counted(monkeypatch)
    c = TB.Case((2,), 5, 9, 136, np.float64, ("periodic", "extend", "fill"), "outer", "full", closed, nan=True)
    kwx, kwy = _resident(c.kwx), _resident(c.kwy)
    got = c.grid.bolus_velocity(kwx, kwy, **c.kw)
    assert calls == {"fused": 1, "chain": 0}
    assert all(isinstance(g.data, torch.Tensor) and g.data.is_cuda and g.is_device for g in got)
    assert tuple(g.dims for g in got) == c.dims_of()
    for g, w in zip(got, c.want()):
        TR._same_bits(g.data.cpu().numpy(), w)
    ptrs = [g.data.data_ptr() for g in got] + [kwx.data.data_ptr(), kwy.data.data_ptr()]
    assert len(set(ptrs)) == 5                                     # three device results of their own storage
    for ref, g in zip(c.one_pass(), got):
        assert isinstance(ref.data, np.ndarray)
        TR._same_bits(ref.values, g.data.cpu().numpy())


def test_under_graph_capture(monkeypatch):
    """the operator captured once, on one stream with no parallel branch, and replayed on new values in the same storage; the
    metrics are HBM-resident (the grid uploads them once, in the capture's warm-up)"""
    from xgcm_amd import graphs

    calls = TB._counted(monkeypatch)
    c = TB.Case((2,), 5, 40, 256, np.float64, ("periodic", "extend", "fill"), "outer", "lead", True)
    c2 = TB.Case((2,), 5, 40, 256, np.float64, c.pads, "outer", "lead", True, seed=5)
    kwx, kwy = _resident(c.kwx), _resident(c.kwy)
    step = graphs.capture(lambda: c.grid.bolus_velocity(kwx, kwy, **c.kw))
    for dst, src in ((kwx, c2.kwx), (kwy, c2.kwy)):
        dst.data.copy_(torch.from_numpy(src.values))
    out = step()
    torch.cuda.synchronize()
    assert calls == {"fused": 3, "chain": 0}   # two warm-up runs and the capture itself: the one pass is what the graph holds
    for o, want, old in zip(out, c2.want(), c.want()):
        assert np.isfinite(want).all() and (want != 0).mean() > 0.6 and not TB._bits_equal(want, old)
        TR._same_bits(o.data.clone().cpu().numpy(), want)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_every_tunable_value_computes_the_same(dtype):
    """`device.bolus_velocity` under every value of every tunable of the battery's table: bit for bit what the defaults give,
    and that is the numpy statement's"""
    from xgcm_amd import _hip
    from xgcm_amd import device as D

    calls, references = TB.tunable_calls(D, dtype)
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
    """the same table with the three results and all uploaded inputs between guard bands, the payload 512-byte aligned, 16
    bytes and one element off"""
    from xgcm_amd import device as D

    for offset in (0, 16, np.dtype(dtype).itemsize):
        assert TB.guarded_table(D, monkeypatch, dtype, offset, TT._same_bits) == 24
    torch.cuda.synchronize()
