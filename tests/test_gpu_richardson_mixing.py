"""The Pacanowski-Philander mixing coefficients on the GPU: `Grid.richardson_mixing` (K7p, one launch) through libxgcm_hip.so
against the numpy statement of the chain it replaces, both results bit for bit (NaN where the other is NaN, -0.0 is not
+0.0), with the closure's properties asserted on every result.  The case builders are those of
tests/test_richardson_mixing.py.  The entry takes its element type as an argument, so the battery of
tests/test_gpu_tunables.py (which looks for `_f64` / `_f32` entries) does not meet it: the sweep over every value of every
launch-shape tunable and the guarded table run here."""

import warnings

import numpy as np
import pytest
import torch

import test_gpu_tunables as TT
import test_richardson_mixing as TM
import test_richardson_number as TR
from xgcm_amd import DataArray

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nx", TR.NXS)
def test_small_shapes(monkeypatch, nx):
    cases = TM.mixed(TR.shape_cases(nx), TR.NXS.index(nx))
    assert len(cases) == len(TR.NZS) * len(TR.NYS)
    TM.compare_with_numpy(cases, monkeypatch)


@pytest.mark.parametrize("pz", TR.BCS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_every_boundary_triple(monkeypatch, pz, dtype):
    cases = [m for px in TR.BCS for py in TR.BCS for m in TM.mixed(TR.matrix_cases((px, py, pz), dtype), TR.PADS3.index((px, py, pz)))]
    solid, unstable = TM.compare_with_numpy(cases, monkeypatch)
    assert unstable > 0 and solid >= (9 if pz == "fill" else 0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_metric_forms_and_leading_dims(monkeypatch, dtype):
    solid, unstable = TM.compare_with_numpy(TM.mixed(TR.metric_cases(dtype)), monkeypatch)
    assert solid > 0 and unstable > 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("nx", [515, 516])
def test_mid_size(monkeypatch, dtype, nx):
    solid, unstable = TM.compare_with_numpy(TM.mid_size_cases(dtype, nx), monkeypatch)
    assert unstable > 1000


@pytest.mark.parametrize("to", TR.TOS)
def test_a_nan_poisons_exactly_what_the_chain_has_as_nan(to):
    for pads in (("periodic", "periodic", "periodic"), ("extend", "fill", "fill"), ("fill", "extend", "fill")):
        TM.check_nan_locality(to, pads)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_without_a_floor_zero_over_zero_is_nan_exactly_where_the_reference_has_it(dtype):
    TM.check_zero_over_zero(dtype)


def test_equals_the_chain_with_its_labels(monkeypatch):
    """the chain itself, through the same library (its squared shear is K7n's one pass): values, dims, coords and names"""
    calls = TM._counted(monkeypatch)
    cases = TM.mixed(TR.matrix_cases(("periodic", "extend", "fill"), np.float64) + TR.matrix_cases(("fill", "periodic", "extend"), np.float32))
    for m in cases:
        for got, want in zip(m.one_pass(), m.chain(s2_written_out=False)):
            TR._same_labelled(got, want)
            TR._same_bits(got.values, want.values)
    assert calls["fused"] == len(cases)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_abi_layouts(dtype):
    TM.abi_layout_cases(dtype)


def test_abi_refuses_bad_calls():
    TM.abi_bad_calls()


def test_seeded_fuzz(monkeypatch):
    """120 cases over the small shapes, the boundary triples, both face positions, the fills, the NaNs, the dtype, the metric
    forms, the leading dims and the scalar sets; one call of the one-pass entry each, so that no case passes by falling back"""
    cases = TM.fuzz_cases()
    solid, unstable = TM.compare_with_numpy(cases, monkeypatch)
    assert len(cases) == 120 and solid >= 5 and unstable > 0


def _resident(x):
    return DataArray(torch.from_numpy(x.values).cuda(), x.dims, name=x.name)


def test_hbm_in_hbm_out(monkeypatch):
    calls = TM._counted(monkeypatch, bar_chain=True)
    m = TM.Mix(TR.Case((2,), 5, 9, 136, np.float64, ("periodic", "extend", "fill"), "outer", "full", nan=True), TM.SCALARS[1])
    f = tuple(_resident(x) for x in m.c.f)
    got = m.c.grid.richardson_mixing(*f, **m.given, **m.c.kw)
    assert calls == {"fused": 1, "chain": 0}
    for g, want in zip(got, m.want()):
        assert isinstance(g.data, torch.Tensor) and g.data.is_cuda and g.is_device
        assert g.dims == ("time", "ZO", "YC", "XC")
        TR._same_bits(g.data.cpu().numpy(), want)
    for g, ref in zip(got, m.one_pass()):
        assert isinstance(ref.data, np.ndarray)
        TR._same_bits(ref.values, g.data.cpu().numpy())


@pytest.mark.parametrize("to", TR.TOS)
def test_nu_and_kappa_feed_the_implicit_solves(to):
    one, other = TM.end_to_end(to, np.float64, dict(s2_written_out=False))
    for got, want in zip(one, other):
        TR._same_labelled(got, want)
        TR._same_bits(got.values, want.values)


def test_under_graph_capture(monkeypatch):
    """the operator captured once, on one stream with no parallel branch, and replayed on new values in the same storage; the
    metrics have the fields' own shape and are HBM-resident (the grid uploads them once, in the capture's warm-up)"""
    from xgcm_amd import graphs

    calls = TM._counted(monkeypatch, bar_chain=True)
    c = TR.Case((2,), 5, 40, 256, np.float64, ("periodic", "extend", "fill"), "outer", "lead")
    c2 = TR.Case((2,), 5, 40, 256, np.float64, c.pads, "outer", "lead", seed=111)
    f, f2 = tuple(_resident(x) for x in c.f), tuple(_resident(x) for x in c2.f)
    step = graphs.capture(lambda: c.grid.richardson_mixing(*f, **TM.SCALARS[1], **c.kw))
    for a, a2 in zip(f, f2):
        a.data.copy_(a2.data)
    out = step()
    torch.cuda.synchronize()
    assert calls == {"fused": 3, "chain": 0}   # two warm-up runs and the capture itself: the one pass is what the graph holds
    want = TM.Mix(c2, TM.SCALARS[1]).want()
    for g, w in zip(out, want):
        got = g.data.clone().cpu().numpy()
        assert got.shape == (2, 6, 40, 256)
        TR._same_bits(got, w)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_every_tunable_value_computes_the_same(dtype):
    """`device.richardson_mixing` under every value of every tunable of the battery's table, on the battery's own shapes: bit
    for bit what the defaults give, and that is the numpy statement's"""
    from xgcm_amd import _hip
    from xgcm_amd import device as D

    calls, references = TM.tunable_calls(D, dtype)
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
        assert TM.guarded_table(D, monkeypatch, dtype, offset, TT._same_bits) == 16
    torch.cuda.synchronize()
