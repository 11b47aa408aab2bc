"""The tapered off-diagonal tensor components at the U and V points on the GPU: `Grid.redi_horizontal_tensor` (K7u, one launch)
through libxgcm_hip.so against the numpy statement of the chain it replaces, both results bit for bit (NaN where the other has
NaN, -0.0 is not +0.0); the statement is held to its own conditions (`Case.solid`) and to the properties of the docstring
before the kernel is asked to match it.  The case builders are those of tests/test_redi_horizontal_tensor.py.  The entry takes
its element type as an argument, so the battery of tests/test_gpu_tunables.py (which looks for `_f64` / `_f32` entries) does
not meet it: the sweep over every value of every launch-shape tunable and the guarded table run here."""

import warnings

import numpy as np
import pytest
import torch

import test_gpu_tunables as TT
import test_isopycnal_slope as TI
import test_redi_horizontal_tensor as TH
import test_richardson_number as TR
from xgcm_amd import DataArray

pytestmark = pytest.mark.gpu


def test_small_shapes(monkeypatch):
    cases = TH.shape_cases()
    assert len(cases) == len(TI.NZS) * len(TI.NYS) * len(TI.NXS)
    assert TH.compare_with_numpy(cases, monkeypatch) >= 15


@pytest.mark.parametrize("pz", TI.BCS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_every_boundary_triple(monkeypatch, pz, dtype):
    cases = [c for px in TI.BCS for py in TI.BCS for c in TH.matrix_cases((px, py, pz), dtype)]
    assert TH.compare_with_numpy(cases, monkeypatch) >= 9


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_metric_forms_and_leading_dims(monkeypatch, dtype):
    assert TH.compare_with_numpy(TH.metric_cases(dtype), monkeypatch) > 10


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("nx", [515, 516])
def test_mid_size(monkeypatch, dtype, nx):
    assert TH.compare_with_numpy(TH.mid_size_cases(dtype, nx), monkeypatch) == 2


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_fills_keep_their_bits(monkeypatch, dtype):
    assert TH.compare_with_numpy(TH.fill_cases(dtype), monkeypatch) == 8


def test_seeded_fuzz(monkeypatch):
    cases = TH.fuzz_cases()
    assert len(cases) == 120 and TH.compare_with_numpy(cases, monkeypatch) >= 10


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_several_segments_and_tiles_per_lead_index(monkeypatch, dtype):
    """(2, 3, 37, 1030): nineteen Y segments, the last one ragged, and several X tiles, the last one partial, per lead index;
    full metrics, then none and the narrow form's odd nx"""
    cases = [TH.Case(TI.Case((2,), 3, 37, 1030, dtype, ("periodic", "extend", "fill"), "outer", "full"), 2.0),
             TH.Case(TI.Case((2,), 3, 37, 1030, dtype, ("fill", "periodic", "extend"), "left", "planes"), 1e-2, 2.5),
             TH.Case(TI.Case((2,), 3, 37, 1029, dtype, ("extend", "fill", "periodic"), "outer", None), None, 3)]
    assert TH.compare_with_numpy(cases, monkeypatch) == 3


def test_equals_the_chain_with_its_labels(monkeypatch):
    """the chain itself, through the same library: values, dims, coords and names"""
    calls = TH._counted(monkeypatch, bar_chain=False)
    cases = (TH.matrix_cases(("periodic", "extend", "fill"), np.float64) + TH.matrix_cases(("fill", "periodic", "extend"), np.float32)
             + TH.label_cases()[:12])
    for c in cases:
        with np.errstate(all="ignore"):
            for got, want in zip(c.one_pass(), c.chain()):
                TR._same_labelled(got, want)
                TR._same_bits(got.values, want.values)
    assert calls["fused"] == len(cases)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_abi_layouts(dtype):
    TH.abi_layout_cases(dtype)


def test_abi_refuses_bad_calls():
    TH.abi_bad_calls()


def test_hbm_in_hbm_out(monkeypatch):
    calls = TH._counted(monkeypatch)
    c = TH.Case(TI.Case((2,), 5, 9, 136, np.float64, ("periodic", "extend", "fill"), "outer", "full", nan=True), 2.0)
    b = DataArray(torch.from_numpy(c.base.b.values).cuda(), c.base.b.dims, name=c.base.b.name)
    got = c.base.grid.redi_horizontal_tensor(b, c.kappa, 2.0, **c.base.kw)
    assert calls == {"fused": 1, "chain": 0} and len(got) == 2
    for g, want, dims in zip(got, c.want(), (TH.DIMS_U, TH.DIMS_V)):
        assert isinstance(g.data, torch.Tensor) and g.data.is_cuda and g.is_device and g.dims == ("time",) + dims
        TR._same_bits(g.data.cpu().numpy(), want)
    assert len({g.data.data_ptr() for g in got}) == 2


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_every_tunable_value_computes_the_same(dtype):
    """`device.redi_horizontal_tensor` under every value of every tunable of the battery's table (every launch-shape tunable
    that reaches the isopycnal plan is among them), on the battery's own shapes: bit for bit what the defaults give, and
    that is the numpy statement's"""
    from xgcm_amd import _hip
    from xgcm_amd import device as D

    calls, references = TH.tunable_calls(D, dtype)
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
        assert TH.guarded_table(D, monkeypatch, dtype, offset, TT._same_bits) == 16
    torch.cuda.synchronize()
