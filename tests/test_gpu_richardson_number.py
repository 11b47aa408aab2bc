"""The squared vertical shear and the Richardson number on the GPU: `Grid.vertical_shear_squared` and
`Grid.richardson_number` (K7n, one launch each) through libxgcm_hip.so against the numpy statement of the chain of nine
launches they replace, bit for bit (NaN where the other is NaN, -0.0 is not +0.0).  The case builders are those of
tests/test_richardson_number.py.  The last test runs the entry under every value of every launch-shape tunable: the battery
of tests/test_gpu_tunables.py looks for `_f64` / `_f32` entries and this one takes its element type as an argument."""

import numpy as np
import pytest
import torch

import test_gpu_tunables as TT
import test_richardson_number as TR
from oracle import refimpl as R
from xgcm_amd import DataArray

pytestmark = pytest.mark.gpu


def _run(monkeypatch, cases):
    """both operators of every case against numpy; one call of the one-pass entry per operator and case"""
    calls = TR._counted(monkeypatch)
    solid = TR.compare_with_numpy(cases)
    assert calls == [True, False] * len(cases)
    return solid


@pytest.mark.parametrize("nx", TR.NXS)
def test_small_shapes(monkeypatch, nx):
    cases = TR.shape_cases(nx)
    assert len(cases) == len(TR.NZS) * len(TR.NYS)
    _run(monkeypatch, cases)


@pytest.mark.parametrize("pz", TR.BCS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_every_boundary_triple(monkeypatch, pz, dtype):
    solid = 0
    for px, py in [(a, b) for a in TR.BCS for b in TR.BCS]:
        solid += _run(monkeypatch, TR.matrix_cases((px, py, pz), dtype))
    assert solid >= (18 if pz == "fill" else 0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_metric_forms_and_leading_dims(monkeypatch, dtype):
    assert _run(monkeypatch, TR.metric_cases(dtype)) > 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("nx", [515, 516])
def test_mid_size(monkeypatch, dtype, nx):
    _run(monkeypatch, TR.mid_size_cases(dtype, nx))


@pytest.mark.parametrize("to", TR.TOS)
def test_a_nan_poisons_exactly_what_the_chain_has_as_nan(to):
    for pads in (("periodic", "periodic", "periodic"), ("extend", "fill", "fill"), ("fill", "extend", "fill")):
        TR.check_nan_locality(to, pads)


def test_equals_the_chain_with_its_labels(monkeypatch):
    """the chain of nine launches itself, through the same library: values, dims, coords and name"""
    calls = TR._counted(monkeypatch)
    cases = TR.matrix_cases(("periodic", "extend", "fill"), np.float64) + TR.matrix_cases(("fill", "periodic", "extend"), np.float32)
    for c in cases:
        for got, want in zip(c.one_pass(), c.chain()):
            TR._same_labelled(got, want)
            TR._same_bits(got.values, want.values)
    assert calls == [True, False] * len(cases)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_abi_layouts(dtype):
    TR.abi_layout_cases(dtype)


def test_abi_refuses_bad_calls():
    TR.abi_bad_calls()


def test_seeded_fuzz(monkeypatch):
    """240 cases over the small shapes, the boundary triples, both face positions, the fills, the NaNs, the dtype, the metric
    forms and the leading dims; 240 calls of the one-pass entry per operator, so that no case passes by falling back"""
    calls = TR._counted(monkeypatch)
    cases = TR.fuzz_cases()
    solid = TR.compare_with_numpy(cases)
    assert len(cases) == 240 and calls.count(True) == 240 and calls.count(False) == 240 and solid >= 10


def _resident(x):
    return DataArray(torch.from_numpy(x.values).cuda(), x.dims, name=x.name)


def test_hbm_in_hbm_out(monkeypatch):
    calls = TR._counted(monkeypatch)
    c = TR.Case((2,), 5, 9, 136, np.float64, ("periodic", "extend", "fill"), "outer", "full", nan=True)
    f = tuple(_resident(x) for x in c.f)
    got = (c.grid.richardson_number(*f, **c.kw), c.grid.vertical_shear_squared(*f[1:], **c.kw))
    assert calls == [True, False]
    for g, want in zip(got, c.want()):
        assert isinstance(g.data, torch.Tensor) and g.data.is_cuda and g.is_device
        assert g.dims == ("time", "ZO", "YC", "XC")
        TR._same_bits(g.data.cpu().numpy(), want)
    for g, ref in zip(got, c.one_pass()):
        assert isinstance(ref.data, np.ndarray)
        TR._same_bits(ref.values, g.data.cpu().numpy())


def test_under_graph_capture(monkeypatch):
    """the operator captured once and replayed on new values in the same storage; the metrics have the fields' own shape and
    are HBM-resident (the grid uploads them once, in the capture's warm-up)"""
    from xgcm_amd import graphs

    calls = TR._counted(monkeypatch)
    c = TR.Case((2,), 5, 40, 256, np.float64, ("periodic", "extend", "fill"), "outer", "lead")
    c2 = TR.Case((2,), 5, 40, 256, np.float64, c.pads, "outer", "lead", seed=111)
    f, f2 = tuple(_resident(x) for x in c.f), tuple(_resident(x) for x in c2.f)
    step = graphs.capture(lambda: c.grid.richardson_number(*f, **c.kw))
    for a, a2 in zip(f, f2):
        a.data.copy_(a2.data)
    out = step()
    torch.cuda.synchronize()
    assert calls == [True] * 3   # two warm-up runs and the capture itself: the one-pass entry, not the chain, is in the graph
    got = out.data.clone().cpu().numpy()
    assert got.shape == (2, 6, 40, 256)
    TR._same_bits(got, c2.want()[0])


def tunable_calls(D, dtype):
    """(calls, references) of the K7n tunable sweep: name -> thunk that calls `D` on inputs uploaded once, name -> thunk
    that gives numpy's result of the same call; tests/test_gpu_guarded_memory.py runs the same table between guard bands"""
    f = lambda shape, seed: R.synthetic_field(shape, seed).astype(dtype)  # noqa: E731
    m = lambda shape, seed: R.synthetic_metric(shape, seed).astype(dtype)  # noqa: E731
    calls, references = {}, {}
    for n, shape in enumerate(((5, 300, 264), (3, 65, 131))):
        nz, ny, nx = shape
        b, u, v = (f(shape, 150 + 3 * n + k) for k in range(3))
        u[1, 7, 9] = v[0, 0, 0] = b[nz - 1, ny - 1, nx - 1] = np.nan
        dev = tuple(D.asdevice(x) for x in (b, u, v))
        for k, (to, pads) in enumerate((("left", ("periodic", "extend", "fill")), ("outer", ("extend", "fill", "periodic")),
                                        ("left", ("fill", "periodic", "extend")), ("outer", ("periodic", "periodic", "fill")))):
            nf = nz + (to == "outer")
            mets = [m((nf, 1, 1), 170)] * 3 if k % 2 else [m((nf, ny, nx), 171 + j) for j in range(3)]
            ri = k != 2                                   # (the third: the squared shear alone)
            dm = tuple(D.asdevice(x) for x in mets)
            key = f"{nx}{to}{pads[2]}"
            fill = [TR.FILL[a] for a in "XYZ"]
            calls[key] = lambda dev=dev, dm=dm, to=to, pads=pads, ri=ri: D.richardson_number(
                dev[0] if ri else None, dev[1], dev[2], *dm, to == "outer", *pads, *fill)
            references[key] = lambda h=(b, u, v), mets=mets, to=to, pads=pads, ri=ri: TR._want(
                h[0] if ri else None, h[1], h[2], pads, to, TR.FILL, *(mets if ri else mets[:2]))
    return calls, references


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_every_tunable_value_computes_the_same(dtype):
    """`device.richardson_number` under every value of every tunable of the battery's table, on the battery's own shapes, both
    face positions, with and without b and both forms of the metrics: bit for bit what the defaults give, and that is
    numpy's"""
    import warnings

    from xgcm_amd import _hip
    from xgcm_amd import device as D

    calls, references = tunable_calls(D, dtype)
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
