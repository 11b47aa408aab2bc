"""The argument order of the fused entry points, without a GPU and without a library: `device._MEM` is swapped for a memory
whose `lib()` records what it is called with, and every recorded argument is compared with the value expected for the
parameter of THAT name in include/xgcm_hip.h.  For the entries the host build of the ABI answers with "unsupported"
(gradient, flux and the four `_halo` forms) no other CPU test sees the order.  CPU only, milliseconds."""

import ctypes
import math

import pytest
import torch

from test_host_logic import header_prototypes
from xgcm_amd import _hip, device

PROTOS = header_prototypes()
STREAM = 0x5EED
SHAPE = (2, 3, 4)


class RecordingLib:
    """every attribute is an entry point that records its arguments and reports success"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0

        return entry


class RecordingMemory:
    """`xgcm_amd.device.HipMemory`'s interface over host tensors and a library that only records"""

    device = "cpu"

    def __init__(self):
        self.recorder = RecordingLib()

    def require(self):
        pass

    def lib(self):
        return self.recorder

    def stream(self):
        return STREAM

    def holds(self, t):
        return not t.is_cuda

    def place(self, t, private=False):
        return t

    def check_current(self, t):
        pass

    def check(self, status):
        assert status == 0

    def after_read(self):
        pass

    def streams_host_blocks(self):
        return False


@pytest.fixture
def recorder(monkeypatch):
    mem = RecordingMemory()
    monkeypatch.setattr(device, "_MEM", mem)
    return mem.recorder


def _field(dtype, shape=SHAPE):
    return torch.arange(math.prod(shape), dtype=dtype).reshape(shape) + 1


def _same(got, want) -> bool:
    if isinstance(got, ctypes.Array):
        got = tuple(got)
    if isinstance(want, float):  # a fill: the value AND its sign bit
        return isinstance(got, float) and got == want and math.copysign(1.0, got) == math.copysign(1.0, want)
    return type(got) is type(want) and got == want


def _check_call(recorder, entry, expected):
    """the one recorded call is `entry`, and its arguments are `expected`, keyed by the header's parameter names"""
    assert [name for name, _ in recorder.calls] == [entry]
    names = [pname for _, pname in PROTOS[entry][1]]
    assert sorted(names) == sorted(expected), set(names) ^ set(expected)
    args = recorder.calls[0][1]
    assert len(args) == len(names)
    wrong = [f"{n}: {tuple(a) if isinstance(a, ctypes.Array) else a!r}, expected {expected[n]!r}" for n, a in zip(names, args)
             if not _same(a, expected[n])]
    assert not wrong, "\n".join(wrong)


# (wrapper, the fields it takes, the metrics it takes): the six entries the host ABI does not serve
CASES = {
    "gradient": ("gradient", ("a",), ("mx", "my")),
    "flux": ("flux", ("u", "v", "t"), ()),
    "gradient_halo": ("gradient", ("a",), ("mx", "my")),
    "flux_halo": ("flux", ("u", "v", "t"), ()),
    "vorticity_halo": ("vorticity", ("u", "v"), ("area",)),
    "divergence_halo": ("divergence", ("u", "v"), ("area",)),
}


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_argument_order_of_the_entries_the_host_abi_does_not_serve(recorder, case, dtype):
    """X periodic, Y a halo axis (the plain forms: a fill axis), fills 1.5 and -0.0, each metric broadcast on one dim"""
    wrapper, fields, metrics = CASES[case]
    halo = case.endswith("_halo")
    vals = {n: _field(dtype) for n in fields}
    # metric k is broadcast on dim k: extent 1 there, stride 0 in the call
    for k, n in enumerate(metrics):
        vals[n] = _field(dtype, tuple(1 if d == k else s for d, s in enumerate(SHAPE)))
    halo_y = _field(dtype, (SHAPE[0], SHAPE[2])) if halo else None
    bc = dict(bc_x="periodic", bc_y="halo" if halo else "fill", fill_x=1.5, fill_y=-0.0)
    res = getattr(device, wrapper)(**vals, **bc, halo_x=None, halo_y=halo_y)
    res = res if isinstance(res, tuple) else (res,)
    assert all(tuple(r.shape) == SHAPE and r.dtype == dtype for r in res)

    expected = {n: vals[n].data_ptr() for n in fields + metrics}
    for k, n in enumerate(metrics):
        expected[n + "_strides"] = tuple(0 if d == k else st for d, st in enumerate(vals[n].stride()))
        assert expected[n + "_strides"].count(0) == 1
    expected.update(zip(("out",) if len(res) == 1 else ("out_x", "out_y"), (r.data_ptr() for r in res)))
    if halo:
        expected.update(halo_x=None, halo_y=halo_y.data_ptr())  # NULL where the axis is not a halo axis
    expected.update(shape=SHAPE, ndim=3, bc_x=_hip.BC["periodic"], fill_x=1.5, bc_y=_hip.BC[bc["bc_y"]], fill_y=-0.0, stream=STREAM)
    assert len(set(v for v in expected.values() if isinstance(v, int) and v > 4096)) == len(fields + metrics) + len(res) + halo + 1
    _check_call(recorder, f"xg_{case}_{'f64' if dtype == torch.float64 else 'f32'}", expected)


def test_an_empty_result_returns_without_a_call(recorder):
    out_x, out_y = device.gradient(_field(torch.float64, (0, 3, 4)), "periodic", "fill")
    assert tuple(out_x.shape) == tuple(out_y.shape) == (0, 3, 4) and not recorder.calls


def _slot_names(row, halo):
    names = ["dtype"] if row.typed else []
    for s in row.slots:
        if s.kind == "halo" and not halo:
            continue
        names += {"metric": [s.name, s.name + "_strides"], "shape": ["shape", "ndim"], "bc": [s.name, *s.fills]}.get(s.kind, [s.name])
    return names


def test_every_row_names_its_slots_as_the_header_names_the_parameters():
    """a wrapper's values reach the slots by name, so the names of a row, in order, are the header's parameter names"""
    seen = 0
    for name, row in _hip.FUSED.items():
        for entry, halo in _hip.forms(name):
            for full in [entry] if row.typed else [entry + "_f64", entry + "_f32"]:
                assert _slot_names(row, halo) == [pname for _, pname in PROTOS[full][1]], full
                seen += 1
    assert seen == 2 * 17 + 10  # 13 pairs and their four `_halo` forms, ten typed entries
