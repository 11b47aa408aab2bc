"""`k_stencil_multi` on the GPU: the cases of tests/test_stencil_multi.py through libxgcm_hip.so, every result (the accepted
forms' and the fallbacks') between guard bands (tests/guarded_memory.py) -- the kernel has four chances per lane to store
past a row's or an array's end -- against `device.stencil1d` one operator at a time and against the oracle, bit for bit."""

import numpy as np
import pytest

import guarded_memory as GM
import stencil_multi_cases as MC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])


@DTYPES
@pytest.mark.parametrize("outer", MC.OUTER)
@pytest.mark.parametrize("ny", MC.HEIGHTS)
def test_every_request_set_between_guards(monkeypatch, dtype, outer, ny):
    from xgcm_amd import device as D

    with GM.guarded(D, monkeypatch, 0) as g:
        for nx in MC.rows_of(dtype):
            MC.check_shape(D, (outer, ny, nx), dtype, after=g.check)
        assert g.handed_out > len(MC.SETS)


@DTYPES
def test_two_dims_declined_shapes_and_unaligned_payloads(monkeypatch, dtype):
    from xgcm_amd import device as D

    with GM.guarded(D, monkeypatch, 0) as g:
        MC.check_shape(D, (5, 8), dtype, sets=MC.SETS[-6:], after=g.check)
        MC.check_shape(D, (2, 2, 5, 8), dtype, sets=MC.SETS[-6:], after=g.check)   # 4-D: declined, the fallback between guards
        MC.check_shape(D, (3, 5, 7), dtype, sets=MC.SETS[-6:], after=g.check)      # odd rows: declined
    # payloads one element off the 16-byte grid: input and results are refused, nothing is launched, the fallback serves
    with GM.guarded(D, monkeypatch, np.dtype(dtype).itemsize) as g:
        a = MC.field((3, 5, 8), dtype)
        x = D.asdevice(a)
        assert x.data_ptr() % 16 != 0
        for s in MC.SETS[-6:]:
            assert D._multi_launch(x, s) is None
            for _ in range(3):  # the caller: such calls are no requests, every one is the single-operator kernel
                outs = [D.stencil1d(r[0], x, *r[1:]) for r in s]
            assert not D._sib_table()
            for req, out in zip(s, outs):
                assert MC.same_bits(D.tohost(out), MC.oracle(a, req)), (s, req)
            g.check(f"unaligned {s}")


@DTYPES
def test_two_to_the_31_cells_or_more_are_declined(dtype):
    """the launcher's own limit checks, on claimed shapes over a small buffer: nothing is launched either way"""
    from xgcm_amd import device as D

    MC.check_cell_limit(D, dtype)
    torch.cuda.synchronize()
