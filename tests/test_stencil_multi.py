"""xg_stencil_multi over the HOST build of the ABI: up to four plain two-point results of one field from one read, against
`device.stencil1d` one operator at a time and against the oracle, bit for bit; every declined form returns XG_DECLINED,
writes nothing, and the caller's fallback gives the single-operator results.  tests/test_gpu_stencil_multi.py runs the same
cases through the kernel (shapes and request sets: tests/stencil_multi_cases.py)."""

import numpy as np
import pytest

import stencil_multi_cases as MC

torch = pytest.importorskip("torch")

DTYPES = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])


@DTYPES
@pytest.mark.parametrize("outer", MC.OUTER)
@pytest.mark.parametrize("ny", MC.HEIGHTS)
def test_every_request_set_equals_the_single_operators(host_abi, dtype, outer, ny):
    from xgcm_amd import device as D

    for nx in MC.rows_of(dtype):
        MC.check_shape(D, (outer, ny, nx), dtype)


@DTYPES
def test_two_dims_are_served_and_four_or_odd_rows_declined(host_abi, dtype):
    from xgcm_amd import device as D

    MC.check_shape(D, (5, 8), dtype, sets=MC.SETS[-6:])            # (Y, X): outer = 1
    MC.check_shape(D, (2, 2, 5, 8), dtype, sets=MC.SETS[-6:])      # 4-D: declined
    MC.check_shape(D, (3, 5, 7), dtype, sets=MC.SETS[-6:])         # odd rows: declined


def _declined(D, x, requests, **kw):
    """XG_DECLINED, and nothing written"""
    from xgcm_amd import _hip

    status, outs = MC.raw_status(D, x, requests, **kw)
    return status == _hip.DECLINED and all(bool((t == 7.0).all()) for t in outs if t is not None)


@DTYPES
def test_every_declined_form(host_abi, dtype):
    from xgcm_amd import _hip
    from xgcm_amd import device as D

    a = MC.field((3, 5, 8), dtype)
    x = D.asdevice(a)
    ok = ("diff", MC.X, 1, 0, "periodic", 0.0)
    assert MC.raw_status(D, x, [ok])[0] == 0
    assert _declined(D, x, [("diff", 0, 1, 0, "fill", 0.0)])                  # the Z axis
    assert _declined(D, x, [ok, ("interp", MC.Y, 1, 1, "extend", 0.0)])       # pads (1, 1)
    assert _declined(D, x, [ok, ("interp", MC.Y, 0, 0, "extend", 0.0)])       # pads (0, 0)
    assert _declined(D, x, [("diff", MC.X, 1, 0, None, 0.0)])                 # no boundary mode
    assert _declined(D, x, [("diff", MC.X, 1, 0, "halo", 0.0)])               # halo mode
    assert _declined(D, D.asdevice(MC.field((2, 2, 5, 8), dtype)), [ok])      # four dims
    assert _declined(D, D.asdevice(MC.field((3, 5, 7), dtype)), [ok])         # odd rows
    # rows that do not start on 16 bytes: a view one element into a longer buffer
    nv = 16 // np.dtype(dtype).itemsize
    buf = D.asdevice(np.zeros(3 * 5 * 8 + nv, dtype))
    off = buf[1:1 + 3 * 5 * 8].view(3, 5, 8)
    assert off.data_ptr() % 16 != 0 and _declined(D, off, [ok])
    assert _declined(D, x, [ok], outs=[torch.full((3 * 5 * 8 + nv,), 7.0, dtype=x.dtype)[1:1 + 3 * 5 * 8].view(3, 5, 8)])
    # results that overlap the input or each other
    status, _ = MC.raw_status(D, x, [ok], outs=[x])
    assert status == _hip.DECLINED and MC.same_bits(D.tohost(x), a)
    shared = torch.full((3, 5, 8), 7.0, dtype=x.dtype)
    assert _declined(D, x, [ok, ("interp", MC.X, 1, 0, "periodic", 0.0)], outs=[shared, shared])
    two = torch.full((2 * 3 * 5 * 8,), 7.0, dtype=x.dtype)
    assert _declined(D, x, [ok, ok], outs=[two[:120].view(3, 5, 8), two[64:184].view(3, 5, 8)])
    # what is an ERROR, not a decline: no request, five requests, an unknown operator or element type, a NULL pointer
    for status in (MC.raw_status(D, x, [], n=0)[0], MC.raw_status(D, x, [ok] * 4, n=5)[0],
                   MC.raw_status(D, x, [(7, MC.X, 1, 0, "periodic", 0.0)])[0], MC.raw_status(D, x, [ok], dtype_code=_hip.DTYPE["int32"])[0],
                   MC.raw_status(D, x, [ok], outs=[None])[0]):
        assert status == -1


@DTYPES
def test_two_to_the_31_cells_or_more_are_declined(host_abi, dtype):
    from xgcm_amd import device as D

    MC.check_cell_limit(D, dtype)
