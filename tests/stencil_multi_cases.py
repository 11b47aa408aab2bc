"""Shapes, request sets and comparisons shared by tests/test_stencil_multi.py (host build of the ABI) and
tests/test_gpu_stencil_multi.py (the kernel): the smallest shapes at which `k_stencil_multi` can go wrong.

Rows: one 16-byte vector (2), less than a wave (6), exactly one tile of 64 f64 lane vectors (128), one tile and one lane (130),
two tiles and one lane (258).  Heights: 1, 2, 3, and around the 4 rows of a workgroup (3, 4, 5), 9.  Outer: 1 and 3.  float32
rows need a multiple of 4 cells, so 2, 6, 130 and 258 are DECLINED there: the same cases then check the decline code and the
fallback, and 128 (half a float32 tile), 256 (one tile) and 260 (one tile and one lane) are added for float32."""

import ctypes as C
import itertools

import numpy as np

from oracle import refimpl as R

NW = 4  # rows of a workgroup (MULTI_NW in xg_stencil.hip)
ROWS = (2, 6, 128, 130, 258)
ROWS_F32 = ROWS + (256, 260)
HEIGHTS = (1, 2, NW - 1, NW, NW + 1, 9)
OUTER = (1, 3)
X, Y = -1, -2

BASE = (("interp", X, 1, 0, "periodic", 0.0), ("diff", X, 1, 0, "periodic", 0.0),
        ("interp", Y, 1, 0, "extend", 0.0), ("diff", Y, 1, 0, "extend", 0.0))
SUBSETS = [tuple(c) for k in range(1, 5) for c in itertools.combinations(BASE, k)]
MIXED = [
    (("min", X, 0, 1, "fill", -0.0), ("max", Y, 0, 1, "periodic", 0.0), ("diff", X, 1, 0, "extend", 0.0), ("interp", Y, 1, 0, "fill", 2.5)),
    (("diff", X, 0, 1, "periodic", 0.0), ("interp", X, 1, 0, "fill", 2.5), ("diff", Y, 0, 1, "extend", 0.0), ("interp", Y, 1, 0, "periodic", 0.0)),
    (("diff", Y, 1, 0, "fill", -0.0), ("diff", Y, 0, 1, "fill", 0.0), ("max", X, 0, 1, "extend", 0.0), ("min", X, 1, 0, "periodic", 0.0)),
    (("interp", X, 0, 1, "fill", -0.0), ("interp", Y, 0, 1, "fill", -0.0)),
]
SETS = SUBSETS + MIXED


def rows_of(dtype):
    return ROWS_F32 if np.dtype(dtype) == np.float32 else ROWS


def accepted(shape, dtype) -> bool:
    """what xg_stencil_multi takes of these cases: 2 or 3 dims and rows that are whole 16-byte vectors"""
    return len(shape) in (2, 3) and (shape[-1] * np.dtype(dtype).itemsize) % 16 == 0


def field(shape, dtype, seed=5):
    """a synthetic field with NaN, +-inf, -0.0 and subnormals at the row ends, the first / last rows and so at every wrap and
    clamp cell"""
    a = R.synthetic_field(shape, seed).astype(dtype)
    tiny = np.finfo(dtype).smallest_subnormal
    a[..., 0, 0] = np.nan
    a[..., -1, -1] = np.inf
    a[..., 0, -1] = -0.0
    a[..., -1, 0] = tiny
    mid = shape[-2] // 2
    b = a.reshape(-1, shape[-2], shape[-1])  # (a view)
    b[0, mid, 0] = -np.inf
    b[-1, mid, -1] = -0.0
    b[-1, mid, shape[-1] // 2] = -tiny
    if shape[-1] > 128:  # the cells on either side of the first tile's end
        a[..., mid, 127] = np.nan
        a[..., 0, 128] = -np.inf
    return a


def same_bits(got, want) -> bool:
    """NaN where the other has NaN; everywhere else the same bit pattern (-0.0 is not +0.0)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    nan = np.isnan(want)
    return np.array_equal(np.where(nan, 0, got).view(bits), np.where(nan, 0, want).view(bits))


def oracle(a, req):
    op, axis, lo, hi, bc, fill = req
    return R.stencil1d(op, a, axis % a.ndim, lo, hi, bc, a.dtype.type(fill))


def raw_status(D, x, requests, outs=None, dtype_code=None, ndim=None, n=None, shape=None):
    """the status xg_stencil_multi itself returns for these requests of the resident tensor `x` (results go to `outs`, or to
    fresh arrays of x's shape).  `shape`: the shape CLAIMED for `x` -- only for requests that are declined, which touch no
    memory"""
    import torch

    from xgcm_amd import _hip

    outs = [torch.full_like(x, 7.0) for _ in requests] if outs is None else outs
    dims = list(x.shape) if shape is None else list(shape)
    desc = (_hip.MultiDesc * max(1, len(requests)))()
    for d, (op, axis, lo, hi, bc, fill), out in zip(desc, requests, outs):
        d.op, d.axis, d.pad_lo, d.pad_hi, d.bc, d.fill = (op if isinstance(op, int) else _hip.OP[op]), axis % len(dims), lo, hi, _hip.BC[bc], fill
        d.out = out.data_ptr() if out is not None else None
    code = _hip.DTYPE[str(x.dtype).replace("torch.", "")] if dtype_code is None else dtype_code
    status = D._MEM.lib().xg_stencil_multi(code, x.data_ptr(), _hip.i64(dims), len(dims) if ndim is None else ndim,
                                           len(requests) if n is None else n, desc, D._MEM.stream())
    return status, outs


def check_shape(D, shape, dtype, sets=SETS, after=None):
    """every request set on one field of `shape`: xg_stencil_multi (or, where it declines, the decline and the fallback)
    against `device.stencil1d` one operator at a time and against the oracle, bit for bit.  `after(name)`: called after every
    library call (the guard check of the GPU twin)."""
    from xgcm_amd import _hip

    a = field(shape, dtype)
    x = D.asdevice(a)
    after = after or (lambda name: None)
    single, bad = {}, []
    with D.sibling_plans_off():
        for req in {r for s in sets for r in s}:
            single[req] = D.tohost(D.stencil1d(req[0], x, *req[1:]))
            after(f"stencil1d {req}")
            if not same_bits(single[req], oracle(a, req)):
                bad.append((shape, "stencil1d against the oracle", req))
    for s in sets:
        outs = D._multi_launch(x, s)
        if accepted(shape, dtype):
            assert outs is not None, (shape, s)
        else:
            assert outs is None, (shape, s)
            status, untouched = raw_status(D, x, s)
            assert status == _hip.DECLINED == 1 and all(bool((t == 7.0).all()) for t in untouched), (shape, s)
            # the caller's fallback: `stencil1d` itself, round after round with the plan switched on -- such calls are no requests
            D.drop_sibling_plans()
            for _ in range(3):
                outs = [D.stencil1d(r[0], x, *r[1:]) for r in s]
            assert not D._sib_table()
        after(f"multi {s}")
        for req, out in zip(s, outs):
            if not same_bits(D.tohost(out), single[req]):
                bad.append((shape, s, req))
    assert not bad, bad[:10]


def last_error(D) -> str:
    buf = C.create_string_buffer(512)
    D._MEM.lib().xg_last_error(buf, 512)
    return buf.value.decode(errors="replace")


def check_cell_limit(D, dtype):
    """"2^31 cells or more" is declined -- by the row length, by the plane, by the whole array -- and 2^31 - 1 is the last count
    that passes.  A decline touches no memory, so the shapes are CLAIMED for a small buffer.  The largest shapes under the
    limit are shown to PASS that check without running them: with a result that overlaps the input they are declined by the
    overlap check, which comes after it (the decline names its condition in xg_last_error)."""
    from xgcm_amd import _hip

    x = D.asdevice(field((2, 4, 8), dtype))
    ok = ("diff", X, 1, 0, "periodic", 0.0)
    oy = ("interp", Y, 1, 0, "extend", 0.0)
    nv = 16 // np.dtype(dtype).itemsize
    over = [(1, 65536, 32768),            # exactly 2^31 cells
            (3, 46341, 46344),            # a plane of more than 2^31 cells (46341 * 46344 = 2^31 + 143657), products that overflow 32 bits
            (3, 32768, 32768),            # planes of 2^30 cells, 3 * 2^30 in all
            (1, 1, 2 ** 31),              # one row of 2^31 cells
            (2 ** 31, 8),                 # 2^31 rows
            (2 ** 33, 1, 8),              # an outer extent beyond 32 bits
            (4, 2 ** 31 - nv), (2 ** 20, 2 ** 20, 2 ** 24)]  # ... whose products wrap to small numbers in 32 and in 64 bits
    for shape in over:
        for reqs in ([ok], [ok, oy]):
            status, outs = raw_status(D, x, reqs, shape=shape)
            assert status == _hip.DECLINED and "2^31 cells" in last_error(D), (shape, status, last_error(D))
            assert all(bool((t == 7.0).all()) for t in outs), shape
    under = [(1, 1, 2 ** 31 - nv), (1, (2 ** 31 - 1) // nv, nv), ((2 ** 31 - 1) // (8 * nv), 8, nv)]  # the most cells rows of whole vectors can have
    before = D.tohost(x).copy()
    for shape in under:
        cells = int(np.prod([int(v) for v in shape], dtype=object))
        assert cells <= 2 ** 31 - 1 and shape[-1] % nv == 0, shape
        status, _ = raw_status(D, x, [ok], outs=[x], shape=shape)
        assert status == _hip.DECLINED and "overlaps the input" in last_error(D), (shape, status, last_error(D))
    assert same_bits(D.tohost(x), before)
