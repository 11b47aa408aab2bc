"""Unlabelled-array layer: HBM-resident arrays in, HBM-resident arrays out (float64 / float32 in their own dtype, integer
and bool arrays exact on int64 lanes -- see xgcm_amd.dtypes).

Each function is one C-ABI call (include/xgcm_hip.h).  PyTorch is used only as plumbing: it owns
the device allocations (`torch.empty`), and its current HIP stream is the stream the kernels are
enqueued on, so `torch.cuda.Event`, `torch.distributed` and user torch code order correctly
against them.  No arithmetic is delegated to torch and there is no CPU path: without a GPU or
without the built library every function raises.

Return types: an HBM `torch.Tensor`, except that `stencil1d` / `cumsum1d` / `reduce1d` handed a HOST array of
`HOST_STREAM_MIN_BYTES` or more return a host `numpy.ndarray` (the block-wise pipelined path below brings the result
back block by block; callers that need a tensor -- `sharding.cumsum_along_sharded_axis` -- normalise).

Metric arguments (`m_in`, `m_out`, `w`, `area`) are tensors with the same number of dims as
the array they weight, each dim either full-size or 1 (broadcast) -- the alignment xarray does
for `da * metric` (reference xgcm/grid.py:806-808,830-832).
"""

from __future__ import annotations

import contextlib
import functools
import os
import threading
import weakref
from collections import OrderedDict
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _hip
from . import dtypes as _dt

__all__ = [
    "convert",
    "asdevice",
    "tohost",
    "is_device_array",
    "stencil1d",
    "stencil1d_halo",
    "drop_sibling_plans",
    "SIBLING_STATS",
    "cumsum1d",
    "reduce1d",
    "pad_nd",
    "gather",
    "put_halo",
    "upload_tokens",
    "transform_linear",
    "transform_conservative",
    "binary",
    "vorticity",
    "divergence",
    "gradient",
    "flux",
    "stencil2d",
    "stencil2d_supported",
    "synthetic",
]


class HipMemory:
    """Where the arrays of this layer live and which build of the C ABI serves them.  The product has exactly ONE: tensors in
    the HBM of the current GPU, libxgcm_hip.so, torch's current HIP stream -- and no CPU fallback: without a GPU `require`
    raises, without the built library `lib` does.  Everything else in this module (dtype / lane plans, geometry, metric
    strides, halo slabs, the slice-by-slice binary, block-wise host streaming) is written against these few methods, so that
    the CPU suite runs THE SAME planning code over host memory and the host build of the ABI (tests/host_abi_device.py swaps
    this object for its own; VERDICT r05 "one planner").  Nothing under xgcm_amd/ defines or selects another memory."""

    device = "cuda"

    def require(self) -> None:
        if not torch.cuda.is_available():
            raise RuntimeError(
                "xgcm_amd needs an AMD GPU (torch.cuda.is_available() is False); there is no CPU fallback."
            )

    def lib(self):
        return _hip.load()

    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    def holds(self, t: torch.Tensor) -> bool:
        return t.is_cuda

    def place(self, t: torch.Tensor, private: bool = False) -> torch.Tensor:
        """a host tensor -> this memory (PCIe copy); `private`: the caller is going to modify the copy in place"""
        return t.cuda()

    def check_current(self, t: torch.Tensor) -> None:
        # kernels are enqueued on the CURRENT device's stream (one process per GPU is the model)
        if t.device.index != torch.cuda.current_device():
            raise RuntimeError(f"array lives on {t.device} but the current device is cuda:{torch.cuda.current_device()}; "
                               "call torch.cuda.set_device() for that GPU first")

    def check(self, status: int) -> None:
        _hip.check(status)

    def after_read(self) -> None:
        _hip.chain_check()  # a chained launch that had to be redone is reported where its result is read

    def streams_host_blocks(self) -> bool:
        return torch.cuda.is_available()


_MEM = HipMemory()


def _require_gpu() -> None:
    _MEM.require()


def _check(status: int) -> None:
    _MEM.check(status)


def is_device_array(x) -> bool:
    return isinstance(x, torch.Tensor) and _MEM.holds(x)


_FLOATS = (torch.float32, torch.float64)
# storage dtypes the library serves: float64 / float32 compute in their own dtype, float16 on float32 lanes (narrowed on
# the way out), integers / bool on int64 / int32 lanes (xgcm_amd.dtypes)
_SERVED = _dt.SERVED


# ---- where results are allocated ------------------------------------------------------------------------------------
# The rate of a kernel whose stores are spread over its whole output -- scans along Z or Y, marches, fills -- depends on
# the PHYSICAL layout of the output buffer: inside one contiguous physical block (what hipMalloc returns) cumsum Z of a
# 3600 x 2400 x 75 record runs 1.78 - 2.0 ms depending on which block the driver happened to pick, in a buffer backed by
# separately created 64 MiB physical allocations 1.67 ms, every time (tools/placement_probe.py).  Outputs
# of SCATTER_MIN_BYTES or more therefore come from a torch MemPool fed by the library's own allocator (xg_pool_alloc: HIP
# virtual memory management); torch still caches, reuses and stream-orders them.  XG_SCATTER_OUT=0 restores plain hipMalloc.
SCATTER_MIN_BYTES = 256 << 20
# ... and up to SCATTER_MAX_BYTES: a result of tens of GB (a whole batch of records in one array) spans many of the driver's
# physical blocks by itself -- config 4's 111 GB outputs ran at the good rate from plain allocations (0.78) -- and a second
# allocator cache of that size next to torch's own would not fit the HBM
SCATTER_MAX_BYTES = 16 << 30
_pool = None
_pool_state = {"enabled": None, "allocator": None}


def _scatter_pool():
    """the MemPool of scattered output buffers (created at first use), or None when switched off / not available"""
    global _pool
    if _pool_state["enabled"] is None:
        import os

        ok = os.environ.get("XG_SCATTER_OUT", "1") != "0" and hasattr(torch.cuda, "MemPool") and hasattr(torch.cuda, "use_mem_pool")
        if ok:
            try:
                from torch.cuda.memory import CUDAPluggableAllocator

                _hip.load()
                alloc = CUDAPluggableAllocator(_hip.LIB_PATH, "xg_pool_alloc", "xg_pool_free")
                _pool_state["allocator"] = alloc  # (kept alive with the pool)
                _pool = torch.cuda.MemPool(alloc.allocator(), use_on_oom=True)
            except Exception as exc:  # noqa: BLE001 -- an allocator torch cannot plug in is a lost optimisation, not an error
                import warnings

                warnings.warn(f"xgcm_amd: scattered output buffers are not available ({exc}); results use plain allocations")
                ok = False
        _pool_state["enabled"] = ok
    return _pool if _pool_state["enabled"] else None


def _empty(shape, dtype, device) -> torch.Tensor:
    """torch.empty for an operator's result; large results come from the scattered-buffer pool"""
    shape = tuple(int(v) for v in shape)
    n = 1
    for v in shape:
        n *= v
    dev = torch.device(device) if not isinstance(device, torch.device) else device
    if dev.type == "cuda" and SCATTER_MIN_BYTES <= n * torch.empty((), dtype=dtype).element_size() <= SCATTER_MAX_BYTES:
        pool = _scatter_pool()
        if pool is not None and not torch.cuda.is_current_stream_capturing():
            try:
                with torch.cuda.use_mem_pool(pool):
                    return torch.empty(shape, dtype=dtype, device=dev)
            except torch.OutOfMemoryError:
                # the pool's cache and torch's own do not lend each other their idle blocks: release both, once; if the
                # HBM is simply full the plain allocation below raises the error the caller should see
                torch.cuda.empty_cache()
                try:
                    with torch.cuda.use_mem_pool(pool):
                        return torch.empty(shape, dtype=dtype, device=dev)
                except torch.OutOfMemoryError:
                    pass
    return torch.empty(shape, dtype=dtype, device=dev)


def _raw_device(x) -> torch.Tensor:
    """numpy / host tensor -> contiguous tensor in HBM with its dtype UNCHANGED (PCIe copy of the raw bytes: an int8
    field crosses the bus as 1 byte per cell and is widened in HBM); device tensors pass.  An array of non-native byte
    order (`np.fromfile(f, ">f4")`, MDS / xmitgcm output -- the reference's numpy bodies take them as they are,
    xgcm/gridops.py:23-24,76-77) crosses as raw bytes too and is byte-swapped in HBM (xg_bswap): the tensor holds the
    VALUES in the native twin of the dtype, which is also what numpy returns.  complex / object / datetime arrays are
    refused with a TypeError (xgcm_amd.dtypes.check_served)."""
    _require_gpu()
    swap = 0
    from_host_array = not isinstance(x, torch.Tensor)
    if not from_host_array:
        t = x
        if t.dtype not in _dt._TORCH_TO_NUMPY:
            raise TypeError(f"array: dtype {t.dtype} is not supported by the MI355X backend")
    else:
        a, swap = _dt.host_intake(np.asarray(x, order="C"))
        if a.flags.writeable:
            t = torch.from_numpy(a)
        else:  # (a read-only memory map of a file: only ever READ here -- no copy, no warning)
            import warnings

            with warnings.catch_warnings():
                warnings.filterwarnings("ignore", message="The given NumPy array is not writable")
                t = torch.from_numpy(a)
    if from_host_array or not _MEM.holds(t):
        t = _MEM.place(t, private=bool(swap))
        if swap and t.numel():  # (a fresh private copy: swapped in place)
            _check(_MEM.lib().xg_bswap(t.data_ptr(), t.numel(), swap, _stream()))
    else:
        _MEM.check_current(t)
    return materialize(t)


def _copy_nd(src_ptr: int, src_strides: Sequence[int], dst: torch.Tensor, shape: Sequence[int]) -> None:
    """dst[...] = the strided source (xg_copy_nd): `dst` is an HBM tensor or view with positive strides, `src_ptr` the
    address of the source element with index 0, strides in elements (negative: flip, 0: broadcast)"""
    if len(shape) > _hip.MAX_NDIM:
        raise ValueError(f"strided copy of a {len(shape)}-d array (at most {_hip.MAX_NDIM} dims)")
    if dst.numel():
        _check(_MEM.lib().xg_copy_nd(src_ptr, _hip.i64(list(src_strides)), dst.data_ptr(), _hip.i64(list(dst.stride())),
                                          _hip.i64(list(shape)), len(shape), dst.element_size(), _stream()))


def materialize(t: torch.Tensor) -> torch.Tensor:
    """an HBM tensor as a C-contiguous one: transposed / expanded / sliced views are laid out by the library's strided
    copy (rows as 16-byte lanes, true transposes through LDS tiles), contiguous tensors pass"""
    if t.is_contiguous():
        return t
    if t.dim() > _hip.MAX_NDIM or t.element_size() not in (1, 2, 4, 8):
        return t.contiguous()  # (more dims / wider elements than xg_copy_nd takes: torch's copy, plumbing outside the hot path)
    out = _empty(t.shape, dtype=t.dtype, device=t.device)
    _copy_nd(t.data_ptr(), t.stride(), out, t.shape)
    return out


def flip(t, axes: Sequence[int]) -> torch.Tensor:
    """numpy.flip(t, axes) of an HBM tensor as a new contiguous tensor (one strided copy with negative source strides)"""
    t = _raw_device(t)
    axes = sorted({a % t.dim() for a in axes})
    strides = list(t.stride())
    off = 0
    for a in axes:
        if t.shape[a]:
            off += (t.shape[a] - 1) * strides[a]
        strides[a] = -strides[a]
    out = _empty(t.shape, dtype=t.dtype, device=t.device)
    _copy_nd(t.data_ptr() + off * t.element_size(), strides, out, t.shape)
    return out


def copy_into(dst: torch.Tensor, src) -> torch.Tensor:
    """dst[...] = src for an HBM destination VIEW (a slice of a larger tensor: concatenation without torch.cat); `src`
    must have dst's shape and dtype"""
    src = _raw_device(src)
    if tuple(src.shape) != tuple(dst.shape) or src.dtype != dst.dtype:
        raise ValueError(f"copy_into: source {tuple(src.shape)} {src.dtype} does not match destination {tuple(dst.shape)} {dst.dtype}")
    _sibling_written(dst)
    _copy_nd(src.data_ptr(), src.stride(), dst, dst.shape)
    return dst


def concatenate(parts: Sequence, axis: int) -> torch.Tensor:
    """numpy.concatenate of HBM tensors along `axis`: one strided copy per part into its slice of the result"""
    parts = [_raw_device(p) for p in parts]
    if len(parts) == 1:
        return parts[0]
    axis = axis % parts[0].dim()
    shape = list(parts[0].shape)
    shape[axis] = sum(int(p.shape[axis]) for p in parts)
    out = _empty(shape, dtype=parts[0].dtype, device=parts[0].device)
    at = 0
    for p in parts:
        copy_into(out.narrow(axis, at, p.shape[axis]), p)
        at += p.shape[axis]
    return out


def convert(x, dst, via=None, scale: float = 1.0, flip: bool = False) -> torch.Tensor:
    """numpy `astype` in HBM (xg_convert): `x` of any served dtype -> `dst` (numpy dtype); `via` / `scale` / `flip` as in
    include/xgcm_hip.h (the narrow dtype's wrap-around, interp's 0.5, uint64 order for the signed min / max kernels)."""
    lib = _MEM.lib()
    t = _raw_device(x)
    src, dst = _dt.np_dtype(t), np.dtype(dst)
    if t.dtype == torch.bfloat16:
        # no numpy twin and xg_convert does not read it: torch's cast to its float32 promotion (storage plumbing, outside
        # the hot path)
        t, src = t.to(torch.float32), _dt.FLOAT32
    if src == dst and via is None and scale == 1.0 and not flip:
        return t
    out = _empty(t.shape, dtype=_dt.torch_dtype(dst), device=t.device)
    if out.numel():
        _check(lib.xg_convert(t.data_ptr(), _hip.DTYPE[src.name], out.data_ptr(), _hip.DTYPE[dst.name], t.numel(),
                                  -1 if via is None else _hip.DTYPE[np.dtype(via).name], float(scale), 1 if flip else 0,
                                  _stream()))
    return out


def asdevice(x, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """numpy / host tensor -> contiguous tensor in HBM (PCIe copy); device tensors pass.

    Without `dtype` the array keeps its dtype (in native byte order) -- float32 / float64 compute in their own dtype like
    numpy, float16 arrays are stored as they are and widened to float32 lanes by the operators, integer and bool arrays
    stay integral (the operators widen them to integer lanes themselves; xgcm_amd.dtypes); bfloat16 tensors become
    float32.  With `dtype` (a float dtype: the lanes a call computes on) the array is converted in HBM by xg_convert,
    numpy's `astype`."""
    t = _raw_device(x)
    if dtype is None:
        return t if t.dtype != torch.bfloat16 else convert(t, _dt.FLOAT32)
    return t if t.dtype == dtype else convert(t, _dt._TORCH_TO_NUMPY[dtype])


def _half(*arrays) -> bool:
    """numpy returns float16 for these operands (xgcm_amd.dtypes.half_result): narrow the float32-lane result"""
    return _dt.half_result(*[_dt.np_dtype(a) for a in arrays if a is not None])


def _out(res, half: bool):
    """a float32-lane result as numpy's float16 where numpy returns float16 (one rounding, xg_convert)"""
    if not half:
        return res
    if isinstance(res, tuple):
        return tuple(_out(r, True) for r in res)
    return convert(res, _dt.FLOAT16)


def _metric_steps(x, m_in, m_out):
    """(pre_mul, post_div) of xgcm_amd.dtypes.metric_steps for these operands"""
    return _dt.metric_steps(_dt.np_dtype(x), None if m_in is None else _dt.np_dtype(m_in),
                            None if m_out is None else _dt.np_dtype(m_out))


def _dtype_of(x) -> torch.dtype:
    """float lanes of one operand on its own: float32 stays, everything else computes in float64"""
    return torch.float32 if _dt.np_dtype(x) == _dt.FLOAT32 else torch.float64


def _is_int(x) -> bool:
    return x is not None and _dt.is_integer(_dt.np_dtype(x))


def _common(*arrays):
    """(dtype, ABI suffix) of the float lanes an array and its metrics share: numpy's promotion -- float32 only if it
    yields float32 (all float32, or float32 next to 8 / 16-bit integers), float64 otherwise."""
    return _lanes(tuple([_dt.np_dtype(a) for a in arrays if a is not None]))


@functools.lru_cache(maxsize=None)
def _lanes(present: tuple):
    """`_common` of these dtypes: every call asks, and few mixes ever occur"""
    return (torch.float32, "f32") if _dt.float_of(*present) == _dt.FLOAT32 else (torch.float64, "f64")


# ---- integer arrays: int64 / int32 lanes between a widening and a narrowing conversion (xgcm_amd.dtypes.lane_of) -------
_LANE_SFX = {"int64": "i64", "int32": "i32"}


def _widen(x, lane=_dt.INT64) -> torch.Tensor:
    """integer / bool array -> tensor of `lane` (int64 / int32) in HBM; an array that IS its lanes (int64 / uint64 on
    int64, int32 / uint32 on int32) passes as the same bits"""
    t = _raw_device(x)
    lane = np.dtype(lane)
    if _dt.same_bits(_dt.np_dtype(t), lane):
        return t if _dt.np_dtype(t) == lane else t.view(_dt.torch_dtype(lane))
    return convert(t, lane)


def _narrow(t: torch.Tensor, dst, via=None, scale: float = 1.0) -> torch.Tensor:
    """integer lanes -> the dtype numpy returns (wrap modulo 2^bits; float64 for interp)"""
    dst = np.dtype(dst)
    if via is None and scale == 1.0 and _dt.same_bits(dst, _dt.np_dtype(t)):
        return t if _dt.np_dtype(t) == dst else t.view(_dt.torch_dtype(dst))
    return convert(t, dst, via=via, scale=scale)


def _lane_int(value, lane=_dt.INT64) -> int:
    """a numpy integer / bool scalar as the two's-complement value the lanes hold (uint64 above 2^63 wraps)"""
    bits = 8 * np.dtype(lane).itemsize
    v = int(value) & ((1 << bits) - 1)
    return v - (1 << bits) if v >= (1 << (bits - 1)) else v


def _divide(res: torch.Tensor, m_out, as_dtype) -> torch.Tensor:
    """`result / m_out` after an integer operator: numpy promotes the integral result, then divides"""
    return res if m_out is None else binary("div", convert(res, as_dtype), m_out)


def tohost(t) -> np.ndarray:
    if _is_chunked(t):
        return t  # a chunked host array (xgcm_amd.chunked.BlockArray, dask ...) IS on the host; numpy.asarray assembles it
    if isinstance(t, torch.Tensor):
        a = t.detach().cpu().numpy()  # synchronises the producing stream
        _MEM.after_read()
        return a
    return np.asarray(t)


def _stream() -> int:
    return _MEM.stream()


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _bstrides(m: Optional[torch.Tensor], shape: Sequence[int], what: str):
    """Per-dim element strides of metric `m` against an array of `shape` (0 = broadcast)."""
    if m is None:
        return None
    if m.dim() != len(shape):
        raise ValueError(f"{what}: metric has {m.dim()} dims, array has {len(shape)}")
    st = []
    for d, (ms, s) in enumerate(zip(m.shape, shape)):
        if ms == s and s != 1:
            st.append(m.stride(d))
        elif ms == 1:
            st.append(0)
        else:
            raise ValueError(f"{what}: metric extent {ms} does not broadcast against {s} on dim {d}")
    return st


def _prep_metric(m, dtype) -> Optional[torch.Tensor]:
    return None if m is None else asdevice(m, dtype)


# ---- large HOST arrays: block-wise through HBM with the copies overlapped ------------------------------------
# numpy in -> numpy out is the reference's normal case.  One synchronous pageable H2D, the kernel and one
# synchronous D2H move a 1.4 GB field at ~8 GB/s; cutting it into blocks of the outermost dim (never the operator's
# own axis here) and running them through xgcm_amd.streaming -- host memory page-locked in place, H2D of block k+1,
# the kernel on block k and D2H of block k-1 on three HIP streams -- reaches ~40 GB/s each way (the link: 48.6).
HOST_STREAM_MIN_BYTES = 256 << 20   # host arrays at least this large take the pipelined path
# one block: a sixth of the array, between 64 MB and 2 GB.  Every block costs hand-offs between the threads and streams of
# the pipeline and its own page-locking call, the first and the last block travel alone: a 5.2 GB record into a fresh
# result array in 75 / 25 / 13 / 6 blocks: 0.19 / 0.19 / 0.19 / 0.14 s = 38 GB/s each way (into a reused, touched array:
# 0.19 s in 75 blocks, 0.13 s in 19 or 5; tools/pcie_probe.py)
HOST_STREAM_BLOCK_BYTES = (64 << 20, 2 << 30)


def _host_streamable(x, axis: int) -> bool:
    # (float32 / float64 in either byte order: the streamer moves raw bytes and swaps big-endian blocks in HBM)
    return (isinstance(x, np.ndarray) and x.ndim >= 2 and axis % x.ndim != 0 and x.shape[0] >= 2
            and _dt.native(x.dtype) in (_dt.FLOAT32, _dt.FLOAT64) and x.nbytes >= HOST_STREAM_MIN_BYTES
            and _MEM.streams_host_blocks())


def _rows(m, sl, ndim: int, what: str = "metric"):
    """rows `sl` of a dim-aligned metric along the outermost dim (a metric broadcast there passes whole)"""
    if m is None:
        return None
    if len(m.shape) != ndim:  # the check _bstrides makes for HBM inputs, before any slicing along dim 0
        raise ValueError(f"{what}: metric has {len(m.shape)} dims, array has {ndim}")
    return m if m.shape[0] == 1 else m[sl]


def _streamed(per_block, x: np.ndarray) -> np.ndarray:
    """`per_block(block_tensor, rows_slice) -> HBM tensor` over consecutive blocks of the outermost dim of `x`"""
    from .streaming import record_blocks, stream_records

    x = np.ascontiguousarray(x)
    lo, hi = HOST_STREAM_BLOCK_BYTES if isinstance(HOST_STREAM_BLOCK_BYTES, tuple) else (HOST_STREAM_BLOCK_BYTES,) * 2
    target = min(max(x.nbytes // 6, lo), hi)
    block = max(1, int(target // max(1, x.nbytes // x.shape[0])))
    spans = iter(record_blocks(x.shape[0], block))

    def on_block(t):
        a, b = next(spans)
        return per_block(t, slice(a, b))

    return stream_records(on_block, x, block=block)


# ---- chunked HOST arrays (dask / zarr / xgcm_amd.chunked.BlockArray): block by block through HBM -------------------------
# The reference walks the chunks of a dask-backed field with `apply_ufunc(dask="parallelized")` over the broadcast dims and
# `map_overlap` along a chunked core dim (xgcm/grid.py:786-818, xgcm/grid_ufunc.py:1057-1133).  Here a block of the NON-core
# dims -- whole along the operator's own axis: chunks along it are read together, which is what map_overlap's halo exchange
# computes -- is one ordinary call of this module; with a GPU the blocks go through `streaming.iter_stream` (the next block is
# read and copied in while this one is computed and the previous result is copied out).  The result keeps the input's
# chunking (along the operator's axis too when its length did not change) and is never concatenated on the host.
def _is_chunked(x) -> bool:
    from . import chunked as _ch

    return _ch.is_chunked(x)


def _block_of(m, sl, axis: Optional[int], ndim: int, what: str = "metric"):
    """the part of a dim-aligned metric that belongs to block `sl` of the array (a dim the metric broadcasts along, and the
    operator's own axis, pass whole); a chunked metric is read for just that part"""
    if m is None:
        return None
    if len(m.shape) != ndim:
        raise ValueError(f"{what}: metric has {len(m.shape)} dims, array has {ndim}")
    key = tuple(slice(None) if (d == axis or m.shape[d] == 1) else sl[d] for d in range(ndim))
    return np.asarray(m[key]) if _is_chunked(m) else m[key]


def _blockwise(per_block, x, axis: Optional[int], n_out: Optional[int] = None, drop_axis: bool = False, lead: int = 0):
    """`per_block(host block, slices) -> result` for every block of the chunked host array `x`, blocks whole along `axis`
    (None: every dim split).  `n_out`: length of the result along `axis`; `drop_axis`: the result has no such dim (sums);
    `lead`: a leading dim of that length the result gains (the stacked numerator / denominator of the pair modes)."""
    from . import chunked as _ch

    chunks = _ch.normalize_chunks(x.chunks, x.shape)
    nd = len(chunks)
    if axis is not None:
        axis %= nd
    todo = list(_ch.block_slices(chunks, whole=() if axis is None else (axis,)))
    blocks = {}
    src_dt = _dt.native(np.dtype(x.dtype))
    if _MEM.streams_host_blocks() and len(todo) > 1 and src_dt in (_dt.FLOAT32, _dt.FLOAT64):
        from .streaming import iter_stream

        at = [0]

        def on_block(t):  # (called once per block, in order)
            _, sl = todo[at[0]]
            at[0] += 1
            return asdevice(per_block(t, sl))

        for (idx, _), res in zip(todo, iter_stream(on_block, _ch.read_ahead(x, [sl for _, sl in todo]))):
            blocks[idx] = res
    else:
        for (idx, sl), blk in zip(todo, _ch.read_ahead(x, [sl for _, sl in todo])):
            blocks[idx] = tohost(per_block(blk, sl))
    dtype = next(iter(blocks.values())).dtype if blocks else x.dtype
    if drop_axis:
        blocks = {idx[:axis] + idx[axis + 1:]: b for idx, b in blocks.items()}
        chunks = chunks[:axis] + chunks[axis + 1:]
    elif axis is not None:
        if n_out == sum(chunks[axis]) and len(chunks[axis]) > 1:
            blocks, chunks = _ch.rechunk_blocks(blocks, chunks, axis, chunks[axis])  # the axis keeps the input's chunks
        else:
            chunks = chunks[:axis] + ((int(n_out),),) + chunks[axis + 1:]
    if lead:
        blocks = {(0,) + idx: b for idx, b in blocks.items()}
        chunks = ((int(lead),),) + chunks
    return _ch.BlockArray(blocks, chunks, dtype)


def _int_stencil1d(plan, op: str, x, halo, axis: int, pad_lo: int, pad_hi: int, bc: Optional[str], fill, m_out):
    """diff / interp / min / max of an integer or bool array on integer lanes (xg_stencil1d_i64 / _i32 and their _halo
    twins), returned in the dtype numpy returns: the array's own for diff / min / max (wrap-around included), float64 for
    interp -- the sum wraps in the array's dtype first, `(a[:-1] + a[1:]) / 2.0` -- and `result / m_out` promoted like
    numpy when an output metric divides (xgcm_amd.dtypes.stencil_plan)."""
    lib = _MEM.lib()
    src = _dt.np_dtype(x)
    lane, sfx = plan.compute, _LANE_SFX[plan.compute.name]
    t = _widen(x, lane)
    axis = axis % t.dim()
    shape = list(t.shape)
    n_out = shape[axis] + pad_lo + pad_hi - 1
    oshape = list(shape)
    oshape[axis] = n_out
    out = _empty(oshape, dtype=_dt.torch_dtype(lane), device=t.device)
    code = _hip.OP[op + "u"] if plan.unsigned else _hip.OP[op]
    if out.numel():
        if halo is not None:
            h = _widen(halo if _dt.np_dtype(halo) == src else convert(halo, src), lane)
            _check(getattr(lib, "xg_stencil1d_halo_" + sfx)(
                code, t.data_ptr(), h.data_ptr() if h.numel() else None, out.data_ptr(), _hip.i64(shape), len(shape),
                axis, n_out, int(pad_lo), int(pad_hi), None, None, _stream()))
        else:
            # numpy.pad casts the constant to the array's dtype (xgcm/padding.py:610-615)
            fv = _lane_int(_dt.fill_as(src, fill), lane) if (bc == "fill" and (pad_lo or pad_hi)) else 0
            _check(getattr(lib, "xg_stencil1d_" + sfx)(
                code, t.data_ptr(), out.data_ptr(), _hip.i64(shape), len(shape), axis, n_out, int(pad_lo),
                int(pad_hi), _hip.BC[bc], fv, None, None, None, None, _stream()))
    res = _narrow(out, plan.result, via=plan.via, scale=plan.scale)
    return _divide(res, m_out, plan.divide_as)


# ---- learned sibling plans: the plain two-point operators a caller asks of one field, round after round, in ONE pass ------
# Model code asks the same operators of the same kind of field every step: interp and diff along X, then along Y -- four
# passes that each read the whole field.  An eager call cannot know what comes next, but it can remember: per thread and
# per KIND of input (device, stream, dtype, shape, strides -- not the tensor: every step brings a new one) the requests
# are logged in rounds, a round ending when its first request comes again.  Two equal rounds of 2 to 4 different requests
# make a plan; from then on the round's first request runs xg_stencil_multi for the whole set (one read of the field), and the
# other results wait -- held against THAT tensor's identity and version -- until they are asked for.  Only the pattern is
# remembered, never a value: every round is computed from the tensor it is asked of.  The first deviation (another tensor in
# mid round, a changed `_version`, a request outside the set) drops what is held and retires the plan; the call then runs
# as it always did, and learning starts over.  XG_SIBLING_PLAN=0 switches all of it off.
SIBLING_MAX_KEYS = 8  # kinds of input remembered per thread, least recently used evicted
SIBLING_MAX_SET = 4   # results of one pass (xg_stencil_multi)


class _Counters:
    """one-pass launches, results served from a held set, held results dropped unused, plans retired -- of ONE thread"""

    __slots__ = ("launches", "served", "dropped", "retired")

    def __init__(self):
        self.launches = self.served = self.dropped = self.retired = 0


_SIB = threading.local()  # .table: OrderedDict field key -> _Siblings; .off: depth of sibling_plans_off(); .stats: _Counters


def _stats() -> _Counters:
    c = getattr(_SIB, "stats", None)
    if c is None:
        c = _SIB.stats = _Counters()
    return c


class _SiblingStats:
    """`device.SIBLING_STATS`: the calling thread's counters (each thread has its own table and its own counts)"""

    def reset(self) -> None:
        _SIB.stats = _Counters()

    def __getitem__(self, name: str) -> int:
        return self.as_dict()[name]

    def as_dict(self) -> dict:
        c = _stats()
        return {"launches": c.launches, "served": c.served, "dropped": c.dropped, "retired": c.retired}


SIBLING_STATS = _SiblingStats()


class _Siblings:
    """what one thread has learnt about, and holds for, one kind of input"""

    __slots__ = ("log", "first", "last", "plan", "held", "ref", "ident", "declined", "stats")

    def __init__(self):
        self.stats = _stats()  # the OWNER's counters: the weak-reference callback may run on whichever thread frees the input
        self.log, self.last, self.plan = [], None, None  # this round so far, the last complete round, the live plan
        self.first = None                                   # weak reference to the tensor this round is asked of
        self.held, self.ref, self.ident = None, None, None  # request -> result, weak reference and identity of their input
        self.declined = False                               # the native entry refused this kind once: not asked again

    def held_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.held or {}).values())

    def drop(self) -> None:
        if self.held:
            self.stats.dropped += len(self.held)
        self.held = self.ref = self.ident = None

    def forget(self) -> None:
        """drop what is held, retire a live plan, learn from scratch"""
        self.drop()
        if self.plan is not None:
            self.stats.retired += 1
        self.log, self.first, self.last, self.plan = [], None, None, None


def _sib_table() -> OrderedDict:
    table = getattr(_SIB, "table", None)
    if table is None:
        table = _SIB.table = OrderedDict()
    return table


def drop_sibling_plans() -> None:
    """forget every plan of the calling thread and release the results it holds"""
    table = _sib_table()
    for st in table.values():
        st.forget()
    table.clear()


@contextlib.contextmanager
def sibling_plans_off():
    """inside, the calling thread neither learns nor serves: for callers with exact knowledge of what is needed (the deferred
    results of `grid.fused()` have their own sibling rules)"""
    _SIB.off = getattr(_SIB, "off", 0) + 1
    try:
        yield
    finally:
        _SIB.off -= 1


def _free_bytes() -> int:
    """free memory where the results live (HBM: torch.cuda.mem_get_info)"""
    if _MEM.device == "cuda":
        return int(torch.cuda.mem_get_info()[0])
    return int(os.sysconf("SC_AVPHYS_PAGES")) * int(os.sysconf("SC_PAGE_SIZE"))


def _sibling_identity(x: torch.Tensor):
    return (x.data_ptr(), x.untyped_storage().data_ptr(), x._version, _stream())


def _sibling_enabled() -> bool:
    if os.environ.get("XG_SIBLING_PLAN", "1") == "0" or getattr(_SIB, "off", 0) > 0:
        return False
    from . import lazy as _lazy

    if getattr(_lazy._ACTIVE, "depth", 0) > 0:  # inside `with grid.fused():`
        return False
    # a capture must record every kernel it is given: nothing learnt before it is served or held across its start
    return not (_MEM.device == "cuda" and torch.cuda.is_current_stream_capturing())


def _multi_launch(x: torch.Tensor, requests):
    """xg_stencil_multi: one result per (op, axis, pad_lo, pad_hi, bc, fill) of the resident float tensor `x`, all from one
    read of it; None when the native entry declines (nothing was launched)"""
    n = len(requests)
    outs = [_empty(x.shape, x.dtype, x.device) for _ in range(n)]
    desc = (_hip.MultiDesc * n)()
    for d, (op, axis, pad_lo, pad_hi, bc, fill), out in zip(desc, requests, outs):
        d.op, d.axis, d.pad_lo, d.pad_hi, d.bc, d.fill, d.out = (_hip.OP[op], axis % x.dim(), pad_lo, pad_hi, _hip.BC[bc], float(fill),
                                                                  out.data_ptr())
    status = _MEM.lib().xg_stencil_multi(_hip.DTYPE[_dt.np_dtype(x).name], x.data_ptr(), _hip.i64(list(x.shape)), x.dim(), n,
                                         desc, _stream())
    if status == _hip.DECLINED:
        return None
    _check(status)
    return outs


SIBLING_MAX_CELLS = 2 ** 31 - 1  # xg_stencil_multi declines 2^31 cells or more


def _sibling_form(x, axis: int, pad_lo: int, pad_hi: int, bc) -> bool:
    """is this a plain operator in a form xg_stencil_multi takes (include/xgcm_hip.h)?  Only such calls are requests."""
    return (2 <= x.dim() <= 3 and axis >= x.dim() - 2 and (pad_lo, pad_hi) in ((1, 0), (0, 1)) and bc in ("periodic", "fill", "extend")
            and x.is_contiguous() and 0 < x.numel() <= SIBLING_MAX_CELLS and (x.shape[-1] * x.element_size()) % 16 == 0
            and x.data_ptr() % 16 == 0)


def _sibling_written(t) -> None:
    """the library itself is about to write into `t` through its address, which `_version` does not see: results held for a
    tensor of that storage are dropped"""
    if isinstance(t, torch.Tensor) and getattr(_SIB, "table", None):
        base = t.untyped_storage().data_ptr()
        for st in _SIB.table.values():
            if st.held is not None and st.ident[1] == base:
                st.forget()


def _sibling_launch(st: _Siblings, x: torch.Tensor, req) -> Optional[torch.Tensor]:
    """the whole set of the live plan from one read of `x`; None: not this time (memory, or the native entry declines)"""
    n = len(st.plan)
    each = x.numel() * x.element_size()
    held_elsewhere = sum(s.held_bytes() for s in _sib_table().values() if s is not st)
    if held_elsewhere + (n - 1) * each >= _free_bytes() // 4:
        return None
    outs = _multi_launch(x, [r[:5] + (float(np.uint64(r[5]).view(np.float64)),) for r in st.plan])  # (requests carry the fill's bits)
    if outs is None:
        st.declined = True
        return None
    st.stats.launches += 1
    results = dict(zip(st.plan, outs))
    first = results.pop(req)
    st.held, st.ident = results, _sibling_identity(x)
    st.ref = weakref.ref(x, lambda _r, st=st: st.drop())  # the input dies: so do the results nobody asked for
    return first


def _sibling_stencil(op: str, x: torch.Tensor, axis: int, pad_lo: int, pad_hi: int, bc: str, fill: float) -> Optional[torch.Tensor]:
    """one eligible `stencil1d` request passes here: its result when a learnt plan serves it, else None (and the caller
    runs the single-operator kernel as ever) -- either way the request is part of what is learnt"""
    if not _sibling_enabled():
        if getattr(_SIB, "table", None):
            drop_sibling_plans()
        return None
    # (the fill keeps its bits -- -0.0 is not 0.0, NaN is itself -- so requests compare by them)
    req = (op, axis, pad_lo, pad_hi, bc, np.float64(fill).view(np.uint64).item() if bc == "fill" else 0)
    key = (str(x.device), _stream(), x.dtype, tuple(x.shape), tuple(x.stride()))
    table = _sib_table()
    st = table.get(key)
    if st is None:
        st = table[key] = _Siblings()
        while len(table) > SIBLING_MAX_KEYS:
            table.popitem(last=False)[1].forget()
    table.move_to_end(key)
    if st.held is not None:
        if st.ref() is x and st.ident == _sibling_identity(x) and req in st.held:
            out = st.held.pop(req)
            st.stats.served += 1
            if not st.held:
                st.held = st.ref = st.ident = None
            st.log.append(req)
            return out
        st.forget()  # another tensor in mid round, new values in this one, a request outside the set
    if st.plan is not None and req not in st.plan:
        st.forget()  # (the same with nothing held any more)
    if st.log and req != st.log[0] and (st.first is None or st.first() is not x):
        st.forget()  # a round is what is asked of ONE tensor: two fields of one kind taking turns (diff(v, X) - diff(u, Y)) make no plan
    if st.log and req == st.log[0]:  # the round is complete
        done = frozenset(st.log)
        valid = 2 <= len(st.log) <= SIBLING_MAX_SET and len(done) == len(st.log)
        if valid and done == st.last:
            if st.plan is None or frozenset(st.plan) != done:
                st.plan = tuple(st.log)
        elif st.plan is not None:
            st.plan = None
            st.stats.retired += 1
        st.last, st.log = (done if valid else None), []
    elif len(st.log) >= SIBLING_MAX_SET:  # a fifth request before the first came again: no round of this kind makes a plan
        st.forget()
    st.log.append(req)
    if len(st.log) == 1:
        st.first = weakref.ref(x)
    if st.plan is not None and len(st.log) == 1 and req == st.plan[0] and not st.declined:
        return _sibling_launch(st, x, req)
    return None


def stencil1d(op: str, x, axis: int, pad_lo: int, pad_hi: int, bc: Optional[str], fill: float = 0.0,
              m_in=None, m_out=None) -> torch.Tensor:
    """Fused pad + diff/interp/min/max along `axis` (xg_stencil1d_f64)."""
    lib = _MEM.lib()
    if _is_chunked(x):  # a dask-style chunked host array: block by block, whole along `axis` (xgcm/grid.py:786-818)
        ax, nd = axis % x.ndim, x.ndim
        return _blockwise(lambda blk, sl: stencil1d(op, blk, ax, pad_lo, pad_hi, bc, fill, _block_of(m_in, sl, ax, nd, "m_in"),
                                                    _block_of(m_out, sl, ax, nd, "m_out")), x, ax, x.shape[ax] + pad_lo + pad_hi - 1)
    if _host_streamable(x, axis):  # a large host array: blocks of the outermost dim, copies overlapped with the kernel
        return _streamed(lambda blk, sl: stencil1d(op, blk, axis, pad_lo, pad_hi, bc, fill, _rows(m_in, sl, x.ndim, 'm_in'), _rows(m_out, sl, x.ndim, 'm_out')), x)
    plan = _dt.stencil_plan(op, _dt.np_dtype(x), None if m_in is None else _dt.np_dtype(m_in),
                            None if m_out is None else _dt.np_dtype(m_out))
    if plan.lanes == "int":
        return _int_stencil1d(plan, op, x, None, axis, pad_lo, pad_hi, bc, fill, m_out)
    pre_mul, post_div = _metric_steps(x, m_in, m_out)
    if pre_mul:  # a float16 product: rounded to float16 before the body sees it
        x, m_in = binary("mul", x, m_in), None
    if post_div:  # the body's result is rounded to ITS dtype before the (wider, or float16) division
        return binary("div", stencil1d(op, x, axis, pad_lo, pad_hi, bc, fill, m_in, None), m_out)
    half = _half(x, m_in, m_out)
    dt, sfx = _common(x, m_in, m_out)
    given = x
    x = asdevice(x, dt)
    axis = axis % x.dim()
    if x is given and m_in is None and m_out is None and not half and _sibling_form(x, axis, pad_lo, pad_hi, bc):
        # a plain operator on a resident field, in a form xg_stencil_multi takes: the learned sibling plan may have it ready
        served = _sibling_stencil(op, x, axis, int(pad_lo), int(pad_hi), bc, float(fill))
        if served is not None:
            return served
    shape = list(x.shape)
    n_out = shape[axis] + pad_lo + pad_hi - 1
    oshape = list(shape)
    oshape[axis] = n_out
    m_in = _prep_metric(m_in, dt)
    m_out = _prep_metric(m_out, dt)
    out = _empty(oshape, dtype=dt, device=x.device)
    if out.numel() == 0:  # empty outer dims: nothing to launch (a NULL data_ptr is not a valid ABI argument)
        return _out(out, half)
    _check(
        getattr(lib, "xg_stencil1d_" + sfx)(
            _hip.OP[op], x.data_ptr(), out.data_ptr(), _hip.i64(shape), len(shape), axis, n_out,
            int(pad_lo), int(pad_hi), _hip.BC[bc], float(fill),
            _ptr(m_in), _hip.i64(_bstrides(m_in, shape, "m_in")),
            _ptr(m_out), _hip.i64(_bstrides(m_out, oshape, "m_out")), _stream(),
        )
    )
    return _out(out, half)


def stencil1d_halo(op: str, x, halo, axis: int, pad_lo: int, pad_hi: int, m_out=None, m_in=None) -> torch.Tensor:
    """diff / interp / min / max along `axis` with pre-gathered halo cells (xg_stencil1d_halo_f64):
    `halo` is shaped like `x` with `axis` shortened to pad_lo + pad_hi, low halo first.  With an input metric `m_in`
    (xg_stencil1d_halo_w_f64) the field is weighted inside the kernel and `halo` holds the halo cells of the PRODUCT
    x * m_in (gathered as gather(x) * gather(m_in)), which are not weighted again."""
    lib = _MEM.lib()
    expect = list(x.shape)
    expect[axis % len(expect)] = pad_lo + pad_hi
    if list(halo.shape) != expect:
        raise ValueError(f"halo buffer has shape {tuple(halo.shape)}, expected {tuple(expect)}")
    if _is_int(x) and _is_int(halo) and m_in is None:
        plan = _dt.stencil_plan(op, _dt.np_dtype(x), None, None if m_out is None else _dt.np_dtype(m_out))
        return _int_stencil1d(plan, op, x, halo, axis, pad_lo, pad_hi, "halo", 0, m_out)
    pre_mul, post_div = _metric_steps(x, m_in, m_out)
    if pre_mul:  # float16: the product (and, by the caller's contract, the halo of the product) is float16 already
        x, m_in = binary("mul", x, m_in), None
    if post_div:
        return binary("div", stencil1d_halo(op, x, halo, axis, pad_lo, pad_hi, None, m_in), m_out)
    half = _half(x, halo, m_out, m_in)
    dt, sfx = _common(x, halo, m_out, m_in)
    x = asdevice(x, dt)
    halo = asdevice(halo, dt)
    axis = axis % x.dim()
    n = x.shape[axis]
    n_out = n + pad_lo + pad_hi - 1
    oshape = list(x.shape)
    oshape[axis] = n_out
    out = _empty(oshape, dtype=dt, device=x.device)
    if out.numel() == 0:
        return _out(out, half)
    m_out = _prep_metric(m_out, dt)
    if m_in is not None:
        m_in = _prep_metric(m_in, dt)
        _check(
            getattr(lib, "xg_stencil1d_halo_w_" + sfx)(
                _hip.OP[op], x.data_ptr(), halo.data_ptr() if halo.numel() else None, out.data_ptr(),
                _hip.i64(list(x.shape)), x.dim(), axis, n_out, int(pad_lo), int(pad_hi), _ptr(m_in),
                _hip.i64(_bstrides(m_in, list(x.shape), "m_in")), _ptr(m_out), _hip.i64(_bstrides(m_out, oshape, "m_out")),
                _stream())
        )
        return _out(out, half)
    _check(
        getattr(lib, "xg_stencil1d_halo_" + sfx)(
            _hip.OP[op], x.data_ptr(), halo.data_ptr() if halo.numel() else None, out.data_ptr(),
            _hip.i64(list(x.shape)), x.dim(), axis, n_out, int(pad_lo), int(pad_hi), _ptr(m_out),
            _hip.i64(_bstrides(m_out, oshape, "m_out")), _stream())
    )
    return _out(out, half)


def _int_cumsum1d(x, axis: int, trim_lo: int, trim_hi: int, pad_lo: int, pad_hi: int, bc: Optional[str], fill,
                  reverse: bool, m_out):
    """prefix sum of an integer / bool array on int64 lanes (xg_cumsum1d_i64): numpy.cumsum accumulates 8 / 16 / 32-bit
    integers and bool in the platform integer, so the result is int64 (uint64 for unsigned), exact modulo 2^64; the halo
    of the padded cumulative result takes the fill value cast to THAT dtype (numpy.pad on the cumsum'ed array)."""
    lib = _MEM.lib()
    res_dt = _dt.cumsum_dtype(_dt.np_dtype(x))
    t = _widen(x)
    axis = axis % t.dim()
    shape = list(t.shape)
    oshape = list(shape)
    oshape[axis] = shape[axis] - trim_lo - trim_hi + pad_lo + pad_hi
    fv = _lane_int(_dt.fill_as(res_dt, fill)) if (bc == "fill" and (pad_lo or pad_hi)) else 0
    if min(oshape) > 0 and shape[axis] - trim_lo - trim_hi == 0:
        if bc != "fill":
            raise ValueError(f"can't extend empty axis {axis} using modes other than 'constant' or 'empty'")
        out = torch.from_numpy(np.full(oshape, fv, dtype=np.int64)).to(t.device)  # only halo cells remain
    else:
        out = _empty(oshape, dtype=torch.int64, device=t.device)
        if out.numel():
            _check(lib.xg_cumsum1d_i64(
                t.data_ptr(), out.data_ptr(), _hip.i64(shape), len(shape), axis, int(bool(reverse)), 0, int(trim_lo),
                int(trim_hi), int(pad_lo), int(pad_hi), _hip.BC[bc], fv, None, None, None, None, _stream()))
    return _divide(_narrow(out, res_dt), m_out, None if m_out is None else _dt.float_of(res_dt, _dt.np_dtype(m_out)))


def cumsum1d(x, axis: int, trim_lo: int, trim_hi: int, pad_lo: int, pad_hi: int, bc: Optional[str],
             fill: float = 0.0, reverse: bool = False, skipna: bool = True, m_in=None, m_out=None) -> torch.Tensor:
    """Prefix sum along `axis` with the Grid.cumsum trim/pad folded in (xg_cumsum1d_f64)."""
    lib = _MEM.lib()
    if _is_chunked(x):  # chunks along `axis` are scanned together (the reference: "it would need blockwise", grid.py:1305)
        ax, nd = axis % x.ndim, x.ndim
        return _blockwise(lambda blk, sl: cumsum1d(blk, ax, trim_lo, trim_hi, pad_lo, pad_hi, bc, fill, reverse, skipna,
                                                   _block_of(m_in, sl, ax, nd, "m_in"), _block_of(m_out, sl, ax, nd, "m_out")),
                          x, ax, x.shape[ax] - trim_lo - trim_hi + pad_lo + pad_hi)
    if _host_streamable(x, axis):
        return _streamed(lambda blk, sl: cumsum1d(blk, axis, trim_lo, trim_hi, pad_lo, pad_hi, bc, fill, reverse, skipna,
                                                  _rows(m_in, sl, x.ndim, 'm_in'), _rows(m_out, sl, x.ndim, 'm_out')), x)
    if _is_int(x) and m_in is None:
        return _int_cumsum1d(x, axis, trim_lo, trim_hi, pad_lo, pad_hi, bc, fill, reverse, m_out)
    pre_mul, post_div = _metric_steps(x, m_in, m_out)
    if pre_mul:
        x, m_in = binary("mul", x, m_in), None
    if post_div:
        return binary("div", cumsum1d(x, axis, trim_lo, trim_hi, pad_lo, pad_hi, bc, fill, reverse, skipna, m_in, None), m_out)
    half = _half(x, m_in, m_out)
    dt, sfx = _common(x, m_in, m_out)
    x = asdevice(x, dt)
    axis = axis % x.dim()
    shape = list(x.shape)
    oshape = list(shape)
    oshape[axis] = shape[axis] - trim_lo - trim_hi + pad_lo + pad_hi
    m_in = _prep_metric(m_in, dt)
    m_out = _prep_metric(m_out, dt)
    out = _empty(oshape, dtype=dt, device=x.device)
    if out.numel() == 0:
        return _out(out, half)
    if shape[axis] - trim_lo - trim_hi == 0:
        # everything trimmed away: only halo cells remain.  numpy.pad can fill an empty axis with a
        # constant but refuses to wrap/extend it -- same here.
        if bc != "fill":
            raise ValueError(f"can't extend empty axis {axis} using modes other than 'constant' or 'empty'")
        synthetic(tuple(oshape), 0, 0, 0.0, float(fill), out=out)
        return _out(out if m_out is None else binary("div", out, m_out), half)
    _check(
        getattr(lib, "xg_cumsum1d_" + sfx)(
            x.data_ptr(), out.data_ptr(), _hip.i64(shape), len(shape), axis, int(bool(reverse)), int(bool(skipna)),
            int(trim_lo), int(trim_hi), int(pad_lo), int(pad_hi), _hip.BC[bc], float(fill),
            _ptr(m_in), _hip.i64(_bstrides(m_in, shape, "m_in")),
            _ptr(m_out), _hip.i64(_bstrides(m_out, oshape, "m_out")), _stream(),
        )
    )
    return _out(out, half)


_REDUCE_MODE = {"valid": 2, "all": 3, "mean_valid": 4, "mean_all": 5, "pair_valid": 6, "pair_all": 7}


def reduce1d(x, axis: int, w=None, skipna=True) -> torch.Tensor:
    """sum_k (x * w) along `axis`, axis removed (xg_reduce1d_f64).  `skipna` True / False, or the count modes
    "valid" (sum of the weights of the non-NaN cells of x) / "all" (sum of the weights), or the weighted mean in
    ONE pass over x: "mean_valid" = sum(x * w | valid) / sum(w | valid), "mean_all" = sum(x * w) / sum(w);
    "pair_valid" / "pair_all" return those two sums stacked along a new leading dim of 2 (means over several dims)."""
    lib = _MEM.lib()
    if _is_chunked(x):
        ax, nd = axis % x.ndim, x.ndim
        return _blockwise(lambda blk, sl: reduce1d(blk, ax, _block_of(w, sl, ax, nd, "w"), skipna), x, ax, drop_axis=True,
                          lead=2 if skipna in ("pair_valid", "pair_all") else 0)
    if _host_streamable(x, axis) and skipna not in ("pair_valid", "pair_all"):
        return _streamed(lambda blk, sl: reduce1d(blk, axis, _rows(w, sl, x.ndim, 'w'), skipna), x)
    if _is_int(x) and w is None and isinstance(skipna, (bool, int, np.bool_)):
        # numpy.sum of integers: accumulated in the platform integer, exact modulo 2^64 (xg_reduce1d_i64)
        res_dt = _dt.cumsum_dtype(_dt.np_dtype(x))
        t = _widen(x)
        axis = axis % t.dim()
        shape = list(t.shape)
        out = torch.zeros(shape[:axis] + shape[axis + 1:], dtype=torch.int64, device=t.device) if t.numel() == 0 else \
            _empty(shape[:axis] + shape[axis + 1:], dtype=torch.int64, device=t.device)
        if out.numel() and t.numel():
            _check(lib.xg_reduce1d_i64(t.data_ptr(), out.data_ptr(), _hip.i64(shape), len(shape), axis, 0, None, None,
                                           _stream()))
        return _narrow(out, res_dt)
    half = _half(x, w)
    if half and w is not None and skipna in _REDUCE_MODE and skipna not in ("valid", "all"):
        # float16 weighted MEAN / PAIR modes: numpy rounds the product x * w to float16 before it is summed, the
        # denominator is the sum of the WEIGHTS (of the valid cells) -- two passes, as `(x * w).sum() / w.where(valid).sum()` is:
        # folding the weight into the field would leave the kernel a plain count for its denominator
        valid = skipna.endswith("_valid")
        num = reduce1d(binary("mul", x, w), axis, None, valid)
        den = reduce1d(x, axis, w, "valid" if valid else "all")
        if skipna.startswith("pair"):
            return torch.stack([asdevice(num), asdevice(den)])
        return binary("div", num, den)
    if half and w is not None and skipna not in ("valid", "all"):  # plain sums: the float16 product is rounded before it is summed
        x, w = binary("mul", x, w), None
    dt, sfx = _common(x, w)
    x = asdevice(x, dt)
    axis = axis % x.dim()
    shape = list(x.shape)
    oshape = shape[:axis] + shape[axis + 1:]
    if skipna in ("pair_valid", "pair_all"):  # numerator and denominator sums side by side: a leading dim of 2
        oshape = [2] + oshape
    w = _prep_metric(w, dt)
    out = _empty(oshape, dtype=dt, device=x.device)
    if out.numel() == 0:
        return _out(out, half)
    if x.numel() == 0:  # sum over an empty axis is 0
        return _out(synthetic(tuple(oshape), 0, 0, 0.0, 0.0, out=out), half)
    _check(
        getattr(lib, "xg_reduce1d_" + sfx)(
            x.data_ptr(), out.data_ptr(), _hip.i64(shape), len(shape), axis, _REDUCE_MODE.get(skipna, int(bool(skipna))),
            _ptr(w), _hip.i64(_bstrides(w, shape, "w")), _stream(),
        )
    )
    return _out(out, half)


def pad_nd(x, widths: dict, bc: dict, fill: dict) -> torch.Tensor:
    """Generic pad; dict keys are axis numbers, dict order is the application order (xg_pad_f64)."""
    lib = _MEM.lib()
    src = _dt.np_dtype(x)
    ints = _dt.is_integer(src)  # numpy.pad keeps an integer array integral and casts the constant to its dtype
    lane = None
    if ints:
        lane = _dt.lane_of(src)
        dt, sfx, x = _dt.torch_dtype(lane), _LANE_SFX[lane.name], _widen(x, lane)
    else:
        dt, sfx = _common(x)
        x = asdevice(x, dt)
    half = src == _dt.FLOAT16
    nd = x.dim()
    lo = [0] * nd
    hi = [0] * nd
    bcv = [0] * nd
    fv = [0 if ints else 0.0] * nd
    order = []
    for ax, (l, h) in widths.items():
        ax = ax % nd
        lo[ax], hi[ax] = int(l), int(h)
        bcv[ax] = _hip.BC[bc.get(ax)]
        f = fill.get(ax, 0.0) if fill.get(ax, 0.0) is not None else 0.0
        fv[ax] = _lane_int(_dt.fill_as(src, f), lane) if ints else float(f)
        order.append(ax)
    order += [d for d in range(nd) if d not in order]
    oshape = [s + l + h for s, l, h in zip(x.shape, lo, hi)]
    if x.numel() == 0 and any(oshape):
        # nothing to read, cells only from the padding (a user ufunc that consumed its whole short axis, padded afterwards):
        # numpy.pad's own rules on the empty array -- 'constant' fills, any other mode on an empty axis is its ValueError --
        # then one upload; there is no kernel to launch over zero input cells
        modes = {0: None, _hip.BC["fill"]: "constant", _hip.BC["periodic"]: "wrap", _hip.BC["extend"]: "edge"}
        host = np.empty(tuple(x.shape), dtype=_dt._TORCH_TO_NUMPY[dt])
        for ax in order:
            if lo[ax] or hi[ax]:
                width = [(0, 0)] * nd
                width[ax] = (lo[ax], hi[ax])
                mode = modes[bcv[ax]]
                host = np.pad(host, width, mode=mode, **({"constant_values": fv[ax]} if mode == "constant" else {}))
        out = asdevice(host, dt)
        return _narrow(out, src) if ints else _out(out, half)
    out = _empty(oshape, dtype=dt, device=x.device)
    if out.numel() == 0:
        return _narrow(out, src) if ints else _out(out, half)
    _check(
        getattr(lib, "xg_pad_" + sfx)(x.data_ptr(), out.data_ptr(), _hip.i64(list(x.shape)), nd, _hip.i64(lo),
                                      _hip.i64(hi), _hip.ints(bcv), _hip.reals(fv, sfx), _hip.ints(order), _stream())
    )
    return _narrow(out, src) if ints else _out(out, half)


def upload_tokens(tokens: np.ndarray) -> torch.Tensor:
    """int64 token plane of a halo map -> HBM (see xg_gather_f64 in include/xgcm_hip.h)."""
    _require_gpu()
    return torch.from_numpy(np.ascontiguousarray(tokens, dtype=np.int64)).to(_MEM.device)


def gather(x, partner, tokens, mapped: Sequence[bool], lo: Sequence[int], out_shape: Sequence[int],
           fills: Sequence[float], partner_perm: Optional[Sequence[int]] = None) -> torch.Tensor:
    """Padded array of a complex topology through a token map (xg_gather_f64)."""
    lib = _MEM.lib()
    ints = _is_int(x) and (partner is None or _is_int(partner))
    res_dt = None
    half = False
    if ints:  # halos of an integer field stay integral (the reference concatenates / pads the array in its own dtype)
        res_dt = np.result_type(_dt.np_dtype(x), *([] if partner is None else [_dt.np_dtype(partner)]))
        ints = _dt.is_integer(res_dt)  # int64 with uint64 promotes to float64
    lane = None
    if ints:
        lane = _dt.lane_of(res_dt)
        dt, sfx = _dt.torch_dtype(lane), _LANE_SFX[lane.name]
        x = _widen(x if _dt.np_dtype(x) == res_dt else convert(x, res_dt), lane)
        fills = [_lane_int(_dt.fill_as(res_dt, f), lane) for f in fills]
    else:
        dt, sfx = _common(x, partner) if partner is not None else _common(x)
        half = _half(x, partner)
        x = asdevice(x, dt)
    nd = x.dim()
    if partner is not None:
        partner = _widen(partner if _dt.np_dtype(partner) == res_dt else convert(partner, res_dt), lane) if ints else asdevice(partner, dt)
        if partner.dim() != nd:
            raise ValueError("gather: the other vector component must have as many dims as the padded one")
        if partner_perm is None:
            partner_perm = list(range(nd))
    if not isinstance(tokens, torch.Tensor):
        tokens = upload_tokens(tokens)
    out = _empty([int(v) for v in out_shape], dtype=dt, device=x.device)
    if out.numel() == 0:
        return _narrow(out, res_dt) if ints else _out(out, half)
    _check(
        getattr(lib, "xg_gather_" + sfx)(
            x.data_ptr(), _ptr(partner), out.data_ptr(), _hip.i64(list(x.shape)),
            _hip.i64(list(partner.shape)) if partner is not None else None, _hip.i64(list(out_shape)), nd,
            _hip.ints([1 if m else 0 for m in mapped]), _hip.ints(partner_perm) if partner is not None else None,
            _hip.i64(list(lo)), tokens.data_ptr(), int(tokens.numel()), _hip.reals(list(fills) or [0.0], sfx),
            len(fills), _stream())
    )
    return _narrow(out, res_dt) if ints else _out(out, half)


def put_halo(out: torch.Tensor, halo, axis: int, pad_lo: int, pad_hi: int) -> torch.Tensor:
    """Write the pre-gathered halo slab `halo` (shaped like `out` with `axis` shortened to pad_lo + pad_hi, low halo first)
    into the halo cells of `out` IN PLACE (xg_halo_put): `Grid.cumsum` on a connected axis scans straight into the padded
    layout and fills the halo cells of the cumulative field afterwards -- no padded copy."""
    _sibling_written(out)
    lib = _MEM.lib()
    if not (isinstance(out, torch.Tensor) and _MEM.holds(out) and out.is_contiguous()):
        raise ValueError("put_halo writes in place: `out` must be a contiguous HBM tensor")
    axis = axis % out.dim()
    expect = list(out.shape)
    expect[axis] = pad_lo + pad_hi
    if list(halo.shape) != expect:
        raise ValueError(f"halo buffer has shape {tuple(halo.shape)}, expected {tuple(expect)}")
    odt = _dt.np_dtype(out)
    if odt == _dt.FLOAT16:  # no float16 lanes: through float32 and back (both exact); callers use the RETURNED tensor
        return convert(put_halo(convert(out, _dt.FLOAT32), halo, axis, pad_lo, pad_hi), _dt.FLOAT16)
    if odt.name not in ("float64", "float32", "int64", "uint64", "int32", "uint32"):
        # (narrower integers never get here: scans / sums of 8 / 16-bit integers return 64-bit)
        raise TypeError(f"put_halo serves float64 / float32 / 64- and 32-bit integer arrays, not {odt}")
    h = _raw_device(halo)
    if _dt.np_dtype(h) != odt:
        h = convert(h, odt)
    sfx = {"float64": "f64", "float32": "f32"}.get(odt.name) or _LANE_SFX[_dt.lane_of(odt).name]
    if h.numel():
        _check(getattr(lib, "xg_halo_put_" + sfx)(h.data_ptr(), out.data_ptr(), _hip.i64(list(out.shape)), out.dim(), axis,
                                                     int(pad_lo), int(pad_hi), _stream()))
    return out


def transform_linear(phi, theta, target, axis: int, mask_edges: bool = True, bypass_checks: bool = False,
                     logarithmic: bool = False) -> torch.Tensor:
    """numpy.interp per column along `axis` (xg_transform_linear_f64).  `theta` and `target` are
    dim-aligned with `phi` (extent 1 = broadcast); along `axis` theta has phi's length, target its
    own number of levels m.  Returns phi's shape with `axis` -> m."""
    lib = _MEM.lib()
    dt, sfx = _common(phi, theta, target)
    phi = asdevice(phi, dt)
    theta = asdevice(theta, dt)
    target = asdevice(target, dt)
    axis = axis % phi.dim()
    shape = list(phi.shape)
    m = int(target.shape[axis])
    oshape = list(shape)
    oshape[axis] = m
    out = _empty(oshape, dtype=dt, device=phi.device)
    if out.numel() == 0:
        return out
    if shape[axis] < 1:
        raise ValueError("transform needs at least one level along the axis")
    th_st = _bstrides(theta, shape, "theta")
    th_st[axis] = theta.stride(axis) if theta.shape[axis] > 1 else 0
    tg_st = _bstrides(target, oshape, "target")
    tg_st[axis] = target.stride(axis) if m > 1 else 0
    _check(
        getattr(lib, "xg_transform_linear_" + sfx)(
            phi.data_ptr(), theta.data_ptr(), _hip.i64(th_st), target.data_ptr(), _hip.i64(tg_st), m, out.data_ptr(),
            _hip.i64(shape), phi.dim(), axis, int(bool(mask_edges)), int(bool(bypass_checks)), int(bool(logarithmic)),
            _stream())
    )
    return out


def transform_conservative(phi, theta, bins, axis: int) -> torch.Tensor:
    """Conservative remap per column (xg_transform_conservative_f64): `theta` is dim-aligned with
    `phi` and has one more level along `axis` (cell vertices); `bins` is a 1-D increasing array of
    bin edges.  Returns phi's shape with `axis` -> len(bins) - 1."""
    lib = _MEM.lib()
    dt, sfx = _common(phi, theta, bins)
    phi = asdevice(phi, dt)
    theta = asdevice(theta, dt)
    bins = asdevice(bins, dt)
    axis = axis % phi.dim()
    shape = list(phi.shape)
    if theta.shape[axis] != shape[axis] + 1:
        raise ValueError(f"theta needs {shape[axis] + 1} vertices along the axis, got {theta.shape[axis]}")
    if bins.dim() != 1 or bins.numel() < 2:
        raise ValueError("bins must be a 1-D array of at least two edges")
    oshape = list(shape)
    oshape[axis] = int(bins.numel()) - 1
    out = _empty(oshape, dtype=dt, device=phi.device)
    if out.numel() == 0:
        return out
    vshape = list(shape)
    vshape[axis] = shape[axis] + 1
    th_st = _bstrides(theta, vshape, "theta")
    th_st[axis] = theta.stride(axis)
    _check(
        getattr(lib, "xg_transform_conservative_" + sfx)(
            phi.data_ptr(), theta.data_ptr(), _hip.i64(th_st), bins.data_ptr(), int(bins.numel()), out.data_ptr(),
            _hip.i64(shape), phi.dim(), axis, _stream())
    )
    return out


def binary(op: str, a, b) -> torch.Tensor:
    """Broadcasting a OP b for dim-aligned operands (same ndim, extents equal or 1)."""
    lib = _MEM.lib()
    if _is_chunked(a) or _is_chunked(b):
        return _binary_blockwise(op, a, b)
    nd = getattr(a, "ndim", 0)
    if nd > _hip.MAX_NDIM and nd == getattr(b, "ndim", -1):
        extents = [max(int(x), int(y)) for x, y in zip(a.shape, b.shape)]
        if sum(n != 1 for n in extents) > _hip.MAX_NDIM:
            # more named dims than the ABI addresses (an outer product of two operator results on different positions of
            # three axes plus a record dim): slice by slice along the first real dim -- each slice has one dim fewer
            d0 = next(d for d, n in enumerate(extents) if n != 1)
            cut = lambda x, i: x if x.shape[d0] == 1 else x[(slice(None),) * d0 + (slice(i, i + 1),)]  # noqa: E731
            return torch.cat([binary(op, cut(a, i), cut(b, i)) for i in range(extents[d0])], dim=d0)
    lanes, res_dt = _dt.binary_plan(op, _dt.np_dtype(a), _dt.np_dtype(b))
    half = False
    if lanes == "int":  # numpy keeps int OP int integral (wrap-around in the promoted dtype): its lanes, narrowed
        lane = _dt.lane_of(res_dt)
        dt, sfx = _dt.torch_dtype(lane), _LANE_SFX[lane.name]
        # an operand narrower than the promoted dtype is converted to IT first (int8 next to uint16 -> int32: sign-extended)
        a = _widen(a if _dt.same_bits(_dt.np_dtype(a), lane) else convert(a, res_dt), lane)
        b = _widen(b if _dt.same_bits(_dt.np_dtype(b), lane) else convert(b, res_dt), lane)
    else:
        dt, sfx = (torch.float32, "f32") if res_dt == _dt.FLOAT32 else (torch.float64, "f64")
        half = _half(a, b)  # one float32 operation rounded once to float16 IS numpy's float16 operation
        a = asdevice(a, dt)
        b = asdevice(b, dt)
    if a.dim() != b.dim():
        raise ValueError("binary: operands must be dim-aligned (same ndim)")
    if a.dim() == 0:  # two scalars (a mean over every dim: total / total weight): one cell of a 1-d launch
        one = binary(op, a.reshape(1), b.reshape(1))
        return one.reshape(())
    shape = []
    for sa, sb in zip(a.shape, b.shape):
        if sa != sb and 1 not in (sa, sb):
            raise ValueError(f"binary: extents {sa} and {sb} do not broadcast")
        shape.append(max(sa, sb) if 0 not in (sa, sb) else 0)
    out = _empty(shape, dtype=dt, device=a.device)
    if out.numel():
        sa, sb = _bstrides(a, shape, "a"), _bstrides(b, shape, "b")
        kshape = list(shape)
        if len(kshape) > _hip.MAX_NDIM:
            # an outer product of many named dims (two operator results on different positions of three axes): extent-1 dims
            # go, neighbours that both operands walk like one dim merge; what still has more dims than the ABI takes is
            # refused below with its message
            keep = [d for d, n in enumerate(kshape) if n != 1] or [0]
            kshape, sa, sb = [kshape[d] for d in keep], [sa[d] for d in keep], [sb[d] for d in keep]
            d = len(kshape) - 2
            while d >= 0:
                if sa[d] == sa[d + 1] * kshape[d + 1] and sb[d] == sb[d + 1] * kshape[d + 1]:
                    kshape[d] *= kshape.pop(d + 1)
                    sa[d], sb[d] = sa.pop(d + 1), sb.pop(d + 1)
                d -= 1
        _check(
            getattr(lib, "xg_binary_" + sfx)(_hip.BINOP[op], a.data_ptr(), _hip.i64(sa), b.data_ptr(),
                              _hip.i64(sb), out.data_ptr(), _hip.i64(kshape), len(kshape), _stream())
        )
    return _narrow(out, res_dt) if lanes == "int" else _out(out, half)


def _binary_blockwise(op: str, a, b):
    """a OP b with a chunked operand: the blocks of the chunked one (of `a` when both are), the other operand's matching part"""
    from . import chunked as _ch

    lead, other, flipped = (a, b, False) if _is_chunked(a) else (b, a, True)
    if len(lead.shape) != len(other.shape):
        raise ValueError("binary: operands must be dim-aligned (same ndim)")
    nd = len(lead.shape)
    for ls, os_ in zip(lead.shape, other.shape):
        if ls != os_ and 1 not in (ls, os_):
            raise ValueError(f"binary: extents {ls} and {os_} do not broadcast")

    def per_block(blk, sl):
        # a dim one of the two only broadcasts along passes whole on the other side
        key = tuple(slice(None) if (lead.shape[d] == 1 or other.shape[d] == 1) else sl[d] for d in range(nd))
        part = np.asarray(other[key]) if _is_chunked(other) else other[key]
        return binary(op, part, blk) if flipped else binary(op, blk, part)

    res = _blockwise(per_block, lead, None)
    # where the chunked operand had extent 1 and the other one more, the single block there is as long as the other operand
    chunks = tuple((int(os_),) if (ls == 1 and os_ != 1) else c for c, ls, os_ in zip(res.chunks, lead.shape, other.shape))
    return _ch.BlockArray(res.blocks, chunks, res.dtype)


class _Plan(NamedTuple):
    """one form of a row of _hip.FUSED, resolved for `_fused` once at import"""

    names: dict      # ABI suffix -> the entry's name (a typed entry has one name and takes the `dtype` code first)
    arrays: tuple    # every array slot of the ROW: the halo slabs count towards the dtype whichever form is called
    fields: tuple    # (name, the header takes NULL)
    same: tuple      # the fields that share the shape everything else is measured against
    base: str        # ... which is "shape", or the "faces" (then the wrapper's check returns `shape`, the levels')
    mismatch: str    # ... and the error when they do not
    metrics: tuple   # (name, name of its strides, the shape it broadcasts against, what a stride error calls it)
    halos: tuple     # (name, the dim of the last two the slab keeps)
    work: tuple      # names
    results: tuple   # (name, the shape it has: "shape" / "faces")
    call: tuple      # (the header's parameter name, value -> argument or None: as it is), in the ABI's order


def _flag(x) -> int:
    return int(bool(x))


# value -> argument of the scalar slots (None: as it is); a pointer that is never NULL goes through Tensor.data_ptr itself
_ARGUMENT = {"flag": _flag, "real": float, "bc": _hip.BC.__getitem__, "stream": None}


def _plan(row, entry: str, halo: bool) -> _Plan:
    slots = [s for s in row.slots if s.kind != "halo" or halo]
    same = row.same or tuple(s.name for s in slots if s.kind == "field" and s.at == "shape")
    call = [("dtype", None)] if row.typed else []
    for s in slots:
        if s.kind == "metric":
            call += [(s.name, _ptr), (s.name + "_strides", None)]
        elif s.kind == "shape":
            call += [("shape", None), ("ndim", None)]
        elif s.kind == "halo" or s.null:
            call.append((s.name, _ptr))
        else:  # (a boundary is its code and then its fills)
            call.append((s.name, _ARGUMENT.get(s.kind, torch.Tensor.data_ptr)))
            call += [(f, float) for f in s.fills]
    return _Plan(
        names={sfx: entry if row.typed else entry + "_" + sfx for sfx in ("f64", "f32")},
        arrays=tuple(s.name for s in row.slots if s.kind in ("field", "halo", "metric")),
        fields=tuple((s.name, s.null) for s in slots if s.kind == "field"), same=same,
        base=next(s.at for s in slots if s.kind == "field" and s.name == same[0]),
        mismatch=f"{row.op}: {', '.join(same[:-1])} and {same[-1]} must have the same shape",
        metrics=tuple((s.name, s.name + "_strides", s.at, s.what) for s in slots if s.kind == "metric"),
        halos=tuple((s.name, s.dim) for s in slots if s.kind == "halo"), work=tuple(s.name for s in slots if s.kind == "work"),
        results=tuple((s.name, s.at) for s in slots if s.kind == "result"), call=tuple(call))


_PLANS = {entry: _plan(row, entry, halo) for name, row in _hip.FUSED.items() for entry, halo in _hip.forms(name)}
_DTYPE_CODE = {"f64": _hip.DTYPE["float64"], "f32": _hip.DTYPE["float32"]}


def _fused(entry: str, v: dict, check=None):
    """ONE call of a fused entry point, marshalled from its row of _hip.FUSED.  `v` holds the values by the parameter names
    of include/xgcm_hip.h: a wrapper hands over its own `locals()` (names the row does not have are ignored), and what is
    made here -- results, work buffers, strides, `shape`, `ndim`, `dtype`, `stream` -- joins them under its own name.
    `check(v)`, called once the fields are placed, is the wrapper's own validation; it returns the shape of the faces of Z
    where the row measures something against them -- and the levels' shape where the row's fields sit at the faces
    themselves.  Returns the result, or the tuple of them."""
    names, arrays, fields, same, base, mismatch, metrics, halos, work, results, call = _PLANS[entry]
    lib = _MEM.lib()
    dt, sfx = _common(*[v[n] for n in arrays])
    for n, null in fields:
        if not (null and v[n] is None):
            v[n] = asdevice(v[n], dt)
    other = None if check is None else check(v)
    first = v[same[0]]
    for n in same[1:]:
        if v[n] is not None and v[n].shape != first.shape:
            raise ValueError(mismatch)
    shape, faces = (other, list(first.shape)) if base == "faces" else (list(first.shape), other)
    shapes = {"shape": shape, "faces": faces}
    for n, _, _, _ in metrics:
        v[n] = _prep_metric(v[n], dt)
    outs = []
    for n, at in results:
        v[n] = _empty(shapes[at], dtype=dt, device=first.device)
        outs.append(v[n])
    if outs[0].numel():  # (nothing to launch for an empty result: a NULL data_ptr is not a valid ABI argument)
        for n, dim in halos:
            v[n] = None if v[n] is None else asdevice(v[n], dt).reshape(shape[:-2] + [shape[dim]])
        for n in work:
            v[n] = _empty(shape, dtype=dt, device=first.device)
        for n, strides, at, what in metrics:
            v[strides] = _hip.i64(_bstrides(v[n], shapes[at], what))
        v["dtype"], v["shape"], v["ndim"], v["stream"] = _DTYPE_CODE[sfx], _hip.i64(shape), len(shape), _stream()
        _check(getattr(lib, names[sfx])(*[v[n] if arg is None else arg(v[n]) for n, arg in call]))
    return outs[0] if len(outs) == 1 else tuple(outs)


def _form(entry: str, bc_x, bc_y) -> str:
    """the `_halo` form of an entry where an axis takes its one-cell halo from a pre-gathered slab"""
    return entry + "_halo" if bc_x == "halo" or bc_y == "halo" else entry


def _faces(t: torch.Tensor, outer: bool, need: str, level: bool = True):
    """shape of the faces of Z over the placed field `t`: its levels (Z:left) or, `outer`, one more (Z:outer); `need`: the
    error for a field without (Z, Y, X) as its last three dims or, `level`, without a level along Z"""
    if t.dim() < 3 or (level and t.shape[-3] == 0):
        raise ValueError(need)
    shape = list(t.shape)
    return shape[:-3] + [shape[-3] + (1 if outer else 0)] + shape[-2:]


def vorticity(u, v, area, bc_x: str, bc_y: str, fill_x: float = 0.0, fill_y: float = 0.0, halo_x=None,
              halo_y=None) -> torch.Tensor:
    """Fused ((v[j,i]-v[j,i-1]) - (u[j,i]-u[j-1,i])) / area on (..., Y, X) arrays (xg_vorticity_f64).
    A boundary mode "halo" takes that axis' one-cell halo from `halo_x` (..., Y) / `halo_y` (..., X)."""
    return _fused(_form("xg_vorticity", bc_x, bc_y), locals())


def divergence(u, v, area, bc_x: str, bc_y: str, fill_x: float = 0.0, fill_y: float = 0.0, halo_x=None,
               halo_y=None) -> torch.Tensor:
    """Fused ((u[j,i+1]-u[j,i]) + (v[j+1,i]-v[j,i])) / area on (..., Y, X) arrays (xg_divergence_f64).
    A boundary mode "halo" takes that axis' one-cell halo from `halo_x` (..., Y) / `halo_y` (..., X)."""
    return _fused(_form("xg_divergence", bc_x, bc_y), locals())


def gradient(a, bc_x: str, bc_y: str, fill_x: float = 0.0, fill_y: float = 0.0, mx=None, my=None, halo_x=None,
             halo_y=None):
    """Fused (a - a[x-1]) / mx and (a - a[y-1]) / my on a (..., Y, X) array, both center -> left
    (xg_gradient_f64); `mx` / `my` None = plain differences.  A boundary mode "halo" takes that axis'
    one-cell halo of `a` from `halo_x` (..., Y) / `halo_y` (..., X).  Returns (out_x, out_y)."""
    return _fused(_form("xg_gradient", bc_x, bc_y), locals())


def flux(u, v, t, bc_x: str, bc_y: str, fill_x: float = 0.0, fill_y: float = 0.0, halo_x=None, halo_y=None):
    """Fused u * (t[x-1] + t) / 2 and v * (t[y-1] + t) / 2 on (..., Y, X) arrays (xg_flux_f64); the
    boundary modes (or the pre-gathered "halo" slabs) pad the TRACER.  Returns (flux_x, flux_y)."""
    return _fused(_form("xg_flux", bc_x, bc_y), locals())


def flux_divergence(u, v, t, area, bc_x: str, bc_y: str, fill_x: float = 0.0, fill_y: float = 0.0) -> torch.Tensor:
    """Fused divergence(flux(u, v, t)) in one pass (xg_flux_divergence_f64): the flux u * (t[x-1] + t) / 2,
    v * (t[y-1] + t) / 2 never leaves the registers.  `bc_x` / `bc_y` pad the tracer below / left of the first cell
    and the flux above / right of the last one, as the two operators of the chain do; `area` None = no division."""
    return _fused("xg_flux_divergence", locals())


def flux_divergence_3d(u, v, w, t, vol, vol2, bc_x: str, bc_y: str, bc_z: str, fill_x: float = 0.0, fill_y: float = 0.0,
                       fill_z: float = 0.0) -> torch.Tensor:
    """Fused 3-D tracer flux divergence in one pass (xg_flux_divergence3d_f64): flux_divergence's horizontal part plus
    Fz[k+1] - Fz[k] with Fz = w * (t[z-1] + t) / 2, divided by `vol` (* `vol2`, the product formed per cell); `vol` None = no
    division.  Each axis pads twice as the chain does: the tracer below the first cell, then the flux above the last one."""
    return _fused("xg_flux_divergence3d", locals())


def vertical_velocity(u, v, mu, mu2, mv, mv2, area, bc_x: str, bc_y: str, bc_z: str, fill_x: float = 0.0,
                      fill_y: float = 0.0, fill_z: float = 0.0, reverse: bool = False) -> torch.Tensor:
    """Fused w from continuity in one pass (xg_vertical_velocity_f64): the divergence of u * (mu * mu2) and v * (mv * mv2)
    (None: the field itself), its nancumsum along Z from the centre to the left position (upward with the Z pad at level 0,
    or `reverse`), negated and divided by `area` (None = no division).  The second factors vary along Z only."""
    return _fused("xg_vertical_velocity", locals())


def hydrostatic_pressure_gradient(b, w, dxC, dyC, bc_x: str, bc_y: str, bc_z: str, fill_x: float = 0.0, fill_y: float = 0.0,
                                  fill_z: float = 0.0):
    """Fused gradient of the hydrostatic pressure in one pass (xg_hydrostatic_pressure_gradient_f64): the nancumsum of
    b * w along Z from the centre to the outer position (the Z pad at level 0), its mean at the centre, and that field's
    differences towards the left points along X and Y, divided by `dxC` / `dyC` (None = no division; `w` None = b itself).
    Returns (gx, gy)."""
    return _fused("xg_hydrostatic_pressure_gradient", locals())


def vertical_momentum_advection(u, v, w, mu, mv, bc_x: str, bc_y: str, bc_z: str, fill_x: float = 0.0, fill_y: float = 0.0,
                                fill_z: float = 0.0):
    """Fused vertical advection of horizontal momentum in one pass (xg_vertical_momentum_advection_f64): w between a cell
    and the one left of / below it, times the difference of u / v to the level above, the mean of that product with the
    next level's, negated and divided by `mu` / `mv` (None = no division).  Each stage pads as the chain does: w left of /
    below the first cell, u and v above level 0, the products beyond the last level.  Returns (gu, gv)."""
    return _fused("xg_vertical_momentum_advection", locals())


def vertical_diffusion(a, kappa, mf, mc, outer: bool, bc_z: str, fill_z: float = 0.0) -> torch.Tensor:
    """Fused vertical diffusion d/dz(kappa da/dz) in one pass (xg_vertical_diffusion): the difference of `a` to the level
    above, divided by `mf` and multiplied by `kappa` (the flux), the difference of the flux to the next level's, divided by
    `mc` (None = that step is absent).  `outer` False: the flux at Z:left -- `a` is padded above level 0, the flux beyond
    the last level; True: at Z:outer -- `a` is padded on both sides, the flux has one level more and needs no pad.  `kappa`
    and `mf` broadcast against the flux' shape, `mc` against `a`'s."""
    need = "vertical_diffusion: the field needs (Z, Y, X) as its last three dims"
    return _fused("xg_vertical_diffusion", locals(), lambda p: _faces(p["a"], outer, need, level=False))


def implicit_vertical_diffusion(a, kappa, mf, mc, outer: bool, dt: float) -> torch.Tensor:
    """Implicit vertical diffusion in one pass (xg_implicit_vertical_diffusion): solves (I - dt D) x = a column by column,
    D = d/dz(kappa d/dz) with no flux through the top and the bottom -- the Thomas algorithm, a forward and a backward sweep
    in one launch.  `kappa` and `mf` (None = absent) broadcast against the flux' shape, which has `a`'s levels (`outer`
    False, Z:left) or one more (True, Z:outer); `mc` against `a`'s.  The workspace of the forward sweep is allocated here,
    per call: the library keeps no state between calls."""
    need = "implicit_vertical_diffusion: the field needs (Z, Y, X) as its last three dims"
    return _fused("xg_implicit_vertical_diffusion", locals(), lambda p: _faces(p["a"], outer, need, level=False))


def implicit_vertical_viscosity(u, v, nu, mfu, mcu, mfv, mcv, outer: bool, bc_x: str, bc_y: str, dt: float,
                                fill_x: float = 0.0, fill_y: float = 0.0):
    """Implicit vertical viscosity of a C-grid velocity in one pass (xg_implicit_vertical_viscosity): `implicit_vertical_diffusion`
    of u and of v with the centre-point `nu` averaged to u's column, (nu[i-1] + nu[i]) * 0.5, and to v's, (nu[j-1] + nu[j]) *
    0.5, inside the solve's coefficient stage.  `bc_x` / `fill_x` pad `nu` left of column 0, `bc_y` / `fill_y` below row 0.
    `nu`, `mfu` and `mfv` (the metrics of the two fluxes; None = absent) broadcast against the flux' shape, which has the
    fields' levels (`outer` False, Z:left) or one more (True, Z:outer); `mcu` and `mcv` against the fields'.  Returns
    `(xu, xv)`.  The two workspaces of the forward sweeps are allocated here, per call: the library keeps no state."""
    def check(p):
        faces = _faces(p["u"], outer, "implicit_vertical_viscosity: the fields need (Z, Y, X) as their last three dims", level=False)
        if nu is None:
            raise ValueError("implicit_vertical_viscosity: nu is required")
        return faces

    return _fused("xg_implicit_vertical_viscosity", locals(), check)


def richardson_number(b, u, v, mu, mv, mb, outer: bool, bc_x: str, bc_y: str, bc_z: str, fill_x: float = 0.0,
                      fill_y: float = 0.0, fill_z: float = 0.0) -> torch.Tensor:
    """Fused gradient Richardson number at the faces of Z in one pass (xg_richardson_number): the differences of u, v and `b`
    to the level above, divided by `mu`, `mv`, `mb` (None = no division), the means of the first two with the difference
    right of / above them, the sum of their squares, the quotient.  `b` None: the squared shear alone (`mb` is ignored).
    `outer` False: nz faces (Z:left), the fields are padded above level 0; True: nz + 1 (Z:outer), padded on both sides.
    The differences are padded right of the last column / above the last row.  The metrics broadcast against the result."""
    def check(p):
        if p["b"] is None:
            p["mb"] = None
        return _faces(p["u"], outer, "richardson_number: the fields need (Z, Y, X) as their last three dims and a level along Z")

    return _fused("xg_richardson_number", locals(), check)


def richardson_mixing(b, u, v, mu, mv, mb, nu0: float, alpha: float, nu_b: float, kappa_b: float, shear_floor: float,
                      outer: bool, bc_x: str, bc_y: str, bc_z: str, fill_x: float = 0.0, fill_y: float = 0.0,
                      fill_z: float = 0.0):
    """Fused Pacanowski-Philander mixing coefficients at the faces of Z in one pass (xg_richardson_mixing): N2 and S2 as
    `richardson_number` forms them from `b`, `u`, `v` and the metrics, then ri = N2 / (S2 + shear_floor),
    rp = (ri + |ri|) * 0.5, den = 1 + alpha * rp, nu = nu0 / (den * den) + nu_b, kappa = nu / den + kappa_b.  The five
    scalars are cast to the fields' dtype once.  Returns (nu, kappa), two tensors of `richardson_number`'s result shape."""
    need = "richardson_mixing: the fields need (Z, Y, X) as their last three dims and a level along Z"
    return _fused("xg_richardson_mixing", locals(), lambda p: _faces(p["u"], outer, need))


def isopycnal_slope(b, mx, my, mz, outer: bool, bc_x: str, bc_y: str, bc_z: str, fill_x: float = 0.0, fill_y: float = 0.0,
                    fill_z: float = 0.0):
    """Fused isopycnal slopes at the faces of Z in one pass (xg_isopycnal_slope): the differences of `b` to the column / row
    before, divided by `mx` / `my` (None = no division), their means with the difference after, the means of those with the
    level above; the difference of `b` to the level above divided by `mz`; the two quotients, negated.  `outer` False: nz
    faces (Z:left), padded above level 0; True: nz + 1 (Z:outer), padded on both sides.  `mx` and `my` broadcast against
    `b`, `mz` against the results.  Returns (sx, sy)."""
    need = "isopycnal_slope: the field needs (Z, Y, X) as its last three dims and a level along Z"
    return _fused("xg_isopycnal_slope", locals(), lambda p: _faces(p["b"], outer, need))


def redi_tensor(b, mx, my, mz, kappa: float, slope_max2, outer: bool, bc_x: str, bc_y: str, bc_z: str, fill_x: float = 0.0,
                fill_y: float = 0.0, fill_z: float = 0.0):
    """Fused tapered Redi / Gent-McWilliams tensor column at the faces of Z in one pass (xg_redi_tensor): the slopes sx and
    sy of `isopycnal_slope` (its arguments), s2 = sx * sx + sy * sy, and kt * sx, kt * sy, kt * s2 with
    kt = kappa * (slope_max2 / max(s2, slope_max2)), the maximum as m2 + (ex + |ex|) * 0.5 over ex = s2 - m2; `slope_max2`
    (the SQUARE of the largest slope) None: kt = kappa, no taper.  Both scalars are cast to the fields' dtype once.
    Returns (kwx, kwy, kwz)."""
    taper = slope_max2 is not None
    slope_max2 = slope_max2 if taper else 0.0
    need = "redi_tensor: the field needs (Z, Y, X) as its last three dims and a level along Z"
    return _fused("xg_redi_tensor", locals(), lambda p: _faces(p["b"], outer, need))


def redi_horizontal_tensor(b, mx, my, mz, kappa: float, slope_max2, outer: bool, bc_x: str, bc_y: str, bc_z: str,
                           fill_x: float = 0.0, fill_y: float = 0.0, fill_z: float = 0.0):
    """Fused tapered off-diagonal components of the Redi / Gent-McWilliams tensor at u's and at v's points in one pass
    (xg_redi_horizontal_tensor, include/xgcm_hip.h): the differences of `b` to the column / row before divided by `mx` /
    `my`; the difference of `b` along Z divided by `mz` at the faces (`outer` False: nz of them, the derivative padded beyond
    the last; True: nz + 1) and averaged back to the levels, then towards u's and v's points; the other derivative averaged
    to the centre and towards the point; the two slopes at each point, s2 = sx * sx + sy * sy and `redi_tensor`'s
    kt = kappa * (slope_max2 / max(s2, slope_max2)); `slope_max2` None: kt = kappa.  `mx` and `my` broadcast against `b`,
    `mz` against its faces.  Returns (kuz, kvz), of `b`'s shape."""
    taper = slope_max2 is not None
    slope_max2 = slope_max2 if taper else 0.0
    need = "redi_horizontal_tensor: the field needs (Z, Y, X) as its last three dims and a level along Z"
    return _fused("xg_redi_horizontal_tensor", locals(), lambda p: _faces(p["b"], outer, need))


def redi_vertical_flux_divergence(a, kwx, kwy, mx, my, mc, outer: bool, closed: bool, bc_x: str, bc_y: str, bc_z: str,
                                  fill_x: float = 0.0, fill_y: float = 0.0, fill_z: float = 0.0) -> torch.Tensor:
    """Fused divergence of the off-diagonal vertical isoneutral flux of `a` in one pass (xg_redi_vertical_flux_divergence):
    the level means of `isopycnal_slope` formed of `a` (its `mx`, `my` and pads), their means at the faces of Z, the flux
    kwx * gx + kwy * gy there, the difference of the flux to the next face's divided by `mc` (None = no division).  `kwx`
    and `kwy` have the face shape, nz faces (`outer` False) or nz + 1 (True): the results of `redi_tensor`.  `closed`: the
    flux at face 0 and, `outer`, at face nz is +0.0 and nothing is read there.  `mx`, `my` and `mc` broadcast against `a`.
    Returns the result, of `a`'s shape."""
    def check(p):
        faces = _faces(p["a"], outer, "redi_vertical_flux_divergence: the field needs (Z, Y, X) as its last three dims and a level along Z")
        for what in ("kwx", "kwy"):
            if list(p[what].shape) != faces:
                raise ValueError(f"redi_vertical_flux_divergence: {what} has shape {tuple(p[what].shape)}, the faces have {tuple(faces)}")
            p[what] = p[what].contiguous()
        return faces

    return _fused("xg_redi_vertical_flux_divergence", locals(), check)


def bolus_velocity(kwx, kwy, mzu, mzv, dyG, dxG, rA, outer: bool, closed: bool, bc_x: str, bc_y: str, bc_z: str,
                   fill_x: float = 0.0, fill_y: float = 0.0, fill_z: float = 0.0):
    """Fused Gent-McWilliams eddy-induced (bolus) velocity in one pass (xg_bolus_velocity): the means of `kwx` / `kwy` with
    the column / row before (the streamfunction), `closed`: +0.0 at face 0 and, `outer`, at face nz, nothing read there; the
    difference to the next face's divided by `mzu` / `mzv` and negated (ub, vb, at the levels); the streamfunction times
    `dyG` / `dxG`, the differences of the two transports to the next column's / row's, their sum divided by `rA` (wb, at
    the faces).  `kwx` and `kwy` have nz faces (`outer` False) or nz + 1 (True): the results of `redi_tensor`.  `mzu` and
    `mzv` broadcast against the levels' shape, `dyG`, `dxG` and `rA` against the faces'; None = that step is absent.
    Returns (ub, vb, wb)."""
    def check(p):
        faces = list(p["kwx"].shape)
        if len(faces) < 3 or faces[-3] < 1 + bool(outer):
            raise ValueError("bolus_velocity: the fields need (Z face, Y, X) as their last three dims and a level along Z")
        for what in ("kwx", "kwy"):
            p[what] = p[what].contiguous()
        return faces[:-3] + [faces[-3] - (1 if outer else 0)] + faces[-2:]

    return _fused("xg_bolus_velocity", locals(), check)


def kinetic_energy(u, v, bc_x: str, bc_y: str, fill_x: float = 0.0, fill_y: float = 0.0) -> torch.Tensor:
    """Fused 0.5 * (interp(u * u, X) + interp(v * v, Y)) at the cell centre in one pass (xg_kinetic_energy_f64): the
    squares are padded right of / above the last column / row (fill: the fill value itself)."""
    return _fused("xg_kinetic_energy", locals())


def momentum_advection(u, v, coriolis, rAz, dxC, dyC, bc_x: str, bc_y: str, fill_x: float = 0.0, fill_y: float = 0.0):
    """Fused vector-invariant momentum advection (+ Coriolis) in one pass (xg_momentum_advection_f64): (gu, gv) with
    gu = interp(zeta, Y) * interp(interp(v, X), Y) - d ke / dx, gv = -(interp(zeta, X) * interp(interp(u, Y), X)) - d ke / dy,
    zeta = vorticity(u, v) / rAz + coriolis.  rAz, dxC, dyC all given or all None; `coriolis` None = no Coriolis term."""
    return _fused("xg_momentum_advection", locals())


def horizontal_viscosity(u, v, rA, rAz, dxC, dyC, dyG, dxG, nu_d, nu_z, bc_x: str, bc_y: str, fill_x: float = 0.0,
                         fill_y: float = 0.0, zfill_x: Optional[float] = None, zfill_y: Optional[float] = None):
    """Fused vector-invariant harmonic viscosity in one pass (xg_horizontal_viscosity_f64): (gu, gv) with
    gu = d(D * nu_d) / dx - d(zeta * nu_z) / dy, gv = d(D * nu_d) / dy + d(zeta * nu_z) / dx, D = divergence(u, v) / rA,
    zeta = vorticity(u, v) / rAz.  The six metrics rA, rAz, dxC, dyC, dyG, dxG all given or all None; the two coefficients
    both given or both None.  `zfill_x` / `zfill_y` pad the product zeta * nu_z (default: `fill_x` / `fill_y`)."""
    zfill_x, zfill_y = fill_x if zfill_x is None else zfill_x, fill_y if zfill_y is None else zfill_y
    return _fused("xg_horizontal_viscosity", locals())


def laplacian(a, bc_x: str, bc_y: str, fill_x: float = 0.0, fill_y: float = 0.0, dxC=None, dyC=None, dyG=None,
              dxG=None, area=None) -> torch.Tensor:
    """Fused finite-volume del2 in one pass (xg_laplacian_f64): Fx = (a - a[x-1]) / dxC * dyG, Fy = (a - a[y-1]) / dyC
    * dxG (the four metrics None: plain differences), then (Fx[x+1] - Fx + Fy[y+1] - Fy) / area -- gradient, the two
    face-length products and divergence bit for bit, with the two boundary rules of that chain (see flux_divergence)."""
    return _fused("xg_laplacian", locals())


def stencil2d_supported(x, padx, pady) -> bool:
    """Can xg_stencil2d_f64 serve this call (else run the two axes one after the other)?"""
    shape = tuple(x.shape)  # numpy (host) or torch (HBM) data
    lane = 2 if _dt.np_dtype(x).itemsize == 8 else 4  # elements of the 16-byte lane vector (float16 computes on float32 lanes)
    if isinstance(x, torch.Tensor) and _MEM.holds(x) and (x.data_ptr() % 16 or not x.is_contiguous()):
        return False  # a contiguous view at an odd element offset: the two 1-D launches handle it (8-byte lanes)
    return (len(shape) >= 2 and shape[-1] % lane == 0 and sum(padx) == 1 and sum(pady) == 1
            and shape[-1] > 0 and shape[-2] > 0)


def stencil2d(op: str, x, order: int, padx, bc_x: str, fill_x: float, pady, bc_y: str, fill_y: float, metrics=None) -> torch.Tensor:
    """OP along the last two axes in one pass (xg_stencil2d_f64); order 0 = X then Y, 1 = Y then X.  `metrics`: the
    three (ny, nx) planes (at the input positions, between the two axes, at the output positions) of a
    `metric_weighted` call on both axes (xg_stencil2d_metric_f64)."""
    lib = _MEM.lib()
    dt, sfx = _common(x, *(metrics or ()))
    x = asdevice(x, dt)
    out = _empty(tuple(x.shape), dtype=dt, device=x.device)
    if out.numel() == 0:
        return out
    head = (_hip.OP[op], x.data_ptr(), out.data_ptr(), _hip.i64(list(x.shape)), x.dim(), int(order),
            int(padx[0]), int(padx[1]), _hip.BC[bc_x], float(fill_x), int(pady[0]), int(pady[1]),
            _hip.BC[bc_y], float(fill_y))
    if metrics is None:
        _check(getattr(lib, "xg_stencil2d_" + sfx)(*head, _stream()))
        return out
    planes = [asdevice(m, dt).contiguous() for m in metrics]
    for m in planes:
        if tuple(m.shape) != tuple(x.shape[-2:]):
            raise ValueError(f"metric plane of shape {tuple(m.shape)} for a field whose last two dims are {tuple(x.shape[-2:])}")
    _check(getattr(lib, "xg_stencil2d_metric_" + sfx)(*head, planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), _stream()))
    return out


def synthetic(shape, seed: int, offset: int = 0, scale: float = 1.0, shift: float = -0.5, out=None,
              dtype=torch.float64) -> torch.Tensor:
    """Deterministic synthetic field generated in HBM, bit-identical to oracle.refimpl.synthetic
    (float32: the float64 value rounded once, i.e. `synthetic(...).astype(np.float32)`)."""
    lib = _MEM.lib()
    _require_gpu()
    if out is None:
        # a synthetic field is an INPUT (like an uploaded array): torch's own allocation, unless XG_SCATTER_INPUTS=1 asks for
        # the results' pool (tools: what does the placement of an input cost a reader?)
        import os

        out = (_empty if os.environ.get("XG_SCATTER_INPUTS") == "1" else torch.empty)(tuple(shape), dtype=dtype, device=_MEM.device)
    if out.numel() == 0:
        return out
    _sibling_written(out)
    sfx = "f32" if out.dtype == torch.float32 else "f64"
    _check(getattr(lib, "xg_fill_synthetic_" + sfx)(out.data_ptr(), out.numel(), int(seed), int(offset), float(scale),
                                         float(shift), _stream()))
    return out
