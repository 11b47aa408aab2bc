"""ctypes binding of libxgcm_hip.so (the C ABI declared in include/xgcm_hip.h).

The reference has no native layer; its FFI for this path would be exactly this table.  cffi is
not available in the target image, so the stdlib `ctypes` is used.  There is deliberately NO
fallback: if the shared library is missing the import of any compute entry point raises.
"""

from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple, Optional, Sequence

_HERE = os.path.dirname(os.path.abspath(__file__))
# XG_HIP_LIB points at another build of the same ABI (A/B measurements of kernel variants on one GPU)
LIB_PATH = os.environ.get("XG_HIP_LIB") or os.path.join(_HERE, "libxgcm_hip.so")

# enums of include/xgcm_hip.h
OP = {"diff": 0, "interp": 1, "min": 2, "max": 3, "minu": 4, "maxu": 5}  # minu / maxu: integer entry points, unsigned arrays
BC = {None: 0, "periodic": 1, "fill": 2, "extend": 3, "halo": 4}
BINOP = {"mul": 0, "div": 1, "add": 2, "sub": 3}
MAX_NDIM = 8

_i64p = C.POINTER(C.c_int64)
_intp = C.POINTER(C.c_int)
_f64p = C.POINTER(C.c_double)
_vp = C.c_void_p

# name -> (restype, argtypes); the complete export list of include/xgcm_hip.h
SIGNATURES = {
    "xg_version": (C.c_int, []),
    "xg_last_error": (C.c_int, [C.c_char_p, C.c_int]),
    "xg_set_tunable": (C.c_int, [C.c_char_p, C.c_int]),
    "xg_get_tunable": (C.c_int, [C.c_char_p, _intp]),
    "xg_device_count": (C.c_int, []),
    "xg_set_device": (C.c_int, [C.c_int]),
    "xg_malloc": (C.c_int, [C.POINTER(_vp), C.c_uint64]),
    "xg_free": (C.c_int, [_vp]),
    "xg_memcpy_h2d": (C.c_int, [_vp, _vp, C.c_uint64, _vp]),
    "xg_pin_host": (C.c_int, [_vp, C.c_uint64]),
    "xg_unpin_host": (C.c_int, [_vp]),
    "xg_memcpy_d2h": (C.c_int, [_vp, _vp, C.c_uint64, _vp]),
    "xg_stream_sync": (C.c_int, [_vp]),
    "xg_scatter_alloc": (C.c_int, [C.POINTER(_vp), C.c_uint64, C.c_uint64, C.c_int, C.c_uint64]),
    "xg_scatter_free": (C.c_int, [_vp]),
    "xg_scatter_stats": (C.c_int, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "xg_scatter_grade": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_double)]),
    "xg_scatter_grade_stats": (C.c_int, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "xg_pool_alloc": (_vp, [C.c_ssize_t, C.c_int, _vp]),
    "xg_pool_free": (None, [_vp, C.c_ssize_t, C.c_int, _vp]),
    "xg_stream_create": (C.c_int, [C.POINTER(_vp)]),
    "xg_stream_destroy": (C.c_int, [_vp]),
    "xg_chain_status": (C.c_int, [_intp, _intp]),
    "xg_chain_rearm": (C.c_int, []),
    "xg_event_create": (C.c_int, [C.POINTER(_vp)]),
    "xg_event_record": (C.c_int, [_vp, _vp]),
    "xg_event_elapsed_ms": (C.c_int, [_vp, _vp, C.POINTER(C.c_float)]),
    "xg_event_destroy": (C.c_int, [_vp]),
    "xg_bswap": (C.c_int, [_vp, C.c_uint64, C.c_int, _vp]),
    "xg_mask_value": (C.c_int, [_vp, C.c_uint64, C.c_int, C.c_double, _vp]),
    "xg_stencil1d_f64": (
        C.c_int,
        [C.c_int, _vp, _vp, _i64p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_double,
         _vp, _i64p, _vp, _i64p, _vp],
    ),
    "xg_stencil1d_halo_f64": (
        C.c_int,
        [C.c_int, _vp, _vp, _vp, _i64p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, _vp, _i64p, _vp],
    ),
    "xg_stencil1d_halo_w_f64": (
        C.c_int,
        [C.c_int, _vp, _vp, _vp, _i64p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, _vp, _i64p, _vp, _i64p, _vp],
    ),
    "xg_cumsum1d_f64": (
        C.c_int,
        [_vp, _vp, _i64p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
         C.c_double, _vp, _i64p, _vp, _i64p, _vp],
    ),
    "xg_reduce1d_f64": (C.c_int, [_vp, _vp, _i64p, C.c_int, C.c_int, C.c_int, _vp, _i64p, _vp]),
    "xg_pad_f64": (C.c_int, [_vp, _vp, _i64p, C.c_int, _i64p, _i64p, _intp, _f64p, _intp, _vp]),
    "xg_gather_f64": (
        C.c_int,
        [_vp, _vp, _vp, _i64p, _i64p, _i64p, C.c_int, _intp, _intp, _i64p, _vp, C.c_int64, _f64p, C.c_int, _vp],
    ),
    "xg_halo_put_f64": (C.c_int, [_vp, _vp, _i64p, C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
    "xg_transform_linear_f64": (
        C.c_int,
        [_vp, _vp, _i64p, _vp, _i64p, C.c_int64, _vp, _i64p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp],
    ),
    "xg_transform_conservative_f64": (
        C.c_int, [_vp, _vp, _i64p, _vp, C.c_int64, _vp, _i64p, C.c_int, C.c_int, _vp],
    ),
    "xg_binary_f64": (C.c_int, [C.c_int, _vp, _i64p, _vp, _i64p, _vp, _i64p, C.c_int, _vp]),
    "xg_stencil2d_f64": (
        C.c_int,
        [C.c_int, _vp, _vp, _i64p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int,
         C.c_int, C.c_double, _vp],
    ),
    "xg_stencil2d_metric_f64": (
        C.c_int,
        [C.c_int, _vp, _vp, _i64p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int,
         C.c_int, C.c_double, _vp, _vp, _vp, _vp],
    ),
    "xg_fill_synthetic_f64": (C.c_int, [_vp, C.c_int64, C.c_uint64, C.c_uint64, C.c_double, C.c_double, _vp]),
}

# float32 twins of the compute entry points: same argument order, `float` fill values
# (xg_fill_synthetic_f32 keeps double scale/shift: the value is formed in f64 and rounded once)
for _name in ["xg_stencil1d", "xg_stencil1d_halo", "xg_stencil1d_halo_w", "xg_cumsum1d", "xg_reduce1d", "xg_pad", "xg_gather", "xg_halo_put", "xg_transform_linear", "xg_transform_conservative", "xg_binary", "xg_stencil2d", "xg_stencil2d_metric", "xg_fill_synthetic"]:
    _res, _args = SIGNATURES[_name + "_f64"]
    SIGNATURES[_name + "_f32"] = (_res, list(_args) if _name == "xg_fill_synthetic" else
                                  [C.c_float if a is C.c_double else (C.POINTER(C.c_float) if a is _f64p else a) for a in _args])

# int64 twins of the entry points that serve integer arrays (numpy keeps them integral: diff / min / max / cumsum / pad /
# gather / +,-,*): same argument order, int64 fill values; metric / weight pointers must be NULL (include/xgcm_hip.h)
_i64p_fill = C.POINTER(C.c_int64)
for _name in ["xg_stencil1d", "xg_stencil1d_halo", "xg_cumsum1d", "xg_reduce1d", "xg_pad", "xg_gather", "xg_halo_put", "xg_binary"]:
    _res, _args = SIGNATURES[_name + "_f64"]
    SIGNATURES[_name + "_i64"] = (_res, [C.c_int64 if a is C.c_double else (_i64p_fill if a is _f64p else a) for a in _args])
# int32 twins: the entry points whose integer result keeps the array's width (scans / sums accumulate in 64 bits)
_i32p_fill = C.POINTER(C.c_int32)
for _name in ["xg_stencil1d", "xg_stencil1d_halo", "xg_pad", "xg_gather", "xg_halo_put", "xg_binary"]:
    _res, _args = SIGNATURES[_name + "_f64"]
    SIGNATURES[_name + "_i32"] = (_res, [C.c_int32 if a is C.c_double else (_i32p_fill if a is _f64p else a) for a in _args])

# element types of xg_convert (enum xg_dtype), keyed by numpy dtype name
DTYPE = {"bool": 0, "int8": 1, "int16": 2, "int32": 3, "int64": 4, "uint8": 5, "uint16": 6, "uint32": 7, "uint64": 8,
         "float32": 9, "float64": 10, "float16": 11}
SIGNATURES["xg_copy_nd"] = (C.c_int, [_vp, _i64p, _vp, _i64p, _i64p, C.c_int, C.c_int, _vp])
SIGNATURES["xg_convert"] = (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_uint64, C.c_int, C.c_double, C.c_int, _vp])
# ---- the fused entry points: ONE description each, read here (SIGNATURES) and by the marshaller (device._fused) -------------
class Slot(NamedTuple):
    """one named argument slot of a fused entry point; its name is the parameter's in include/xgcm_hip.h"""

    kind: str            # field | halo | metric | work | result | shape | flag | real | bc | stream
    name: str
    at: str = "shape"    # field / metric / result: it has (broadcasts against) the fields' "shape" or the "faces" of Z
    what: str = ""       # metric (a pointer plus broadcast strides): what a stride error calls it
    null: bool = False   # field: the header takes NULL
    dim: int = 0         # halo (a field that only the `_halo` form has, NULL off a halo axis): the dim of the last two it keeps
    fills: tuple = ()    # bc (a code plus its fills): the names of the fills


class Row(NamedTuple):
    op: str              # the wrapper's name, as the error messages spell it
    slots: tuple         # in the ABI's own order
    typed: bool = False  # one entry with a leading `dtype` code; else an `_f64` / `_f32` pair (the reals are `float` in `_f32`)
    same: tuple = ()     # the fields that share a shape, as the error lists them (default: the fields at "shape", in slot order)


def _fields(*names, **kw):
    return tuple(Slot("field", n, **kw) for n in names)


def _metrics(*names, at="shape"):
    """names, or (name, what a stride error calls it)"""
    return tuple(Slot("metric", n, at, n) if isinstance(n, str) else Slot("metric", n[0], at, n[1]) for n in names)


def _results(*names, at="shape"):
    return tuple(Slot("result", n, at) for n in names)


def _of(kind, *names):
    return tuple(Slot(kind, n) for n in names)


def _bc(*axes):
    return tuple(Slot("bc", "bc_" + a, fills=("fill_" + a,)) for a in axes)


_HALOS = (Slot("halo", "halo_x", dim=-2), Slot("halo", "halo_y", dim=-1))
_SHAPE = _of("shape", "shape")  # `shape` plus `ndim`
_STREAM = _of("stream", "stream")
_XY = _SHAPE + _bc("x", "y")
_XYZ = _SHAPE + _bc("x", "y", "z")
_OUTER_XYZ = _SHAPE + _of("flag", "outer") + _bc("x", "y", "z")
_KAPPA = _fields("a") + _metrics("kappa", ("mf", "metric of the flux"), at="faces") + _metrics(("mc", "metric of the result"))
_SHEAR = _metrics(("mu", "metric at u's points"), ("mv", "metric at v's points"), ("mb", "metric at the centre"), at="faces")
_SLOPE = _fields("b") + _metrics(("mx", "X metric"), ("my", "Y metric")) + _metrics(("mz", "Z metric at the faces"), at="faces")

FUSED = {
    "xg_gradient": Row("gradient", _fields("a") + _HALOS + _results("out_x", "out_y") + _XY + _metrics("mx", "my") + _STREAM),
    "xg_flux": Row("flux", _fields("u", "v", "t") + _HALOS + _results("out_x", "out_y") + _XY + _STREAM),
    "xg_flux_divergence": Row("flux_divergence", _fields("u", "v", "t") + _metrics("area") + _results("out") + _XY + _STREAM),
    "xg_flux_divergence3d": Row("flux_divergence_3d", _fields("u", "v", "w", "t") + _metrics(("vol", "volume"), ("vol2", "volume"))
                                + _results("out") + _XYZ + _STREAM),
    "xg_vertical_velocity": Row("vertical_velocity", _fields("u", "v")
                                + _metrics(*((m, "face weight") for m in ("mu", "mu2", "mv", "mv2")), "area") + _results("out")
                                + _XYZ + _of("flag", "reverse") + _STREAM),
    "xg_hydrostatic_pressure_gradient": Row("hydrostatic_pressure_gradient", _fields("b") + _metrics(("w", "Z weight"), "dxC", "dyC")
                                            + _results("out_x", "out_y") + _XYZ + _STREAM),
    "xg_vertical_momentum_advection": Row("vertical_momentum_advection", _fields("u", "v", "w")
                                          + _metrics(("mu", "metric of gu"), ("mv", "metric of gv")) + _results("out_u", "out_v") + _XYZ + _STREAM),
    "xg_kinetic_energy": Row("kinetic_energy", _fields("u", "v") + _results("out") + _XY + _STREAM),
    "xg_momentum_advection": Row("momentum_advection", _fields("u", "v") + _metrics("coriolis", "rAz", "dxC", "dyC")
                                 + _results("out_u", "out_v") + _XY + _STREAM),
    "xg_horizontal_viscosity": Row("horizontal_viscosity", _fields("u", "v")
                                   + _metrics("rA", "rAz", "dxC", "dyC", "dyG", "dxG", "nu_d", "nu_z") + _results("out_u", "out_v") + _SHAPE
                                   + tuple(Slot("bc", "bc_" + a, fills=("fill_" + a, "zfill_" + a)) for a in "xy") + _STREAM),
    "xg_laplacian": Row("laplacian", _fields("a") + _metrics("dxC", "dyC", "dyG", "dxG", "area") + _results("out") + _XY + _STREAM),
    "xg_vertical_diffusion": Row("vertical_diffusion", _KAPPA + _results("out") + _SHAPE + _of("flag", "outer") + _bc("z") + _STREAM, True),
    "xg_implicit_vertical_diffusion": Row("implicit_vertical_diffusion", _KAPPA + _of("work", "work") + _results("out") + _SHAPE
                                          + _of("flag", "outer") + _of("real", "dt") + _STREAM, True),
    "xg_implicit_vertical_viscosity": Row("implicit_vertical_viscosity", _fields("u", "v")
                                          + _metrics("nu", ("mfu", "metric of u's flux"), at="faces") + _metrics(("mcu", "metric of u's result"))
                                          + _metrics(("mfv", "metric of v's flux"), at="faces") + _metrics(("mcv", "metric of v's result"))
                                          + _of("work", "work_u", "work_v") + _results("out_u", "out_v") + _SHAPE + _of("flag", "outer")
                                          + _bc("x", "y") + _of("real", "dt") + _STREAM, True),
    "xg_richardson_number": Row("richardson_number", _fields("b", null=True) + _fields("u", "v") + _SHEAR + _results("out", at="faces")
                                + _OUTER_XYZ + _STREAM, True, ("u", "v", "b")),
    "xg_richardson_mixing": Row("richardson_mixing", _fields("b", "u", "v") + _SHEAR
                                + _of("real", "nu0", "alpha", "nu_b", "kappa_b", "shear_floor")
                                + _results("out_nu", "out_kappa", at="faces") + _OUTER_XYZ + _STREAM, True, ("u", "v", "b")),
    "xg_isopycnal_slope": Row("isopycnal_slope", _SLOPE + _results("out_x", "out_y", at="faces") + _OUTER_XYZ + _STREAM, True),
    "xg_redi_tensor": Row("redi_tensor", _SLOPE + _of("real", "kappa", "slope_max2") + _of("flag", "taper")
                          + _results("out_x", "out_y", "out_z", at="faces") + _OUTER_XYZ + _STREAM, True),
    "xg_redi_vertical_flux_divergence": Row("redi_vertical_flux_divergence", _fields("a") + _fields("kwx", "kwy", at="faces")
                                            + _metrics(("mx", "X metric"), ("my", "Y metric"), ("mc", "Z metric at the centre"))
                                            + _results("out") + _SHAPE + _of("flag", "outer", "closed") + _bc("x", "y", "z") + _STREAM, True),
    # every field at the faces of Z: `shape`, the levels', is no field's and comes from the wrapper's check (device._Plan.base)
    "xg_bolus_velocity": Row("bolus_velocity", _fields("kwx", "kwy", at="faces")
                             + _metrics(("mzu", "Z metric at u's points"), ("mzv", "Z metric at v's points"))
                             + _metrics(("dyG", "Y metric at u's points"), ("dxG", "X metric at v's points"), ("rA", "area"), at="faces")
                             + _results("out_u", "out_v") + _results("out_w", at="faces") + _SHAPE + _of("flag", "outer", "closed")
                             + _bc("x", "y", "z") + _STREAM, True, ("kwx", "kwy")),
    "xg_redi_horizontal_tensor": Row("redi_horizontal_tensor", _SLOPE + _of("real", "kappa", "slope_max2") + _of("flag", "taper")
                                     + _results("out_u", "out_v") + _OUTER_XYZ + _STREAM, True),
}
for _name in ("vorticity", "divergence"):
    FUSED["xg_" + _name] = Row(_name, _fields("u", "v") + _HALOS + _metrics("area") + _results("out") + _XY + _STREAM)


def forms(name: str):
    """(entry, has the halo slots) of the forms of row `name`: itself, and `_halo` where the row has halo slots"""
    return [(name, False)] + [(name + "_halo", True)] * any(s.kind == "halo" for s in FUSED[name].slots)


def _argtypes(row: Row, halo: bool, real):
    per = {"metric": [_vp, _i64p], "shape": [_i64p, C.c_int], "flag": [C.c_int], "real": [real]}
    args = [C.c_int] if row.typed else []
    for s in row.slots:
        if s.kind != "halo" or halo:
            args += [C.c_int] + [real] * len(s.fills) if s.kind == "bc" else per.get(s.kind, [_vp])
    return args


for _name, _row in FUSED.items():
    for _entry, _halo in forms(_name):
        if _row.typed:
            SIGNATURES[_entry] = (C.c_int, _argtypes(_row, _halo, C.c_double))
        else:
            SIGNATURES[_entry + "_f64"] = (C.c_int, _argtypes(_row, _halo, C.c_double))
            SIGNATURES[_entry + "_f32"] = (C.c_int, _argtypes(_row, _halo, C.c_float))


class MultiDesc(C.Structure):
    """struct xg_multi_desc: one result of xg_stencil_multi"""

    _fields_ = [("op", C.c_int), ("axis", C.c_int), ("pad_lo", C.c_int), ("pad_hi", C.c_int), ("bc", C.c_int),
                ("fill", C.c_double), ("out", _vp)]


DECLINED = 1  # XG_DECLINED: xg_stencil_multi launched nothing; the caller runs the single-operator entries
SIGNATURES["xg_stencil_multi"] = (C.c_int, [C.c_int, _vp, _i64p, C.c_int, C.c_int, C.POINTER(MultiDesc), _vp])

SUFFIX ={"float64": "f64", "float32": "f32", "int64": "i64", "int32": "i32"}

_lib: Optional[C.CDLL] = None


class XgcmHipError(RuntimeError):
    """A C-ABI call returned a negative status (message from xg_last_error)."""


class XgcmInvalidArgument(XgcmHipError, ValueError):
    """XG_ERR_INVALID: the library refused its arguments (an empty axis padded with 'wrap' / 'edge', widths that do not
    fit ...).  numpy raises ValueError for the same requests, and code written against the reference catches that."""


def error_for(status: int, text: str) -> XgcmHipError:
    return (XgcmInvalidArgument if status == -1 else XgcmHipError)(text)


def load() -> C.CDLL:
    """Load the shared library (once) and type every export.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
            "xgcm_amd has no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.xg_version() != 1:
        raise ImportError(f"libxgcm_hip.so ABI version {lib.xg_version()} != 1")
    _lib = lib
    return lib


def set_tunable(name: str, value: int) -> None:
    """launch-shape tunable of the library (speed only, never results); see INTEGRATION.md"""
    check(load().xg_set_tunable(name.encode(), int(value)))


def get_tunable(name: str) -> int:
    v = C.c_int(0)
    check(load().xg_get_tunable(name.encode(), C.byref(v)))
    return int(v.value)


class ChainRescueWarning(RuntimeWarning):
    """A chained scan / reduction gave up on a hand-off and was redone, in stream, by its marching twin."""


_chain_reported = [0, 0]


def chain_status():
    """(gave_up, redone) of xg_chain_status: sticky "some chunk of a chained launch gave up", launches redone so far"""
    g, r = C.c_int(0), C.c_int(0)
    check(load().xg_chain_status(C.byref(g), C.byref(r)))
    return int(g.value), int(r.value)


def chain_check() -> None:
    """Called wherever results leave the library towards the host (tohost / .values, graph replays, stream syncs of
    the streaming paths): warn ONCE per event that a chained launch had to be redone.  The data the caller reads is
    the marching kernel's -- correct -- so this is a warning, not an error (include/xgcm_hip.h: xg_chain_status)."""
    if _lib is None:
        return
    g, r = chain_status()
    if g > _chain_reported[0] or r > _chain_reported[1]:
        _chain_reported[0], _chain_reported[1] = g, r
        import warnings

        warnings.warn(
            f"xgcm_amd: a chained scan / reduction kernel gave up waiting for a predecessor chunk; {r} launch(es) so far "
            "were redone by the marching kernel on the same stream (results are correct).  The library plans marching "
            "kernels from now on; xgcm_amd._hip.chain_rearm() re-enables the chained ones, XG_SCAN_CHAIN=0 avoids them.",
            ChainRescueWarning, stacklevel=3)


def chain_rearm() -> None:
    check(load().xg_chain_rearm())
    _chain_reported[0] = 0


def scatter_stats() -> dict:
    """scattered result buffers made so far, bytes alive, and pool requests that fell back to plain hipMalloc"""
    a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    check(load().xg_scatter_stats(C.byref(a), C.byref(b), C.byref(c)))
    g, r = C.c_uint64(0), C.c_uint64(0)
    check(load().xg_scatter_grade_stats(C.byref(g), C.byref(r)))
    # graded: pool requests of 1 GiB or more whose buffer was graded; rejected: buffers parked and released on the way to a good one
    return {"buffers_made": int(a.value), "live_bytes": int(b.value), "pool_fallbacks": int(c.value), "graded": int(g.value),
            "rejected": int(r.value)}


def last_error() -> str:
    buf = C.create_string_buffer(512)
    load().xg_last_error(buf, 512)
    return buf.value.decode(errors="replace")


def check(status: int) -> None:
    if status != 0:
        raise error_for(status, f"xgcm_hip status {status}: {last_error()}")


def i64(values: Optional[Sequence[int]]):
    if values is None:
        return None
    return (C.c_int64 * len(values))(*[int(v) for v in values])


def ints(values: Optional[Sequence[int]]):
    if values is None:
        return None
    return (C.c_int * len(values))(*[int(v) for v in values])


def reals(values: Optional[Sequence[float]], suffix: str):
    """array of fill values in the C type of the `_f64` / `_f32` entry point"""
    if values is None:
        return None
    if suffix == "i64":
        return (C.c_int64 * len(values))(*[int(v) for v in values])
    if suffix == "i32":
        return (C.c_int32 * len(values))(*[int(v) for v in values])
    ctype = C.c_double if suffix == "f64" else C.c_float
    return (ctype * len(values))(*[float(v) for v in values])
