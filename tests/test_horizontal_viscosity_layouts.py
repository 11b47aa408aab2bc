"""Layout paths of xg_horizontal_viscosity (K7k) through the C ABI, called DIRECTLY with views as tests/test_fused_layouts.py
calls the other one-pass entries (its view helpers are imported unchanged): the launcher chooses the lane width V from the
alignment of the four field pointers, the form of the plane loads from the strides of every plane that is there, and the
band-major order from the planes' leading strides.  Every view lives in a buffer whose other cells are NaN, so a read outside
it shows up in the result; every result is compared bit for bit with the same entry over the same values held contiguous
and aligned, and that control with the numpy oracle chain of tests/test_horizontal_viscosity.py.

Two legs: libxgcm_host.so (`host_abi`, CPU) and libxgcm_hip.so (marked gpu)."""

import types

import numpy as np
import pytest
import torch

import test_horizontal_viscosity as TH
from oracle import refimpl as R
from test_fused_layouts import ALIGNED, NVS, SFX, TORCH, _abi_strides, _lay, _strided, leg  # noqa: F401  (`leg`: a fixture)
from xgcm_amd import _hip

SHAPES = [(2, 5, 130), (1, 3, 7)]
PADS = [("periodic", "extend"), ("fill", "periodic"), ("extend", "fill")]
PLANES = ("rA", "rAz", "dxC", "dyC", "dyG", "dxG", "nu_d", "nu_z")
FILL = TH.FILL
# broadcast along X / along Y / one value, misaligned, row pitch nx + 1 (float32 also nx + 2), transposed; with a leading
# extent above 1 also one plane per outer index, contiguous and with a pitch
FORMS = ["ex", "ey", "e0", "b", "c", "c2", "d", "f", "g"]

both = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
shapes = pytest.mark.parametrize("shape", SHAPES, ids=["2x5x130", "1x3x7"])


def _values(shape, dtype):
    vals = {"u": R.synthetic_field(shape, 101).astype(dtype), "v": R.synthetic_field(shape, 102).astype(dtype)}
    for k, p in enumerate(PLANES):
        m = R.synthetic_field(shape, 111 + k) * 3.0 if p.startswith("nu") else R.synthetic_metric(shape, 111 + k)
        vals[p] = m.astype(dtype)
    return vals


def _launch(D, dtype, shape, k, u, v, planes):
    """one call of the entry over the views `u`, `v` (contiguous: the ABI takes the fields by pointer alone) and `planes`
    (absent: None); returns (out_u, out_v) as numpy arrays"""
    px, py = PADS[k]
    assert u.is_contiguous() and v.is_contiguous()
    args = [u.data_ptr(), v.data_ptr()]
    for p in PLANES:
        w = planes.get(p)
        args += [None, None] if w is None else [w.data_ptr(), _hip.i64(_abi_strides(w, shape))]
    junk = [torch.full(shape, float("nan"), dtype=TORCH[dtype], device=D._MEM.device) for _ in range(2)]
    del junk  # (the allocator's next blocks are poisoned: an unwritten output cell cannot pass by luck)
    outs = [D._empty(list(shape), TORCH[dtype], D._MEM.device) for _ in range(2)]
    args += [o.data_ptr() for o in outs] + [_hip.i64(list(shape)), len(shape), _hip.BC[px], FILL["X"], FILL["X"], _hip.BC[py],
                                            FILL["Y"], FILL["Y"]]
    D._check(getattr(D._MEM.lib(), "xg_horizontal_viscosity_" + SFX[dtype])(*args, D._stream()))
    return tuple(o.cpu().numpy() for o in outs)


def _equal(got, want, what):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        if not np.array_equal(g, w, equal_nan=True):
            bad = np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))
            raise AssertionError(f"{what}: {len(bad)} cells differ, first {bad[:6].tolist()}, NaN {int(np.isnan(g).sum())}")


def _control(D, dtype, shape, k, vals, present):
    """everything contiguous and aligned; `vals`: what each plane holds, broadcast to its full extent"""
    nv = NVS[dtype]
    u, v = (_lay(D, vals[f], "a", 2, nv)[0] for f in ("u", "v"))
    planes = {p: _lay(D, vals[p], "a", 2, nv)[0] for p in present}
    return _launch(D, dtype, shape, k, u, v, planes)


def _forms(shape, dtype):
    return [f for f in FORMS if (f != "c2" or dtype is np.float32) and (f not in ("f", "g") or shape[0] > 1)]


@both
@shapes
def test_the_contiguous_form_is_the_oracle_chain(leg, dtype, shape):  # noqa: F811
    import xgcm_amd.device as D

    vals = _values(shape, dtype)
    for k, (px, py) in enumerate(PADS):
        for present in (PLANES, PLANES[:6], PLANES[6:], ()):
            shared = {p: vals[p][:1] for p in present}
            got = _control(D, dtype, shape, k, {**vals, **shared}, present)
            ds = {p: types.SimpleNamespace(values=shared[p]) for p in present if not p.startswith("nu")}
            nu = tuple(shared.get(p) for p in PLANES[6:])
            _equal(got, TH._want(vals["u"], vals["v"], px, py, ds or None, nu), f"control {np.dtype(dtype)} {shape} {PADS[k]}")


@both
@shapes
def test_misaligned_fields_inside_poison(leg, dtype, shape):  # noqa: F811
    """u, v or both one element into their NaN-filled allocations (the lane width drops to 1), all planes and none"""
    import xgcm_amd.device as D

    nv = NVS[dtype]
    vals = _values(shape, dtype)
    for k in range(len(PADS)):
        for present in (PLANES, ()):
            shared = {**vals, **{p: vals[p][:1] for p in present}}
            want = _control(D, dtype, shape, k, shared, present)
            planes = {p: _lay(D, shared[p], "a", 2, nv)[0] for p in present}
            for odd in (("u",), ("v",), ("u", "v")):
                u, v = (_lay(D, vals[f], "b" if f in odd else "a", 2, nv)[0] for f in ("u", "v"))
                assert all((w.data_ptr() % 16 != 0) == (f in odd) for f, w in (("u", u), ("v", v)))
                _equal(_launch(D, dtype, shape, k, u, v, planes), want, f"misaligned {odd} {np.dtype(dtype)} {shape} {PADS[k]}")


@both
@shapes
def test_strided_fields_through_the_device_wrapper(leg, dtype, shape):  # noqa: F811
    """the ABI takes the fields by pointer alone, so strided views of u and v go through `device.horizontal_viscosity`, which
    gathers them first: a row pitch of nx + 1 and a transposed store, inside NaN poison"""
    import xgcm_amd.device as D

    nv = NVS[dtype]
    vals = _values(shape, dtype)
    shared = {**vals, **{p: vals[p][:1] for p in PLANES}}
    planes = [_lay(D, shared[p], "a", 2, nv)[0] for p in PLANES]
    for k, (px, py) in enumerate(PADS):
        want = _control(D, dtype, shape, k, shared, PLANES)
        for form in ("c", "d"):
            u, v = (_lay(D, vals[f], form, 2, nv)[0] for f in ("u", "v"))
            assert not u.is_contiguous() or shape[-2] == 1
            gu, gv = D.horizontal_viscosity(u, v, *planes, px, py, FILL["X"], FILL["Y"])
            _equal((gu.cpu().numpy(), gv.cpu().numpy()), want, f"fields in form {form} {np.dtype(dtype)} {shape} {PADS[k]}")


@both
@shapes
def test_plane_forms(leg, dtype, shape):  # noqa: F811
    """the eight planes broadcast, misaligned, pitched, transposed and one per outer index: all eight in the form together,
    then one plane alone in it (a different one per form) while the others stay contiguous"""
    import xgcm_amd.device as D

    nv = NVS[dtype]
    vals = _values(shape, dtype)
    u, v = (_lay(D, vals[f], "a", 2, nv)[0] for f in ("u", "v"))
    for k in range(len(PADS)):
        for n, form in enumerate(_forms(shape, dtype)):
            for group in (PLANES, (PLANES[n % 8],)):
                views, held = {}, dict(vals)
                for p in PLANES:
                    fm = form if p in group else "a"
                    a = vals[p] if fm in ("f", "g") else vals[p][:1]
                    views[p], held[p] = _lay(D, a, fm, 2, nv)
                want = _control(D, dtype, shape, k, held, PLANES)
                _equal(_launch(D, dtype, shape, k, u, v, views), want,
                       f"planes {group} in form {form} {np.dtype(dtype)} {shape} {PADS[k]}")
        # the coefficients alone in every form (no metrics), and the metrics alone
        for form in _forms(shape, dtype):
            for present in (PLANES[6:], PLANES[:6]):
                views, held = {}, dict(vals)
                for p in present:
                    a = vals[p] if form in ("f", "g") else vals[p][:1]
                    views[p], held[p] = _lay(D, a, form, 2, nv)
                want = _control(D, dtype, shape, k, held, present)
                _equal(_launch(D, dtype, shape, k, u, v, views), want,
                       f"planes {present} alone in form {form} {np.dtype(dtype)} {shape} {PADS[k]}")
