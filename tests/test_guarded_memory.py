"""The guard harness of tests/guarded_memory.py on a machine without a GPU: that it reports what it has to report, and the
battery of tests/test_gpu_tunables.py between guard bands through the host build of the C ABI.

Liveness: planted operators that store one element before and after a result, in the last byte of the far guard, leave a
cell unwritten and read one element outside a placed input -- all through the arena's base tensor, inside memory the test
owns -- must each be reported, and the correct operator must pass, at every offset and in both float types.

The host leg runs `xgcm_amd.device`'s own planning code over libxgcm_host.so with every result and every input guarded: each
battery thunk whose entry the host build serves, at offsets 0, 16 and the element size, float64 and float32, the guards checked
after every thunk and the result compared with the unguarded run.  The thunks whose entry the host build does not serve are
listed in `NOT_SERVED_BY_THE_HOST_BUILD`; that their status is XG_ERR_UNSUPPORTED and nothing else is asserted.  The call
matrix of tests/test_integer_exact.py::test_integer_kernels_at_kernel_sizes runs here at (3, 67, 131) in every integer
dtype: the host build's loops are not the HIP kernels, what is checked is the marshalling and the widening / narrowing
conversions around them.

The limits of the method are those stated in tests/guarded_memory.py: a read outside an input whose value is discarded is
not visible, and memory that the library allocates by itself is not guarded."""

import numpy as np
import pytest

import guarded_memory as GM
import test_gpu_tunables as TT
from oracle import refimpl as R

XG_ERR_UNSUPPORTED = -2
DTYPES = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
# battery thunks whose ABI entry the host build answers with XG_ERR_UNSUPPORTED (it has the 1-D operators, the one-pass
# operators K7d - K7n, vorticity and divergence, the two stencil halo forms, the copy and the conversion): thunk name -> the
# entry it needs
NOT_SERVED_BY_THE_HOST_BUILD = {
    **{k: "xg_stencil2d / xg_stencil2d_metric: no fused two-axis entry in the host build" for k in ("i2", "i2mw")},
    "grad": "xg_gradient: not in the host build", "flux": "xg_flux: not in the host build",
    **{k: "xg_transform_linear / xg_transform_conservative: not in the host build" for k in ("tlin", "tcon")},
    **{f"h{op}{nx}{form}": f"xg_{name}_halo: the host build has the two stencil halo forms only"
       for nx, form in ((260, "shared"), (259, "own"))
       for op, name in (("vort", "vorticity"), ("dive", "divergence"), ("grad", "gradient"), ("flux", "flux"))},
    **{f"hgather{k}": "xg_gather: not in the host build" for k in range(3)},
}


def offsets(dtype):
    return (0, 16, np.dtype(dtype).itemsize)


# ---- liveness ----------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("plant", (None,) + GM.PLANTS)
def test_planted_operators_are_reported(host_abi, monkeypatch, dtype, plant):
    import xgcm_amd.device as D

    x = R.synthetic_field((3, 5, 37), 7).astype(dtype)
    for offset in offsets(dtype):
        got = GM.planted_verdict(D, monkeypatch, x, plant, offset, TT._same_bits)
        print(f"{np.dtype(dtype)} offset {offset}: {plant or 'the correct operator'}: {got}")
        assert got == GM.planted_expectation(x, plant, offset), (plant, offset)


def test_a_call_without_a_guarded_result_is_reported(host_abi, monkeypatch):
    import xgcm_amd.device as D

    with GM.guarded(D, monkeypatch) as g:
        D.asdevice(np.zeros(4))
        with pytest.raises(AssertionError, match="bypasses"):
            g.check("asdevice")
        assert g.placed == 1 and g.handed_out == 0


def test_the_guards_are_nan_and_cover_a_plane_and_a_tail_band():
    import torch

    tile = np.array(GM.PATTERN * 2, dtype=np.uint8)
    assert GM.POISON not in GM.PATTERN
    for at in (0, 4, 8):
        assert np.isnan(tile[at:at + 4].view(np.float32)).all() and (at % 8 or np.isnan(tile[at:at + 8].view(np.float64)).all())
    assert np.isnan(np.full(8, GM.POISON, dtype=np.uint8).view(np.float64)).all() and np.isnan(np.full(4, GM.POISON, dtype=np.uint8).view(np.float32)).all()
    for shape, item in (((5, 300, 264), 8), ((2, 4, 40, 4100), 4), ((3, 9, 4100), 8), ((4099,), 1), ((), 8), ((5, 1, 1), 8)):
        G = GM._guard_bytes(shape, item)
        row = (shape[-1] if shape else 1) * item
        assert G % 512 == 0 and G >= 64 << 10 and G >= 32 * row and G >= 2 * row * (shape[-2] if len(shape) > 1 else 1)
    g = GM.Guards("cpu", 16)
    t = g.empty((3, 5), torch.float32)
    base, at = GM.arena_of(t)
    assert t.is_contiguous() and at == GM._guard_bytes((3, 5), 4) + 16 and t.data_ptr() % 16 == 0 and t.data_ptr() % 32 == 16
    assert torch.isnan(t).all() and g.empty((0, 5), torch.float32).numel() == 0 and len(g.results) == 1
    g.check("empty")
    assert g.results == []


# ---- the host leg --------------------------------------------------------------------------------------------------------
def _close(got, want, exact, dtype):
    if exact:
        return TT._same_bits(got, want)
    rtol = 1e-12 if dtype is np.float64 else 2e-5
    return got.shape == want.shape and got.dtype == want.dtype and np.allclose(got, want, rtol=rtol, atol=300 * rtol, equal_nan=True)


def _hosted(D, r):
    return [D.tohost(x) for x in r] if isinstance(r, tuple) else [D.tohost(r)]


@DTYPES
def test_the_battery_through_the_host_abi_between_guards(host_abi, monkeypatch, dtype):
    import xgcm_amd.device as D

    statuses = []
    check = D._MEM.check
    monkeypatch.setattr(D._MEM, "check", lambda status: (statuses.append(status), check(status))[1])
    # the unguarded run: what every guarded result has to equal, and which thunks the host build serves
    want, unserved = {}, set()
    for k, (fn, _) in TT._battery(D, dtype).items():
        del statuses[:]
        try:
            want[k] = _hosted(D, fn())
        except Exception as err:  # noqa: BLE001 -- whatever it is, it has to be the status checked here
            assert statuses and statuses[-1] == XG_ERR_UNSUPPORTED and all(s == 0 for s in statuses[:-1]), f"{k}: {err!r}"
            unserved.add(k)
    assert unserved == set(NOT_SERVED_BY_THE_HOST_BUILD), sorted(unserved ^ set(NOT_SERVED_BY_THE_HOST_BUILD))
    assert len(want) == 110 and len(unserved) == 17
    bad = []
    for offset in offsets(dtype):
        with GM.guarded(D, monkeypatch, offset) as g:
            calls = TT._battery(D, dtype)   # built inside: the inputs uploaded once are guarded too
            assert g.placed > 100 and set(calls) == set(want) | unserved
            for k, (fn, exact) in calls.items():
                if k in unserved:
                    continue
                got = _hosted(D, fn())
                g.check(f"{k} at offset {offset}")
                if len(got) != len(want[k]) or not all(_close(a, b, exact, dtype) for a, b in zip(got, want[k])):
                    bad.append((k, offset))
            assert g.handed_out >= len(want)
    assert not bad, bad[:20]


@pytest.mark.parametrize("name", ["bool", "int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64"])
def test_the_integer_matrix_through_the_host_abi_between_guards(host_abi, monkeypatch, name):
    """the call matrix of test_integer_kernels_at_kernel_sizes at (3, 67, 131), against numpy on the same integers; offset 8
    keeps every element type aligned to itself and no result aligned to 16 bytes"""
    import test_integer_exact as TE
    import xgcm_amd.device as D

    assert name in TE.INT_DTYPES and len(TE.INT_DTYPES) == 9
    rng = np.random.default_rng(TE.INT_DTYPES.index(name))
    dt = np.dtype(name)
    shape = GM.KERNEL_SHAPES[1]
    a = rng.integers(0, 2, shape).astype(dt) if name == "bool" else rng.integers(np.iinfo(dt).min, np.iinfo(dt).max, shape, dtype=dt, endpoint=True)
    references = {}
    for offset in (0, 8):
        with GM.guarded(D, monkeypatch, offset) as g:
            x = D.asdevice(a)
            n = 0
            for key, thunk, reference in GM.kernel_size_matrix(D, R, x, a, integer=True, no_diff=name == "bool"):
                got = D.tohost(thunk())
                g.check(f"{name} {key} at offset {offset}")
                if key not in references:
                    references[key] = reference()
                TE._same(got, references[key])
                n += 1
            assert n == 3 * (12 * (3 if name == "bool" else 4) + 24 + 1) + 1
