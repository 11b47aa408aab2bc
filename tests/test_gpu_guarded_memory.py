"""Every result and every input of the HIP library between guard bands (tests/guarded_memory.py): a store that lands outside
a result, a cell a kernel never writes and a read outside an input that changes a result fail here; the rest of the suite
looks at the cells inside a result only.

What runs: the battery of tests/test_gpu_tunables.py and the K7l - K7n call tables of the three operators' own tunable sweeps,
at payload offsets 0, 16 and the element size, and at offset 0 under every value of every tunable; the float twins of the call
matrix of tests/test_integer_exact.py::test_integer_kernels_at_kernel_sizes (the int32-lane stencils are the float32 templates
with `MET = 0`) against `oracle.refimpl` on small integers, where numpy is exact; `materialize` / `flip` / `concatenate` /
`copy_into` and the conversion pairs.  The guards are checked after every call, and every call has to have taken at least one
result from `device._empty`.  Battery and K7l - K7n results are compared bit for bit with the unguarded default result, which
is itself compared with the numpy references the tables carry (the contiguous-axis sums: the battery's tolerance).

No integer entry (`*_i64`, `*_i32`) runs here: tests/test_guarded_memory.py runs their call matrix through the host build.

Limits of the method: a read outside an input whose value is discarded (loaded and masked off, or a NaN that a NaN-skipping
sum counts as 0) is not visible; the
workspaces the library allocates by itself (the hand-off words of the chained scans, LDS) are not guarded; inputs that a test
uploads with `.cuda()` instead of `device.asdevice` are not guarded; a store further from the result than the guard (at
least 64 KiB, two (Y, X) planes and 32 rows) is not seen.  Every planted access and every guard is inside memory that the
test owns."""

import functools
import itertools
import warnings

import numpy as np
import pytest

import guarded_memory as GM
import test_gpu_tunables as TT
from oracle import refimpl as R

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
K7LMN = ("xg_vertical_diffusion", "xg_implicit_vertical_diffusion", "xg_richardson_number")


def offsets(dtype):
    return (0, 16, np.dtype(dtype).itemsize)


def _tables(D, dtype, references=None):
    """name -> (thunk, exact?): the battery, then the K7l - K7n tables of the three operators' own sweeps"""
    import test_gpu_implicit_vertical_diffusion as GI
    import test_gpu_richardson_number as GR
    import test_gpu_vertical_diffusion as GD

    calls = dict(TT._battery(D, dtype, references))
    for tag, module in (("vdiff", GD), ("ivdiff", GI), ("ri", GR)):
        table, refs = module.tunable_calls(D, dtype)
        assert len(table) == 8 and set(table) == set(refs)
        for k, fn in table.items():
            assert tag + k not in calls
            calls[tag + k] = (fn, True)
            if references is not None:
                references[tag + k] = lambda ref=refs[k]: [ref()]
    return calls


def _hosted(D, r):
    return [D.tohost(x) for x in r] if isinstance(r, tuple) else [D.tohost(r)]


@functools.lru_cache(maxsize=None)
def _default(dtype):
    """the unguarded results under the default tunables, compared with every numpy reference the tables carry; computed once
    per element type and shared"""
    from xgcm_amd import device as D

    references = {}
    calls = _tables(D, dtype, references)
    want = {k: _hosted(D, fn()) for k, (fn, _) in calls.items()}
    assert len(references) == 20 + 23 + 20 + 24
    for k, reference in references.items():
        ref = reference()
        assert len(ref) == len(want[k]) and all(TT._same_bits(g, w) for g, w in zip(want[k], ref)), f"{k}: the default result is not numpy's"
    return want


@functools.lru_cache(maxsize=None)
def _guarded_tables(dtype):
    """the tables built once with guarded inputs at offset 0, for the sweep"""
    from xgcm_amd import device as D

    with pytest.MonkeyPatch.context() as mp, GM.guarded(D, mp, 0) as g:
        calls = _tables(D, dtype)
        assert g.placed > 100
    return calls


# battery thunks whose entry has no form for arrays that are not aligned to 16 bytes and says so (XG_ERR_UNSUPPORTED): `Grid` asks
# `device.stencil2d_supported` first and runs the two axes one after the other.  With the payload at an offset that is no multiple
# of 16 the refusal itself is what is checked, and that the refused call stored nothing
REFUSES_UNALIGNED = {"i2": "fused 2-D stencil needs an X extent that is a multiple of the 16-byte lane vector",
                     "i2mw": "fused 2-D stencil"}


@pytest.fixture(scope="module", autouse=True)
def _release_the_shared_results():
    yield
    _default.cache_clear()
    _guarded_tables.cache_clear()


def _run_guarded(D, g, calls, want, dtype, tag):
    from xgcm_amd import _hip

    rtol = 1e-12 if dtype is np.float64 else 2e-5
    bad = []
    for k, (fn, exact) in calls.items():
        if g.offset % 16 and k in REFUSES_UNALIGNED:
            with pytest.raises(_hip.XgcmHipError, match="status -2: " + REFUSES_UNALIGNED[k]):
                fn()
            g.check(f"{k} {tag}, refused")
            continue
        got = _hosted(D, fn())
        g.check(f"{k} {tag}")
        ok = len(got) == len(want[k]) and all(
            TT._same_bits(a, b) if exact else (a.shape == b.shape and np.allclose(a, b, rtol=rtol, atol=300 * rtol, equal_nan=True))
            for a, b in zip(got, want[k]))
        if not ok:
            bad.append((k, tag))
    return bad


# ---- a. liveness on the device -------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("plant", (None,) + GM.PLANTS)
def test_planted_operators_are_reported(monkeypatch, dtype, plant):
    from xgcm_amd import device as D

    x = R.synthetic_field((3, 5, 37), 7).astype(dtype)
    for offset in offsets(dtype):
        got = GM.planted_verdict(D, monkeypatch, x, plant, offset, TT._same_bits)
        print(f"{np.dtype(dtype)} offset {offset}: {plant or 'the correct operator'}: {got}")
        assert got == GM.planted_expectation(x, plant, offset), (plant, offset)


# ---- b, c. the battery and K7l - K7n -------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("which", [0, 1, 2], ids=["aligned", "16", "itemsize"])
def test_battery_and_k7lmn_between_guards(monkeypatch, dtype, which):
    from xgcm_amd import _hip
    from xgcm_amd import device as D

    want = _default(dtype)
    offset = offsets(dtype)[which]
    rec = TT._Recorder(D._MEM.lib())
    with GM.guarded(D, monkeypatch, offset) as g:
        calls = _tables(D, dtype)   # built inside: the inputs uploaded once are guarded too
        assert g.placed > 100 and set(calls) == set(want)
        monkeypatch.setattr(D._MEM, "lib", lambda: rec, raising=True)
        bad = _run_guarded(D, g, calls, want, dtype, f"at offset {offset}")
        assert g.handed_out >= len(calls)
    # what was reached, through guarded calls
    sfx = "_f64" if dtype is np.float64 else "_f32"
    abi = {n[:-4] for n in _hip.SIGNATURES if n.startswith("xg_") and n.endswith(sfx)}
    reached = {n[:-4] for n in rec.fetched if n.endswith(sfx)}
    assert abi - reached - set(TT.NOT_IN_BATTERY) == set(), f"ABI entries that no guarded call reaches: {sorted(abi - reached - set(TT.NOT_IN_BATTERY))}"
    assert set(K7LMN) <= rec.fetched, sorted(set(K7LMN) - rec.fetched)
    assert not any(n.endswith(("_i64", "_i32")) for n in rec.fetched)
    assert not bad, bad[:20]


# ---- f. the sweep --------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name", sorted(TT.ALTERNATIVES))
def test_every_tunable_value_between_guards(monkeypatch, dtype, name):
    import torch

    from xgcm_amd import _hip
    from xgcm_amd import device as D

    want, calls = _default(dtype), _guarded_tables(dtype)
    bad = []
    before = _hip.get_tunable(name)
    try:
        with GM.guarded(D, monkeypatch, 0) as g:
            for val in TT.ALTERNATIVES[name]:
                _hip.set_tunable(name, val)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    bad += _run_guarded(D, g, calls, want, dtype, f"under {name} = {val}")
    finally:
        _hip.set_tunable(name, before)
        torch.cuda.synchronize()
        _hip.chain_rearm()
    assert not bad, bad[:20]


# ---- d. the float twins of the integer matrix -----------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("shape", GM.KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_float_twins_of_the_integer_matrix(monkeypatch, dtype, shape, axis):
    """small integers in float lanes: numpy's sums are exact, so the contiguous-axis scans and sums are compared bit for bit
    like everything else"""
    from xgcm_amd import device as D

    rng = np.random.default_rng(shape[2])
    a = rng.integers(-40, 41, shape).astype(dtype)
    assert max(shape) * 40 < 2 ** 23
    references = {}
    for offset in (0, np.dtype(dtype).itemsize):
        with GM.guarded(D, monkeypatch, offset) as g:
            x = D.asdevice(a)
            n = 0
            for key, thunk, reference in GM.kernel_size_matrix(D, R, x, a, axes=(axis,)):
                got = D.tohost(thunk())
                g.check(f"{key} at offset {offset}")
                if key not in references:
                    references[key] = reference()
                assert TT._same_bits(got, references[key]), (key, offset)
                n += 1
            assert n == 48 + 24 + 1 + 3 + (axis == 0) and g.placed == 1


# ---- e. layout and conversion --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32", "int64", "int16", "bool"])
def test_layouts_between_guards(monkeypatch, dtype):
    """the calls of tests/test_copy.py::test_device_layouts_match_numpy; then every part of a concatenation copied alone into
    its slice of a result: the cells of the neighbouring parts keep their 0xFF bytes"""
    import torch

    from xgcm_amd import device as D

    rng = np.random.default_rng(2)
    item = np.dtype(dtype).itemsize
    for shape in ((3, 40, 130), (2, 5, 64, 96), (7, 33), (4, 3, 2, 5, 6, 7)):
        a = (rng.standard_normal(shape) * 100)
        a = (a > 0) if dtype == "bool" else a.astype(dtype)
        nd = a.ndim
        for offset in (0, 16, item):
            with GM.guarded(D, monkeypatch, offset) as g:
                t = D.asdevice(a)
                assert g.placed == 1

                def same(got, want, what):
                    assert got.is_contiguous()
                    g.check(f"{what} of {shape} {dtype} at offset {offset}")
                    np.testing.assert_array_equal(D.tohost(got), want)

                for perm in itertools.islice(itertools.permutations(range(nd)), 0, 30, 3):
                    if perm == tuple(range(nd)):
                        continue   # contiguous already: `materialize` hands the tensor back, there is no result to guard
                    same(D.materialize(t.permute(*perm)), np.ascontiguousarray(a.transpose(perm)), f"materialize {perm}")
                for axes in ([0], [-1], [0, -1], list(range(nd))):
                    same(D.flip(t, axes), np.flip(a, axes), f"flip {axes}")
                    same(D.flip(t.permute(*reversed(range(nd))), axes), np.flip(a.T, axes), f"flip {axes} of the transpose")
                same(D.materialize(t[..., ::2]), a[..., ::2], "materialize every second column")
                same(D.materialize(t[:1].expand(*shape)), np.broadcast_to(a[:1], shape), "materialize a broadcast")
                for ax in range(nd):
                    parts = [t.narrow(ax, 0, 1), t, t.narrow(ax, shape[ax] - 1, 1)]
                    hparts = [a.take([0], ax), a, a.take([shape[ax] - 1], ax)]
                    same(D.concatenate(parts, ax), np.concatenate(hparts, ax), f"concatenate along {ax}")
                    oshape = list(shape)
                    oshape[ax] += 2
                    for k, at in enumerate((0, 1, shape[ax] + 1)):
                        out = D._empty(oshape, t.dtype, t.device)
                        D.copy_into(out.narrow(ax, at, hparts[k].shape[ax]), parts[k])
                        g.check(f"copy_into part {k} along {ax} of {shape} {dtype} at offset {offset}")
                        got = D.tohost(out.view(-1).view(torch.uint8)).reshape(tuple(oshape) + (item,))
                        want = np.full(got.shape, GM.POISON, dtype=np.uint8)
                        sl = [slice(None)] * nd
                        sl[ax] = slice(at, at + hparts[k].shape[ax])
                        want[tuple(sl)] = np.ascontiguousarray(hparts[k]).view(np.uint8).reshape(hparts[k].shape + (item,))
                        assert np.array_equal(got, want), (shape, dtype, offset, ax, k)


def test_conversions_between_guards(monkeypatch):
    """the pairs of tests/test_integer_exact.py::test_convert_kernel_is_numpy_astype at n = 4099; offset 8 keeps every element
    type aligned to itself and nothing aligned to 16 bytes"""
    import test_integer_exact as TE
    from xgcm_amd import device as D

    rng = np.random.default_rng(9)
    n = 4099
    cases = []
    for src in TE.INT_DTYPES + ("float32", "float64"):
        sdt = np.dtype(src)
        if sdt.kind == "f":
            a = (rng.random(n) * 200 - 100).astype(sdt)
        elif src == "bool":
            a = rng.integers(0, 2, n).astype(sdt)
        else:
            a = rng.integers(np.iinfo(sdt).min, np.iinfo(sdt).max, n, dtype=sdt, endpoint=True)
        for dst in TE.INT_DTYPES + ("float32", "float64"):
            if sdt.kind == "f" and np.dtype(dst).kind in "iu" and np.dtype(dst).itemsize < 8:
                continue  # out-of-range float -> narrow int is undefined in C and in numpy alike
            if sdt.kind == "f" and np.dtype(dst).kind == "u":
                continue  # negative float -> unsigned: undefined
            if src == dst:
                continue  # `convert` hands the array back: no kernel, no result
            cases.append((a, dst, {}, a.astype(dst)))
    w = rng.integers(-2**62, 2**62, n, dtype=np.int64)
    cases.append((w, np.float64, dict(via=np.int8, scale=0.5), w.astype(np.int8) / 2.0))
    u = rng.integers(0, 2**64 - 1, n, dtype=np.uint64, endpoint=True)
    assert len(cases) == 9 * 10 + 2 * 3 + 1
    for offset in (0, 16, 8):
        with GM.guarded(D, monkeypatch, offset) as g:
            for a, dst, kw, want in cases:
                got = D.tohost(D.convert(D.asdevice(a), dst, **kw))
                g.check(f"convert {a.dtype} -> {np.dtype(dst)} {kw} at offset {offset}")
                TE._same(got, want)
            flipped = D.convert(D.asdevice(u), np.int64, flip=True)   # uint64 order on signed lanes, and back
            g.check(f"convert uint64 -> int64 flipped at offset {offset}")
            assert np.array_equal(np.argsort(D.tohost(flipped), kind="stable"), np.argsort(u, kind="stable"))
            back = D.convert(flipped, np.uint64, flip=True)
            g.check(f"convert int64 -> uint64 flipped at offset {offset}")
            TE._same(D.tohost(back), u)
            assert g.placed == len(cases) + 1
