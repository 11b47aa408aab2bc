"""The K7i - K7k entries of the tunables battery (`test_gpu_tunables._one_pass_entries`), its entries for the fused vector
operators and K7d - K7h (`_early_entries`) and those for the pre-gathered halo forms and the gather (`_halo_entries`) on a
machine without a GPU.

The same thunks that tests/test_gpu_tunables.py sweeps over every tunable value run here once through the `host_abi` fixture
(the product's `xgcm_amd.device` over libxgcm_host.so) and are compared bit for bit with their numpy references: the
arguments, their order, the shapes, the boundary rotation and the references themselves are checked before any GPU time is
spent on them.  The host build reads no tunable, so there is nothing to sweep here."""

import numpy as np
import pytest

import test_gpu_tunables as TT


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_one_pass_entries_equal_their_numpy_references(host_abi, dtype):
    import xgcm_amd.device as D

    entries = TT._one_pass_entries(D, dtype)
    # two nx, each: K7i and K7j with shared and own metrics, K7k in its five forms; one unweighted K7i and K7j call
    assert len(entries) == 20
    assert {k[:5] for k in entries} == {"pgrad", "vmadv", "hvisc"}
    for name, (thunk, reference) in entries.items():
        got = [D.tohost(x) for x in thunk()]
        want = reference()
        assert len(got) == len(want) == 2, name
        for g, w in zip(got, want):
            assert g.dtype == np.dtype(dtype), name
            if name.startswith("pgrad"):   # a NaN product counts as 0 in the running sum
                assert not np.isnan(w).any(), name
            else:                          # the NaN cells reach the result and stay local
                assert np.isnan(w).any() and np.isnan(w).mean() < 0.01, name
            assert TT._same_bits(g, w), name


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_early_entries_equal_their_numpy_references(host_abi, dtype):
    """`_early_entries`: K7d - K7h through the host build of the ABI; the fused vector operators and the two-axis stencil
    (which the host build does not have) on the oracle's double"""
    import xgcm_amd.device as D
    from oracle import fake_device

    entries = TT._early_entries(D, dtype, V=fake_device)
    two = ("grad", "flux", "madv", "madvu", "madv0")
    assert list(entries) == ["vort", "divg", "grad", "flux", "i2", "i2mw", "fdiv", "lap", "lapa", "madv", "fdivu", "lapu", "lapau",
                             "madvu", "madv0", "ke", "fdiv3", "fdiv3p", "wcont", "wcontr"]
    for name, (thunk, reference) in entries.items():
        got = thunk()
        got = [D.tohost(x) for x in got] if isinstance(got, tuple) else [D.tohost(got)]
        want = reference()
        assert len(got) == len(want) == (2 if name in two else 1), name
        for g, w in zip(got, want):
            assert g.dtype == np.dtype(dtype), name
            assert np.isfinite(w).all() and (w != 0).any(), name
            assert TT._same_bits(g, w), name


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_halo_entries_equal_their_numpy_references(host_abi, dtype):
    """`_halo_entries`: the two stencil forms through the host build of the ABI, the vector forms and the gather (for which
    the host build answers `unsupported`) on the oracle's double"""
    import test_halo_forms as TH
    import xgcm_amd.device as D
    from oracle import fake_device

    entries = TT._halo_entries(D, dtype, V=fake_device)
    assert len(entries) == 8 + 12 + 3
    assert {k[:5] for k in entries} == {"hvort", "hdive", "hgrad", "hflux", "hstwa", "hstwo", "hstod", "hsta0", "hsta1", "hsta2", "hgath"}
    for name, (thunk, reference) in entries.items():
        got = thunk()
        got = [D.tohost(x) for x in got] if isinstance(got, tuple) else [D.tohost(got)]
        want = reference()
        assert len(got) == len(want) == (2 if name[:5] in ("hgrad", "hflux") else 1), name
        for g, w in zip(got, want):
            assert g.dtype == np.dtype(dtype), name
            assert np.isnan(w).any() and np.isnan(w).mean() < 0.01, name
            assert TT._same_bits(g, w), name
    # the eight vector entries take the mode pairs in turn: between them every pair that contains a halo
    vector = [k for k in entries if k[:5] in ("hvort", "hdive", "hgrad", "hflux")]
    assert len(vector) == 8 and set((TH.PAIRS * 2)[:len(vector)]) == set(TH.PAIRS) and len(set(TH.PAIRS)) == 7


def test_the_entries_meet_every_boundary_mode_and_shape():
    """what the sweep relies on, stated over the tables: every K7i / K7j triple holds all three modes, the K7k pairs between
    them put each mode on each axis; ny is ragged against every band height, nx gives the vector and the narrow form"""
    modes = {"periodic", "extend", "fill"}
    assert all(set(p) == modes for p in TT.PADS_K7I + TT.PADS_K7J)
    assert all(p[2] in ("fill", "extend") for p in TT.PADS_K7I)   # K7i refuses a periodic Z
    assert {p[0] for p in TT.PADS_K7K} == {p[1] for p in TT.PADS_K7K} == modes and all(a != b for a, b in TT.PADS_K7K)
    nseg = (TT.OP_NY + 1) // 2
    assert TT.OP_NY % 2 == 1 and all(nseg % segs for segs in (2, 4, 8)) and nseg > 8
    assert TT.OP_NXS[0] % 4 == 0 and TT.OP_NXS[0] % 256 and TT.OP_NXS[0] % 128 and TT.OP_NXS[0] > 256
    assert TT.OP_NXS[1] % 2 == 1 and TT.OP_NXS[1] % 64 and TT.OP_NXS[1] > 256
