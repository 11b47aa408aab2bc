"""The pre-gathered halo forms on the HIP library, at kernel sizes: every case of tests/test_halo_forms.py through
`xgcm_amd.device`, bit for bit against the numpy statements there.

What the small faces of tests/test_topology.py and the shapes of tests/test_gpu_kernels.py never gave the halo branches of
`k_vorticity`, `k_divergence` and `k_pair2d`: a second tile (lane 0 takes its left neighbour itself, the others by DPP across
the seam), ZK = 2 and 4 level groups with a short last group that indexes the slabs by a repeated level, the band-major order,
a segment of one row, the float32 vector form, an unaligned row slab that drops the launch to V = 1; and for
`xg_stencil1d_halo` / `_halo_w` every kernel family with each metric form at a march of 300 rows and at odd rows.  Inputs cut
from NaN-filled allocations show a value taken from outside a field or a slab in the result."""

import itertools

import numpy as np
import pytest
import torch

import test_gpu_tunables as TT
import test_halo_forms as TH
from test_fused_layouts import ALIGNED, _contig, _strided

pytestmark = pytest.mark.gpu
DTYPES = [pytest.param(np.float64, id="f64"), pytest.param(np.float32, id="f32")]
SFX = {np.float64: "_f64", np.float32: "_f32"}


@pytest.fixture
def D():
    from xgcm_amd import device

    return device


@pytest.fixture
def fetched(D, monkeypatch):
    """the names of the entries fetched from the library, through a recorder on `D._MEM.lib()`"""
    rec = TT._Recorder(D._MEM.lib())
    monkeypatch.setattr(D._MEM, "lib", lambda: rec, raising=True)
    return rec.fetched


def _guarded(D, a):
    """`a` as a contiguous slice from the middle of a NaN-filled allocation, a multiple of 16 bytes in: the vector form stays"""
    t = _strided(D, a, _contig(a.shape), ALIGNED)
    assert t.is_contiguous() and t.data_ptr() % 16 == 0 and (ALIGNED * a.dtype.itemsize) % 16 == 0
    return t


# ---- vorticity / divergence / gradient / flux -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ny,nx", TH.SHAPES)
def test_vorticity_and_divergence_with_slabs(D, fetched, ny, nx, dtype):
    """the full product of shapes, leading dims, area forms and mode pairs; the `_halo` entry is the one fetched"""
    n = 0
    for lead in TH.LEADS:
        case = TH.VectorCase(ny, nx, lead, dtype)
        n += TH.check_vector_case(D, case, TH.curl_div_forms(case), D.tohost, fetched, D.asdevice)
    assert n == 7 * 2 * (4 + 4 + 5)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ny,nx", TH.SHAPES)
def test_gradient_and_flux_with_slabs(D, fetched, ny, nx, dtype):
    """gradient without metrics, with level-shared mx and my (banded) and with metrics of the field's own shape; flux"""
    n = 0
    for lead in TH.LEADS:
        case = TH.VectorCase(ny, nx, lead, dtype)
        n += TH.check_vector_case(D, case, TH.pair_forms(case), D.tohost, fetched, D.asdevice)
    assert n == 7 * 4 * 3


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,value", [("vec_zk", 1), ("vec_zk", 2), ("vec_zk", 4), ("vec_zb_rows", 8), ("vec_zb_rows", 32)])
def test_level_shared_area_under_every_level_group_and_band_height(D, name, value, dtype):
    """the level-shared area cases again with 1, 2 and 4 levels per wave-task (groups of 4 + 1 and 4 + 2, an odd last group
    of 2: `ok` repeats the last level and indexes both slabs with it) and with bands of 8 and 32 rows"""
    from xgcm_amd import _hip

    assert _hip.get_tunable("zband") == 1
    keep = _hip.get_tunable(name)
    _hip.set_tunable(name, value)
    try:
        for (ny, nx), lead in itertools.product(TH.SHAPES, TH.LEADS):
            case = TH.VectorCase(ny, nx, lead, dtype)
            forms = [(op, "shared", (case.area("shared"),)) for op in ("vorticity", "divergence")]
            assert forms[0][2][0].shape == (1,) * len(lead) + (ny, nx)
            TH.check_vector_case(D, case, forms, D.tohost, None, D.asdevice)
    finally:
        _hip.set_tunable(name, keep)


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_unaligned_row_slab_takes_the_scalar_form_and_computes_the_same(D, dtype):
    """`halo_y` as an HBM-resident contiguous slice one element into a larger allocation: the launch drops to V = 1"""
    case = TH.VectorCase(29, 260, (5,), dtype)
    for op, (bx, by) in itertools.product(("vorticity", "divergence", "gradient", "flux"), (("halo", "halo"), ("periodic", "halo"))):
        planes = {"gradient": (case.area("shared", 331), case.area("own", 332)), "flux": ()}.get(op, (case.area("shared"),))
        arrays = {k: D.asdevice(a) for k, a in case.sets[op].items()}
        hy = case.sets[op]["hy"]
        buf = torch.full((hy.size + 8,), float("nan"), dtype=arrays["hy"].dtype, device=arrays["hy"].device)
        off = buf[1:1 + hy.size].view(hy.shape)
        off.copy_(arrays["hy"])
        assert arrays["hy"].data_ptr() % 16 == 0 and off.is_contiguous() and off.data_ptr() % 16 != 0
        aligned = [D.tohost(x) for x in case.call(D, op, bx, by, planes, arrays)]
        moved = [D.tohost(x) for x in case.call(D, op, bx, by, planes, dict(arrays, hy=off))]
        for g, a, w in zip(moved, aligned, case.want(op, bx, by, planes)):
            TH.same_bits(g, a, f"{op} ({bx}, {by}): unaligned against aligned")
            TH.same_bits(g, w, f"{op} ({bx}, {by}): unaligned against numpy")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nx", [260, 259])
def test_guarded_fields_and_slabs(D, fetched, nx, dtype):
    """fields and slabs cut from the middle of NaN-filled allocations: a value from outside one of them poisons the result"""
    for lead in TH.LEADS:
        case = TH.VectorCase(29, nx, lead, dtype)
        guarded = {op: {k: _guarded(D, a) for k, a in case.sets[op].items()} for op in ("vorticity", "divergence", "pair")}
        guarded["gradient"] = guarded["flux"] = guarded["pair"]
        forms = list(TH.curl_div_forms(case)) + list(TH.pair_forms(case))
        for (op, form, planes), (bx, by) in itertools.product(forms, TH.PAIRS):
            fetched.clear()
            got = case.call(D, op, bx, by, planes, guarded[op])
            assert f"xg_{op}_halo{SFX[dtype]}" in fetched
            for g, w in zip(got, case.want(op, bx, by, planes)):
                TH.same_bits(D.tohost(g), w, f"{op} {case} {form} ({bx}, {by})")


# ---- stencil1d_halo / stencil1d_halo_w ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", TH.STENCIL_FIELDS, ids=str)
def test_stencil_with_slabs(D, fetched, shape, dtype):
    x, cases = TH.stencil_cases(shape, dtype)
    TH.check_stencil_cases(D, x, cases, D.tohost, D.asdevice(x), fetched)


@pytest.mark.parametrize("dtype", DTYPES)
def test_stencil_with_guarded_field_and_slabs(D, dtype):
    x, cases = TH.stencil_cases((3, 65, 131), dtype)
    xg = _guarded(D, x)
    for op, axis, lo, hi, halo, m_in, m_out, forms in cases:
        got = D.tohost(D.stencil1d_halo(op, xg, _guarded(D, halo), axis, lo, hi, m_out, m_in))
        TH.same_bits(got, TH.want_stencil(op, x, halo, axis, lo, hi, m_out, m_in), f"{op} axis {axis} ({lo}, {hi}) {forms}")


# ---- gather ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_cases(D, fetched, dtype):
    for k in range(len(TH.GATHER_CASES)):
        x, partner, args, want = TH.gather_case(k, dtype)
        TH.same_bits(D.tohost(D.gather(x, partner, *args)), want, f"gather case {k}")
    assert "xg_gather" + SFX[dtype] in fetched


# ---- refusals, before any launch ------------------------------------------------------------------------------------------
def test_refusals(D):
    from xgcm_amd import _hip

    case = TH.VectorCase(5, 6, (2,), np.float64)
    f = case.sets["vorticity"]
    hip = {k: D.asdevice(a) for k, a in f.items()}
    # a halo mode without its slab
    for call in (lambda: D.vorticity(f["u"], f["v"], None, "halo", "periodic"), lambda: D.divergence(f["u"], f["v"], None, "fill", "halo"),
                 lambda: D.gradient(f["t"], "halo", "halo", 0.0, 0.0, None, None, f["hx"], None),
                 lambda: D.flux(f["u"], f["v"], f["t"], "halo", "extend")):
        with pytest.raises(_hip.XgcmInvalidArgument):
            call()
    # the plain entries refuse a halo mode
    lib, shape, out = D._MEM.lib(), _hip.i64([2, 5, 6]), torch.zeros_like(hip["u"])
    for entry, bcx, bcy in itertools.product((lib.xg_vorticity_f64, lib.xg_divergence_f64), ("halo", "fill"), ("halo", "extend")):
        status = entry(hip["u"].data_ptr(), hip["v"].data_ptr(), None, None, out.data_ptr(), shape, 3, _hip.BC[bcx], 0.0, _hip.BC[bcy],
                       0.0, D._stream())
        assert (status == -1) == ("halo" in (bcx, bcy)) and status in (0, -1)
    # a slab of the wrong extent: (..., X) where (..., Y) belongs, one row too many, one cell short
    with pytest.raises((ValueError, RuntimeError)):
        D.vorticity(f["u"], f["v"], None, "halo", "halo", 0.0, 0.0, f["hy"], f["hy"])
    with pytest.raises((ValueError, RuntimeError)):
        D.flux(f["u"], f["v"], f["t"], "halo", "halo", 0.0, 0.0, f["hx"], np.zeros((3, 6)))
    with pytest.raises(ValueError, match="halo buffer has shape"):
        D.stencil1d_halo("diff", f["u"], np.zeros((2, 5, 2)), 2, 1, 0)
    with pytest.raises(ValueError, match="halo buffer has shape"):
        D.stencil1d_halo("diff", f["u"], np.zeros((2, 1, 5)), 1, 1, 0, None, f["v"])
    torch.cuda.synchronize()


# ---- Grid on connected faces that cross tiles -----------------------------------------------------------------------------
@pytest.mark.parametrize("conn", ["x2x", "x2y_rev", "cubed_sphere"])
@pytest.mark.parametrize("n,dtype", [pytest.param(132, np.float64, id="132-f64"), pytest.param(260, np.float32, id="260-f32")])
def test_grid_on_connected_faces_that_cross_tiles(fetched, conn, n, dtype):
    """`Grid.vorticity`, `divergence`, `gradient(metric_weighted=True)`, `flux` and `interp(metric_weighted=...)` on faces of
    more than one tile, three levels, per-face metrics, NaN cells on face edges, against numpy differences of the arrays
    padded by `oracle.topology.pad_face_connections`"""
    TH.check_grid_case(TH.connections()[conn], n, dtype)
    sfx = SFX[dtype]
    assert {"xg_vorticity_halo", "xg_divergence_halo", "xg_gradient_halo", "xg_flux_halo", "xg_stencil1d_halo_w", "xg_gather"} <= {
        k[:-4] for k in fetched if k.endswith(sfx)}
