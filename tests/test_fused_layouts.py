"""Layout paths of the six one-pass entries of the C ABI: xg_flux_divergence, xg_laplacian (K7d), xg_flux_divergence3d (K7e),
xg_vertical_velocity (K7f), xg_kinetic_energy (K7g), xg_momentum_advection (K7h).

Their launchers choose per call the lane width V (NV only when every field and output pointer is 16-byte aligned and
nx % NV == 0), the FORM of each metric load (`plane_vec_ok`: one aligned vector per lane, or element by element) and, for K7d /
K7h, the work order (band-major when every plane is shared by all outer indices).  `xgcm_amd.device` materializes every
non-contiguous metric before the launch, so the Grid never reaches the strided branches; the ABI documents broadcast strides and
is a product surface.  The table below therefore calls the entries DIRECTLY with views: every view lives in a buffer whose other
cells are NaN (a read outside the view shows up in the result), every case asserts the pointer / stride precondition of the form
it names and the branch it thereby requests (`_request`), and every result is compared bit for bit

  1. form (a) -- contiguous, aligned -- with the numpy oracle chain composed by the CPU suites' own helpers;
  2. every other form with the same entry on form (a) holding the same values.

Two legs: libxgcm_host.so (`host_abi`; checks the table and the host loops' stride handling without a GPU) and
libxgcm_hip.so (marked gpu).  The Grid-level cases at the end give the Grid metrics in layouts it has to reorder itself."""

import types

import numpy as np
import pytest
import torch

import test_flux_divergence_3d as T3
import test_momentum_advection as TM
import test_vertical_velocity as TV
from oracle import refimpl as R
from test_fused_second_order import _want_flux_div, _want_laplacian
from xgcm_amd import DataArray, Dataset, Grid, _hip

NVS = {np.float64: 2, np.float32: 4}          # elements per 16-byte lane vector
SFX = {np.float64: "f64", np.float32: "f32"}
TORCH = {np.float64: torch.float64, np.float32: torch.float32}
# several wave tiles (64 lanes x NV columns) with a partial last one, a partial 2-row segment, more than one 8-row and one
# 16-row band with a partial last band, outer >= 2; nz = 5 is longer than K7f's 3-level window and no multiple of it
WIDE = {np.float64: 260, np.float32: 516}
OUTER2, OUTER3, NZ, NY = 3, 2, 5, 19
PADS = [("periodic", "extend"), ("fill", "periodic"), ("extend", "fill")]
PADS_Z = ["extend", "fill", "periodic"]                                  # K7e: one Z boundary per pair
PADS_W = [("fill", False), ("extend", False), ("periodic", True)]        # K7f: (Z boundary, reverse) per pair
FILL = {"X": 1.75, "Y": -0.625, "Z": 0.375}                              # (the oracle helpers' own fill values)
assert FILL["X"] == TM.FILL["X"] and FILL == T3.FILL == TV.FILL
ALIGNED = 16                                                             # elements in front of an aligned view (64 / 128 B)
ODD_FORMS = ["b", "c", "c2", "d", "ex", "ey", "e0", "f", "g"]           # 2-D planes; 3-D planes: + "h"


@pytest.fixture(params=["host_abi", pytest.param("hip", marks=pytest.mark.gpu)])
def leg(request):
    """the library under test behind `xgcm_amd.device._MEM`: the host build (CPU) or the HIP build (GPU)"""
    if request.param == "host_abi":
        request.getfixturevalue("host_abi")
    return request.param


# ---- views ---------------------------------------------------------------------------------------------------------------
def _strided(D, values, strides, offset):
    """`values` laid out with `strides` (elements), `offset` elements into a NaN-filled allocation"""
    t = torch.from_numpy(np.array(values, order="C"))
    span = offset + sum((n - 1) * s for n, s in zip(t.shape, strides)) + 1
    buf = torch.full((span + ALIGNED,), float("nan"), dtype=t.dtype, device=D._MEM.device)
    assert buf.data_ptr() % 16 == 0
    view = buf.as_strided(tuple(t.shape), tuple(strides), offset)
    view.copy_(t)
    return view


def _contig(shape):
    st, n = [], 1
    for s in reversed(shape):
        st.insert(0, n)
        n *= s
    return st


def _lay(D, a, form, core, nv):
    """(view, values): the plane `a` (lead + core dims, lead extent 1 or the fields') in the layout `form` names, inside NaN
    poison, with the form's precondition asserted; `values` is what the view holds (forms (e) repeat one row / column / cell)"""
    shape = list(a.shape)
    ny, nx = shape[-2:]
    item = a.dtype.itemsize
    if form in ("ex", "ey", "e0"):   # (e) stride 0 along a full-extent dim: X only / Y only / one value per level
        cut = {"ex": a[..., :1, :], "ey": a[..., :, :1], "e0": a[..., :1, :1]}[form]
        stored = _strided(D, cut, _contig(cut.shape), ALIGNED)
        view = stored.expand(*shape)
        assert view.data_ptr() % 16 == 0
        assert (view.stride(-2) == 0 or form == "ey" or ny == 1) and (view.stride(-1) == 0 or form == "ex" or nx == 1)
        return view, np.ascontiguousarray(np.broadcast_to(cut, shape))
    st, off = _contig(shape), ALIGNED
    if form in ("a", "f"):           # (a) the control; (f): one plane per outer index, contiguous
        pass
    elif form == "b":                # (b) contiguous, one element into its allocation
        off = 1
    elif form in ("c", "c2"):        # (c) aligned base, row pitch nx + 1 (float32 also nx + 2: even, no multiple of 4)
        pitch = nx + (1 if form == "c" else 2)
        st = _contig(shape[:-1] + [pitch])
    elif form == "d":                # (d) stored transposed: X stride ny
        st = _contig(shape[:-2] + [nx, ny])
        st[-2], st[-1] = st[-1], st[-2]
    elif form == "g":                # (g) one plane per outer index, level pitch (core size) + 1
        n = int(np.prod(shape[-core:]))
        st = [(n + 1) * s for s in _contig(shape[:-core])] + _contig(shape[-core:])
    elif form == "h":                # (h) 3-D planes: Z stride ny * nx + 1
        assert core == 3
        st = [(ny * nx + 1) * s for s in _contig(shape[:-2])] + [nx, 1]
    else:
        raise AssertionError(form)
    view = _strided(D, a, st, off)
    if form in ("a", "f"):
        assert view.is_contiguous() and view.data_ptr() % 16 == 0 and view.storage_offset() % nv == 0
    elif form == "b":
        assert view.is_contiguous() and view.storage_offset() == 1 and view.data_ptr() % 16 == item
    elif form in ("c", "c2"):
        assert view.data_ptr() % 16 == 0 and view.stride(-1) == 1 and view.stride(-2) == nx + (1 if form == "c" else 2)
    elif form == "d":
        assert view.data_ptr() % 16 == 0 and view.stride(-1) == ny and view.stride(-2) == 1
    elif form == "g":
        assert view.data_ptr() % 16 == 0 and view.stride(-core - 1) == int(np.prod(shape[-core:])) + 1 and shape[-core - 1] > 1
        assert list(view.stride()[-core:]) == _contig(shape[-core:])
    elif form == "h":
        assert view.data_ptr() % 16 == 0 and view.stride(-3) == ny * nx + 1 and list(view.stride()[-2:]) == [nx, 1]
    return view, np.ascontiguousarray(a)


def _abi_strides(view, shape):
    """broadcast strides against `shape` as the ABI takes them: 0 where the plane has extent 1"""
    assert all(m in (1, s) for m, s in zip(view.shape, shape))
    return [0 if m == 1 else view.stride(d) for d, m in enumerate(view.shape)]


def _vec_ok(view, strides, core, nv):
    """the launcher's `plane_vec_ok` (and the Z stride test of the 3-D kernels), restated for the assertions"""
    lead = strides[:-core] + ([strides[-3]] if core == 3 else [])
    return strides[-1] == 1 and strides[-2] % nv == 0 and view.data_ptr() % 16 == 0 and all(s % nv == 0 for s in lead)


# ---- the six entries ------------------------------------------------------------------------------------------------------
class Entry:
    def __init__(self, name, fields, planes, core, nout=1, zonly=(), banded=False):
        self.name, self.fields, self.planes, self.core, self.nout = name, fields, planes, core, nout
        self.zonly, self.banded = zonly, banded   # planes that vary along Z only; does the launcher have a band-major order?


FLUXDIV = Entry("xg_flux_divergence", ("u", "v", "t"), ("area",), 2, banded=True)
LAPLACE = Entry("xg_laplacian", ("t",), ("dxC", "dyC", "dyG", "dxG", "area"), 2, banded=True)
DIV3D = Entry("xg_flux_divergence3d", ("u", "v", "w", "t"), ("vol", "vol2"), 3)
WCONT = Entry("xg_vertical_velocity", ("u", "v"), ("mu", "mu2", "mv", "mv2", "area"), 3, zonly=("mu2", "mv2"))
KINETIC = Entry("xg_kinetic_energy", ("u", "v"), (), 2)
MOMADV = Entry("xg_momentum_advection", ("u", "v"), ("coriolis", "rAz", "dxC", "dyC"), 2, nout=2, banded=True)
SEEDS = {n: 101 + k for k, n in enumerate(("u", "v", "w", "t", "area", "dxC", "dyC", "dyG", "dxG", "vol", "vol2", "mu", "mu2",
                                           "mv", "mv2", "coriolis", "rAz"))}
_VALUES = {}    # (entry, dtype, nx) -> the inputs, made once
_CONTROL = {}   # (leg, entry, dtype, nx, boundary index, planes present, planes varying per outer / cut by (e)) -> results
_REQUESTED = {}  # entry name -> {(V == NV, vector-form flag per plane present, band-major)}: what the cases asked for


def _shape(e, dtype, nx):
    return ((OUTER2, NY, nx) if e.core == 2 else (OUTER3, NZ, NY, nx))


def _values(e, dtype, nx):
    key = (e.name, dtype, nx)
    if key not in _VALUES:
        shape = _shape(e, dtype, nx)
        vals = {f: R.synthetic_field(shape, SEEDS[f]).astype(dtype) for f in e.fields}
        for p in e.planes:
            pshape = shape if p not in e.zonly else (shape[0], NZ, 1, 1)   # [0]: shared by the outer indices; all: per outer
            m = (R.synthetic_field(pshape, SEEDS[p]) * 3.0) if p == "coriolis" else R.synthetic_metric(pshape, SEEDS[p])
            vals[p] = m.astype(dtype)
        _VALUES[key] = vals
    return _VALUES[key]


def _oracle(e, f, m, px, py, k):
    """the numpy oracle chain of entry `e` over fields `f` and plane values `m` (absent: None), as the CPU suites compose it"""
    if e is FLUXDIV:
        return (_want_flux_div(f["u"], f["v"], f["t"], px, py, 1.0 if m["area"] is None else m["area"]),)
    if e is LAPLACE:
        if m["dxC"] is None and m["area"] is None:
            return (_want_laplacian(f["t"], px, py, None),)
        one = np.ones((), dtype=f["t"].dtype)   # (x / 1 and x * 1 are exact: the chain with only some of its planes)
        met = {k_: (one if m[k_] is None else m[k_]) for k_ in ("dxC", "dyC", "dyG", "dxG")}
        met["rA"] = one if m["area"] is None else m["area"]
        return (_want_laplacian(f["t"], px, py, met),)
    if e is DIV3D:
        vol = m["vol"] if m["vol2"] is None else R.binary("mul", m["vol"], m["vol2"])
        return (T3._want(f["u"], f["v"], f["w"], f["t"], px, py, PADS_Z[k], vol),)
    if e is WCONT:
        pz, rev = PADS_W[k]
        faces = None
        if m["mu"] is not None:
            faces = tuple(a if b is None else R.binary("mul", a, b) for a, b in ((m["mu"], m["mu2"]), (m["mv"], m["mv2"])))
        return (TV._want(f["u"], f["v"], px, py, pz, rev, faces=faces, area=m["area"]),)
    if e is KINETIC:
        return (TM._want_ke(f["u"], f["v"], px, py),)
    ds = None if m["rAz"] is None else {p: types.SimpleNamespace(values=m[p]) for p in ("rAz", "dxC", "dyC")}
    return TM._want(f["u"], f["v"], px, py, ds, m["coriolis"])


def _launch(D, e, dtype, shape, fields, planes, k):
    """one call of the entry: `fields` / `planes` are views (a plane None: absent); returns its results as numpy arrays"""
    px, py = PADS[k]
    args = [fields[f].data_ptr() for f in e.fields]
    for p in e.planes:
        v = planes.get(p)
        args += [None, None] if v is None else [v.data_ptr(), _hip.i64(_abi_strides(v, shape))]
    # poison the allocator's next block so that an unwritten output cell cannot pass by luck
    junk = [torch.full(shape, float("nan"), dtype=TORCH[dtype], device=D._MEM.device) for _ in range(e.nout)]
    del junk
    outs = [D._empty(shape, TORCH[dtype], D._MEM.device) for _ in range(e.nout)]
    assert all(o.data_ptr() % 16 == 0 for o in outs)
    args += [o.data_ptr() for o in outs] + [_hip.i64(shape), len(shape), _hip.BC[px], FILL["X"], _hip.BC[py], FILL["Y"]]
    if e is DIV3D:
        args += [_hip.BC[PADS_Z[k]], FILL["Z"]]
    if e is WCONT:
        args += [_hip.BC[PADS_W[k][0]], FILL["Z"], int(PADS_W[k][1])]
    D._check(getattr(D._MEM.lib(), e.name + "_" + SFX[dtype])(*args, D._stream()))
    return tuple(o.cpu().numpy() for o in outs)


def _request(e, dtype, shape, fields, planes):
    """the branch this call asks the launcher for, from the pointers and strides alone (recorded per entry)"""
    nv = NVS[dtype]
    wide = shape[-1] % nv == 0 and all(v.data_ptr() % 16 == 0 for v in fields.values())
    present = [p for p in e.planes if planes.get(p) is not None and p not in e.zonly]
    vec = tuple(wide and _vec_ok(planes[p], _abi_strides(planes[p], shape), e.core, nv) for p in present)
    shared = all(all(s == 0 for s in _abi_strides(planes[p], shape)[:-2]) for p in present)
    req = (wide, vec, bool(e.banded and present and shared))
    _REQUESTED.setdefault((e.name, dtype, shape[-1]), set()).add(req)
    return req


def _case(leg, e, dtype, nx, k, forms=None, present=None, misaligned=()):
    """Run entry `e` under boundary pair `k` with the planes `present` (default: all) laid out as `forms` names them (default
    (a)) and the fields `misaligned` one element into their allocations; compare with the control -- the same entry, the
    same values, everything in form (a) -- which is itself compared with the oracle chain the first time it is made."""
    import xgcm_amd.device as D

    nv = NVS[dtype]
    forms = dict(forms or {})
    present = e.planes if present is None else present
    shape = _shape(e, dtype, nx)
    base = _values(e, dtype, nx)
    vals, views = {}, {}
    for p in e.planes:
        if p not in present:
            vals[p] = None
            continue
        form = forms.get(p, "a")
        a = base[p] if form in ("f", "g") else base[p][:1]
        views[p], vals[p] = _lay(D, a, form, e.core, nv)
    variant = tuple((p, forms[p]) for p in e.planes if forms.get(p) in ("f", "g", "ex", "ey", "e0"))
    variant = tuple((p, "f" if fm == "g" else fm) for p, fm in variant)
    key = (leg, e.name, dtype, nx, k, tuple(present), variant)
    if key not in _CONTROL:
        cf = {f: _lay(D, base[f], "a", e.core, nv)[0] for f in e.fields}
        cp = {p: _lay(D, vals[p], "a", e.core, nv)[0] for p in present}
        req = _request(e, dtype, shape, cf, cp)
        if nx % nv == 0:
            assert req[0] and all(req[1])        # the control: V = NV, every plane in the vector form
        got = _launch(D, e, dtype, shape, cf, cp, k)
        want = _oracle(e, {f: base[f] for f in e.fields}, vals, *PADS[k], k)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype == np.dtype(dtype) and g.shape == w.shape
            assert np.array_equal(g, w, equal_nan=True), f"{e.name} control {key}: differs from the oracle chain"
        _CONTROL[key] = got
    control = _CONTROL[key]
    if not forms and not misaligned:
        return
    fviews = {f: _lay(D, base[f], "b" if f in misaligned else "a", e.core, nv)[0] for f in e.fields}
    req = _request(e, dtype, shape, fviews, views)
    if nx % nv == 0:   # (else V = 1 whatever the pointers are)
        assert req[0] == (not misaligned)
        for p, ok in zip([p for p in present if p not in e.zonly], req[1]):
            odd = forms.get(p, "a") not in ("a", "f", "ex")   # (a row shared by all Y is still one aligned vector per lane)
            assert ok == (not odd and not misaligned), f"{p} in form {forms.get(p, 'a')}: vector form {ok}"
    got = _launch(D, e, dtype, shape, fviews, views, k)
    for g, w in zip(got, control):
        if not np.array_equal(g, w, equal_nan=True):
            bad = np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))
            raise AssertionError(f"{e.name} {np.dtype(dtype)} nx {nx} {PADS[k]} forms {forms} misaligned {misaligned}: "
                                 f"{len(bad)} cells differ from the control, first {bad[:6].tolist()}, NaN {int(np.isnan(g).sum())}")


def _forms(e, dtype):
    out = [f for f in ODD_FORMS if f != "c2" or dtype is np.float32]
    return out + (["h"] if e.core == 3 else [])


def _plane_table(leg, e, dtype, nx, groups, present=None):
    """every form for every group of planes (a plane alone while the others stay (a), or several together), under every
    boundary pair"""
    for k in range(len(PADS)):
        _case(leg, e, dtype, nx, k, present=present)
        for group in groups:
            for n, form in enumerate(_forms(e, dtype)):
                planes = group(n) if callable(group) else group
                _case(leg, e, dtype, nx, k, {p: form for p in planes}, present=present)


def _asked(e, dtype, nx):
    return _REQUESTED[(e.name, dtype, nx)]


NXS = ["wide", 1, 2]   # nx = 1: a single lane; nx = 2: a single vector (float64) / below one (float32)
both = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
sizes = pytest.mark.parametrize("nx", NXS)


def _nx(nx, dtype):
    return WIDE[dtype] if nx == "wide" else nx


@both
@sizes
def test_flux_divergence_area_forms(leg, dtype, nx):
    nx = _nx(nx, dtype)
    _plane_table(leg, FLUXDIV, dtype, nx, [("area",)])
    for k in range(len(PADS)):
        _case(leg, FLUXDIV, dtype, nx, k, present=())   # no area at all
    if nx % NVS[dtype] == 0:
        asked = _asked(FLUXDIV, dtype, nx)
        assert (True, (False,), True) in asked and (True, (False,), False) in asked   # element-wise under V = NV, both orders
        assert (True, (True,), True) in asked and (True, (True,), False) in asked     # vector form, both orders


@both
@sizes
def test_laplacian_plane_forms(leg, dtype, nx):
    """K7d's four metric planes share one all-or-nothing bit, the area has its own: the area alone in each form, one metric
    plane alone (a different one per form), then all five; and the area as the only plane"""
    nx = _nx(nx, dtype)
    mets = ("dxC", "dyC", "dyG", "dxG")
    _plane_table(leg, LAPLACE, dtype, nx, [("area",), lambda n: (mets[n % 4],), LAPLACE.planes])
    _plane_table(leg, LAPLACE, dtype, nx, [("area",)], present=("area",))
    _plane_table(leg, LAPLACE, dtype, nx, [mets], present=mets)
    for k in range(len(PADS)):
        _case(leg, LAPLACE, dtype, nx, k, present=())
    if nx % NVS[dtype] == 0:
        asked = _asked(LAPLACE, dtype, nx)
        mixed = [r for r in asked if r[0] and len(r[1]) == 5 and any(r[1]) and not all(r[1])]
        assert any(not r[1][4] for r in mixed) and any(r[1][4] for r in mixed)       # area odd alone / one metric odd alone
        assert {r[2] for r in mixed} == {True, False}                                 # per-plane mixed forms, both orders
        assert any(r[0] and not any(r[1]) and len(r[1]) == 5 for r in asked)          # all five element-wise under V = NV


@both
@sizes
def test_momentum_advection_plane_forms(leg, dtype, nx):
    """K7h: coriolis, rAz, dxC, dyC under one bit: one plane alone in each form (a different one per form), then all; the
    coriolis plane alone and the three metrics without it"""
    nx = _nx(nx, dtype)
    _plane_table(leg, MOMADV, dtype, nx, [lambda n: (MOMADV.planes[n % 4],), lambda n: (MOMADV.planes[(n + 2) % 4],),
                                          MOMADV.planes])
    _plane_table(leg, MOMADV, dtype, nx, [("coriolis",)], present=("coriolis",))
    _plane_table(leg, MOMADV, dtype, nx, [lambda n: (MOMADV.planes[1 + n % 3],)], present=MOMADV.planes[1:])
    for k in range(len(PADS)):
        _case(leg, MOMADV, dtype, nx, k, present=())
    if nx % NVS[dtype] == 0:
        asked = _asked(MOMADV, dtype, nx)
        mixed = [r for r in asked if r[0] and len(r[1]) == 4 and any(r[1]) and not all(r[1])]
        assert {r[2] for r in mixed} == {True, False}
        assert {r[2] for r in asked if r[0] and len(r[1]) == 4 and all(r[1])} == {True, False}


@both
@sizes
def test_flux_divergence_3d_plane_forms(leg, dtype, nx):
    """K7e: each volume factor has its own bit: each alone in each form, then both; one factor only"""
    nx = _nx(nx, dtype)
    _plane_table(leg, DIV3D, dtype, nx, [("vol",), ("vol2",), DIV3D.planes])
    _plane_table(leg, DIV3D, dtype, nx, [("vol",)], present=("vol",))
    for k in range(len(PADS)):
        _case(leg, DIV3D, dtype, nx, k, present=())
    if nx % NVS[dtype] == 0:
        assert {r[1] for r in _asked(DIV3D, dtype, nx) if r[0] and len(r[1]) == 2} == {(True, True), (True, False),
                                                                                        (False, True), (False, False)}


@both
@sizes
def test_vertical_velocity_plane_forms(leg, dtype, nx):
    """K7f: u's and v's first face-weight factor and the area have a bit each: each alone in each form, then all three; the
    second factors vary along Z only (contiguous, and with a Z step of 3 elements); no face weights; no area"""
    import xgcm_amd.device as D

    nx = _nx(nx, dtype)
    _plane_table(leg, WCONT, dtype, nx, [("mu",), ("mv",), ("area",), ("mu", "mv", "area")])
    _plane_table(leg, WCONT, dtype, nx, [lambda n: (("mu", "mv")[n % 2],)], present=("mu", "mv"))
    _plane_table(leg, WCONT, dtype, nx, [("area",)], present=("area",))
    shape = _shape(WCONT, dtype, nx)
    base = _values(WCONT, dtype, nx)
    for k in range(len(PADS)):
        _case(leg, WCONT, dtype, nx, k, present=())
        # the Z-only factors 3 elements apart, inside poison
        control = _CONTROL[(leg, WCONT.name, dtype, nx, k, WCONT.planes, ())]
        fields = {f: _lay(D, base[f], "a", 3, NVS[dtype])[0] for f in WCONT.fields}
        planes = {p: _lay(D, base[p][:1], "a", 3, NVS[dtype])[0] for p in ("mu", "mv", "area")}
        for p in WCONT.zonly:
            planes[p] = _strided(D, base[p][:1], [3 * NZ, 3, 1, 1], 1)
            assert planes[p].stride(1) == 3 and planes[p].storage_offset() == 1
        got = _launch(D, WCONT, dtype, shape, fields, planes, k)
        assert np.array_equal(got[0], control[0], equal_nan=True)
    if nx % NVS[dtype] == 0:
        seen = {r[1] for r in _asked(WCONT, dtype, nx) if r[0] and len(r[1]) == 3}
        assert {(True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False)} <= seen


@both
@sizes
@pytest.mark.parametrize("e", [FLUXDIV, LAPLACE, DIV3D, WCONT, KINETIC, MOMADV], ids=lambda e: e.name)
def test_misaligned_fields(leg, e, dtype, nx):
    """V must drop to 1 for ALL fields when any one of them starts off a 16-byte boundary: all fields one element into
    their allocations (V = 1 with an even nx over several tiles), each field alone, and the metrics in forms (a) and (d)
    under misaligned fields"""
    nx = _nx(nx, dtype)
    for k in range(len(PADS)):
        _case(leg, e, dtype, nx, k, misaligned=e.fields)
        for f in e.fields:
            _case(leg, e, dtype, nx, k, misaligned=(f,))
        if e.planes:
            odd = [p for p in e.planes if p not in e.zonly]
            _case(leg, e, dtype, nx, k, {p: "d" for p in odd}, misaligned=e.fields)
            _case(leg, e, dtype, nx, k, {p: "d" for p in odd}, misaligned=e.fields[:1])
            _case(leg, e, dtype, nx, k, {p: "f" for p in odd}, misaligned=e.fields[-1:])   # V = 1, plain work order
    if nx % NVS[dtype] == 0:
        asked = _asked(e, dtype, nx)
        assert any(not r[0] for r in asked) and any(r[0] for r in asked)   # V = 1 with nx a multiple of NV, and V = NV
        if e.banded:
            assert {r[2] for r in asked if not r[0]} == {True, False}      # V = 1 in both work orders


# ---- Grid level -----------------------------------------------------------------------------------------------------------
AXES = {"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"}}
NAMES = {"dxC": ("YC", "XG"), "dyG": ("YC", "XG"), "dyC": ("YG", "XC"), "dxG": ("YG", "XC"), "rA": ("YC", "XC"),
         "rAz": ("YG", "XG"), "f": ("YG", "XG")}
GRID_METRICS = {("X",): ["dxC", "dxG"], ("Y",): ["dyC", "dyG"], ("X", "Y"): ["rA", "rAz"]}
FUSED = ("flux_divergence", "laplacian", "kinetic_energy", "momentum_advection")
CHAIN = ("flux", "gradient", "divergence", "vorticity", "binary", "stencil1d")


class _Calls:
    """counts the calls of the one-pass device entries and of the chain's while the `with` block runs"""

    def __enter__(self):
        import xgcm_amd.device as D

        self.patch = pytest.MonkeyPatch()
        self.n = dict.fromkeys(FUSED + CHAIN, 0)
        for name in self.n:
            self.patch.setattr(D, name, self._counted(getattr(D, name), name))
        return self

    def __exit__(self, *exc):
        self.patch.undo()

    def _counted(self, fn, name):
        def wrapped(*a, **k):
            self.n[name] += 1
            return fn(*a, **k)
        return wrapped

    def fused_only(self, **want):
        assert {k: v for k, v in self.n.items() if v} == want, self.n


def _coords(lead, ny, nx):
    c = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0), "YC": ("YC", np.arange(ny) + 0.5),
         "YG": ("YG", np.arange(ny) * 1.0)}
    if lead:
        c["time"] = ("time", np.arange(lead) * 2.0)
    return c


def _metric_values(ny, nx, dtype, lead=0):
    shape = ((lead,) if lead else ()) + (ny, nx)
    out = {k: R.synthetic_metric(shape, 61 + n).astype(dtype) for n, k in enumerate(("dxC", "dyG", "dyC", "dxG", "rA", "rAz"))}
    out["f"] = (R.synthetic_field(shape, 68) * 3.0).astype(dtype)
    return out


def _grid_of(data, lead, ny, nx, pad):
    ds = Dataset(data, _coords(lead, ny, nx))
    return Grid(ds, coords=AXES, metrics=GRID_METRICS, padding={"X": pad[0], "Y": pad[1]}, autoparse_metadata=False), ds


def _grid_fields(lead, ny, nx, dtype, put):
    shape = (lead, ny, nx)
    mk = lambda seed, dims: DataArray(put(R.synthetic_field(shape, seed).astype(dtype)), ("time",) + dims)  # noqa: E731
    return mk(72, ("YC", "XG")), mk(73, ("YG", "XC")), mk(71, ("YC", "XC"))


def _all_fused(grid, ds, u, v, t, f="f"):
    cor = ds[f] if isinstance(f, str) else f
    return (grid.flux_divergence(u, v, t, fill_value=FILL), grid.laplacian(t, fill_value=FILL),
            grid.kinetic_energy(u, v, fill_value=FILL), *grid.momentum_advection(u, v, cor, fill_value=FILL))


def _host(x):
    d = x.data
    return d.cpu().numpy() if isinstance(d, torch.Tensor) else np.asarray(d)


def _same_results(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert tuple(g.dims) == tuple(w.dims) and type(g.data) is type(w.data)
        gh, wh = _host(g), _host(w)
        assert gh.dtype == wh.dtype and np.array_equal(gh, wh, equal_nan=True)


def _puts(leg):
    """how the inputs reach the Grid: host numpy, and (HIP leg) HBM-resident"""
    return [lambda a: a] + ([lambda a: torch.from_numpy(np.array(a, order="C")).cuda()] if leg == "hip" else [])


GRID_SHAPE = {np.float64: (3, 19, 132), np.float32: (3, 19, 136)}


@both
def test_grid_metrics_stored_in_x_y_order(leg, dtype):
    """every metric (and the coriolis parameter) stored with its dims in (X, Y) order: the one-pass entries still run, once
    each, with the results of the same grid built from plain (Y, X) metrics"""
    lead, ny, nx = GRID_SHAPE[dtype]
    vals = _metric_values(ny, nx, dtype)
    for put in _puts(leg):
        for pad in PADS:
            plain, pds = _grid_of({k: (NAMES[k], put(a)) for k, a in vals.items()}, lead, ny, nx, pad)
            turned, tds = _grid_of({k: (NAMES[k][::-1], put(np.ascontiguousarray(a.T))) for k, a in vals.items()}, lead, ny, nx, pad)
            u, v, t = _grid_fields(lead, ny, nx, dtype, put)
            want = _all_fused(plain, pds, u, v, t)
            with _Calls() as calls:
                _same_results(_all_fused(turned, tds, u, v, t), want)
            calls.fused_only(flux_divergence=1, laplacian=1, kinetic_energy=1, momentum_advection=1)


@both
def test_grid_coriolis_of_one_axis_or_none(leg, dtype):
    """coriolis as f(XG) alone, f(YG) alone and a 0-d value: one pass with broadcast strides, equal to the full plane that
    repeats those values"""
    lead, ny, nx = GRID_SHAPE[dtype]
    vals = _metric_values(ny, nx, dtype)
    fx, fy, f0 = vals["f"][3], vals["f"][:, 5], vals["f"][2, 7]
    for put in _puts(leg):
        grid, ds = _grid_of({k: (NAMES[k], put(a)) for k, a in vals.items()}, lead, ny, nx, PADS[0])
        u, v, t = _grid_fields(lead, ny, nx, dtype, put)
        for small, dims, full in ((fx, ("XG",), np.broadcast_to(fx, (ny, nx))), (fy, ("YG",), np.broadcast_to(fy[:, None], (ny, nx))),
                                  (np.asarray(f0), (), np.broadcast_to(f0, (ny, nx)))):
            want = grid.momentum_advection(u, v, DataArray(put(np.ascontiguousarray(full)), ("YG", "XG")), fill_value=FILL)
            with _Calls() as calls:
                got = grid.momentum_advection(u, v, DataArray(put(np.array(small)), dims), fill_value=FILL)
            calls.fused_only(momentum_advection=1)
            _same_results(got, want)


@both
def test_grid_metrics_sliced_out_of_larger_arrays(leg, dtype):
    """metrics that are views of a larger array -- starting one element in, and with an odd row pitch -- HBM-resident on the
    HIP leg: the one-pass entries run on them and give the plain grid's results"""
    lead, ny, nx = GRID_SHAPE[dtype]
    vals = _metric_values(ny, nx, dtype)

    def offset_view(put, a):
        big = np.full(a.size + 1, np.nan, dtype=a.dtype)
        big[1:] = a.reshape(-1)
        view = put(big)[1:].reshape(ny, nx)
        if isinstance(view, torch.Tensor):
            assert view.storage_offset() == 1 and view.data_ptr() % 16 != 0
        return view

    def pitch_view(put, a):
        big = np.full((ny + 2, nx + 3), np.nan, dtype=a.dtype)
        big[1:-1, 2:-1] = a
        view = put(big)[1:-1, 2:-1]
        if isinstance(view, torch.Tensor):
            assert view.stride(0) == nx + 3 and not view.is_contiguous()
        else:
            assert view.strides[0] == (nx + 3) * a.itemsize
        return view

    for put in _puts(leg):
        plain, pds = _grid_of({k: (NAMES[k], put(a)) for k, a in vals.items()}, lead, ny, nx, PADS[1])
        u, v, t = _grid_fields(lead, ny, nx, dtype, put)
        want = _all_fused(plain, pds, u, v, t)
        for cut in (offset_view, pitch_view):
            grid, ds = _grid_of({k: (NAMES[k], cut(put, a)) for k, a in vals.items()}, lead, ny, nx, PADS[1])
            with _Calls() as calls:
                _same_results(_all_fused(grid, ds, u, v, t), want)
            calls.fused_only(flux_divergence=1, laplacian=1, kinetic_energy=1, momentum_advection=1)


@both
def test_grid_metrics_with_a_leading_dim_the_fields_share(leg, dtype):
    """metrics and coriolis of (time, Y, X) under (time, Y, X) fields: one pass with non-zero leading strides (the plain work
    order), equal level by level to the grid whose metrics are that level's (Y, X) planes"""
    lead, ny, nx = GRID_SHAPE[dtype]
    vals = _metric_values(ny, nx, dtype, lead)
    for put in _puts(leg):
        for pad in PADS:
            grid, ds = _grid_of({k: (("time",) + NAMES[k], put(a)) for k, a in vals.items()}, lead, ny, nx, pad)
            u, v, t = _grid_fields(lead, ny, nx, dtype, put)
            with _Calls() as calls:
                got = _all_fused(grid, ds, u, v, t)
            calls.fused_only(flux_divergence=1, laplacian=1, kinetic_energy=1, momentum_advection=1)
            for lev in range(lead):
                one, ods = _grid_of({k: (NAMES[k], put(a[lev])) for k, a in vals.items()}, 1, ny, nx, pad)
                cut = [DataArray(put(np.ascontiguousarray(_host(x)[lev:lev + 1])), x.dims) for x in (u, v, t)]
                want = _all_fused(one, ods, *cut)
                for g, w in zip(got, want):
                    assert np.array_equal(_host(g)[lev:lev + 1], _host(w), equal_nan=True)
