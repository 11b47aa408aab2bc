"""The ten early one-pass operators against plain numpy, bit for bit, on both libraries.

K7d `flux_divergence` / `laplacian`, K7e `flux_divergence_3d`, K7f `vertical_velocity`, K7g `kinetic_energy`, K7h
`momentum_advection`, K7i `hydrostatic_pressure_gradient`, K7j `vertical_momentum_advection`, K7k `horizontal_viscosity` and
K7l `vertical_diffusion` promise the bits of the chain they replace.  Their GPU suites compare them with that chain run through
the same library, the same boundary loads and the same Python plan; here the reference is the numpy statement of each
operator's CPU suite (imported, not restated) and the comparison is `test_richardson_number._same_bits`: NaN where numpy has
NaN, the same bit pattern everywhere else, so that -0.0 is not +0.0.

Two legs (the `leg` fixture): libxgcm_host.so, which makes the tables checkable without a GPU and keeps the statements honest,
and libxgcm_hip.so (marked gpu), which is the point.  Every case runs twice: through `Grid`, and directly through
`xgcm_amd.device.<operator>` on arrays laid out from the statement's own inputs with the fill values passed as floats -- a
loss in the Python plan and a loss in the kernel show up apart.  Both calls are counted on the one-pass entry while the chain's
device functions are barred, so no case passes by falling back.

Every table returns the number of its SOLID cases -- the numpy result holds a finite non-zero value (and a NaN, where NaNs
were planted) -- and each test asserts that number against a constant computed from the numpy statements alone.  For
all-zero inputs, whose results are zeros, NaNs and whatever a finite fill value leaves, a case is also solid when the numpy
result holds zeros of BOTH signs: that is what makes the sign comparison see anything.

Cases the operators hand to the chain by design are not in the tables: a single column (ny * nx == 1) for K7f and K7i, and for
K7f a periodic Z, or one level under `extend`, without `reverse`."""

import itertools
import types

import numpy as np
import pytest

import test_flux_divergence_3d as T3
import test_fused_second_order as TF
import test_horizontal_viscosity as TH
import test_momentum_advection as TM
import test_pressure_gradient as TP
import test_vertical_diffusion as TD
import test_vertical_momentum_advection as TJ
import test_vertical_velocity as TV
from test_richardson_number import FILLS as RI_FILLS
from test_richardson_number import _aligned, _same_bits

BCS = ["periodic", "extend", "fill"]
NAN = float("nan")
FILL = {"X": 1.75, "Y": -0.625, "Z": 0.375}
NEG0 = {"X": -0.0, "Y": -0.0, "Z": -0.0}
FILLS = list(RI_FILLS) + [NEG0]          # finite, -0.0 / NaN mixed, NaN / -0.0 mixed, -0.0 on every axis
assert RI_FILLS[0] == FILL and len(FILLS) == 4
DTYPES = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
# the chain's device functions: barred while a table runs
CHAIN = ("stencil1d", "stencil2d", "stencil1d_halo", "binary", "cumsum1d", "reduce1d", "vorticity", "divergence", "gradient",
         "flux", "pad_nd")


@pytest.fixture(params=["host_abi", pytest.param("hip", marks=pytest.mark.gpu)])
def leg(request):
    """the library under test behind `xgcm_amd.device._MEM`: the host build (CPU) or the HIP build (GPU)"""
    if request.param == "host_abi":
        request.getfixturevalue("host_abi")
    return request.param


# ---- one case -------------------------------------------------------------------------------------------------------------
class Spec:
    """what a builder turns into one call: the shape, the dtype, the operator's boundary tuple, the fill set, the variant
    number `k` (metric form, weighted or not, Coriolis / coefficient form: each builder takes it apart its own way) and an
    `edit` applied to the list of field arrays before the call (zeros, planted NaNs)"""

    def __init__(self, lead, nz, ny, nx, dtype, pads, fill=FILL, k=0, edit=None, note=""):
        self.lead, self.nz, self.ny, self.nx, self.dtype = tuple(lead), nz, ny, nx, dtype
        self.pads, self.fill, self.k, self.edit, self.note = tuple(pads), fill, k, edit, note

    def __repr__(self):
        return (f"lead {self.lead} nz {self.nz} ny {self.ny} nx {self.nx} {np.dtype(self.dtype)} {self.pads} fill {self.fill} "
                f"k {self.k} {self.note}")


def _edited(s, fields):
    """the labelled fields with `s.edit` applied to private copies of their values"""
    vals = [np.array(f.values) for f in fields]
    if s.edit is not None:
        s.edit(vals)
    return [f._replace(data=a) for f, a in zip(fields, vals)], vals


def _xy(s):
    return {"X": s.pads[0], "Y": s.pads[1]}, {"X": s.fill["X"], "Y": s.fill["Y"]}


def _xyz(s):
    return dict(zip("XYZ", s.pads[:3])), dict(s.fill)


def _run(entry, grid, direct, want, dims):
    return types.SimpleNamespace(entry=entry, grid=grid, direct=direct, want=want, dims=tuple(dims))


# ---- the ten builders: Spec -> (entry, Grid call, direct call, numpy statement, dims) -------------------------------------
def b_fdiv(s):
    px, py = s.pads
    weighted, met_lead = s.k % 4 != 1, TF.LEAD_NAMES[:len(s.lead)] if s.k % 4 == 2 else ()
    pad, fill = _xy(s)
    grid, ds, dims = TF._grid(s.lead, s.ny, s.nx, s.dtype, pad, met_lead=met_lead)
    (u, v, t), (nu, nv, nt) = _edited(s, TF._fields(s.lead, s.ny, s.nx, s.dtype, dims))
    area = TF._metric_arrays(ds, dims, met_lead)["rA"] if weighted else None
    return _run("flux_divergence", lambda: grid.flux_divergence(u, v, t, fill_value=fill, metric_weighted=weighted),
                lambda D: D.flux_divergence(nu, nv, nt, _full(area, nt.ndim), px, py, fill["X"], fill["Y"]),
                lambda: (TF._want_flux_div(nu, nv, nt, px, py, 1.0 if area is None else area, fill=fill),), [t.dims])


def b_lap(s):
    px, py = s.pads
    weighted, met_lead = s.k % 4 != 1, TF.LEAD_NAMES[:len(s.lead)] if s.k % 4 == 2 else ()
    pad, fill = _xy(s)
    grid, ds, dims = TF._grid(s.lead, s.ny, s.nx, s.dtype, pad, met_lead=met_lead)
    (t,), (nt,) = _edited(s, TF._fields(s.lead, s.ny, s.nx, s.dtype, dims)[2:])
    met = TF._metric_arrays(ds, dims, met_lead) if weighted else None
    planes = [None] * 5 if met is None else [_full(met[k], nt.ndim) for k in ("dxC", "dyC", "dyG", "dxG", "rA")]
    return _run("laplacian", lambda: grid.laplacian(t, fill_value=fill, metric_weighted=weighted),
                lambda D: D.laplacian(nt, px, py, fill["X"], fill["Y"], *planes),
                lambda: (TF._want_laplacian(nt, px, py, met, fill=fill),), [t.dims])


def b_fdiv3(s):
    px, py, pz = s.pads
    weighted, volume = s.k % 3 != 1, ("product", "registered")[(s.k // 3) % 2]
    pad, fill = _xyz(s)
    grid, ds, dims = T3._grid(s.lead, s.nz, s.ny, s.nx, s.dtype, pad, volume=volume)
    f, n = _edited(s, T3._fields(s.lead, s.nz, s.ny, s.nx, s.dtype, dims))
    vol = T3._volume(ds, volume) if weighted else None
    if not weighted:
        planes = (None, None)
    elif volume == "registered":
        planes = (_full(vol, n[0].ndim), None)
    else:
        planes = (_full(np.asarray(ds["rA"].values)[None], n[0].ndim), _full(np.asarray(ds["drF"].values)[:, None, None], n[0].ndim))
    return _run("flux_divergence_3d", lambda: grid.flux_divergence_3d(*f, fill_value=fill, metric_weighted=weighted),
                lambda D: D.flux_divergence_3d(*n, *planes, px, py, pz, fill["X"], fill["Y"], fill["Z"]),
                lambda: (T3._want(*n, px, py, pz, vol, fill=fill),), [f[3].dims])


def b_wvel(s):
    px, py, pz, rev = s.pads
    fw, mw = s.k % 3 != 1, s.k % 4 != 2
    faces, area = ("factors", "registered")[(s.k // 2) % 2], ("plane", "full")[(s.k // 3) % 2]
    pad, fill = _xyz(s)
    grid, ds, dims = TV._grid(s.lead, s.nz, s.ny, s.nx, s.dtype, pad, faces=faces, area=area)
    (u, v), (nu, nv) = _edited(s, TV._fields(s.lead, s.nz, s.ny, s.nx, s.dtype, dims))
    nd = nu.ndim
    if not fw:
        mus = (None, None, None, None)
    elif faces == "registered":
        mus = (_full(ds["yzA"].values, nd), None, _full(ds["xzA"].values, nd), None)
    else:
        drf = _full(np.asarray(ds["drF"].values)[:, None, None], nd)
        mus = (_full(np.asarray(ds["dyG"].values)[None], nd), drf, _full(np.asarray(ds["dxG"].values)[None], nd), drf)
    a = TV._area(ds, area) if mw else None
    a3 = None if a is None else (a[None] if a.ndim == 2 else a)
    return _run("vertical_velocity",
                lambda: grid.vertical_velocity(u, v, fill_value=fill, reverse=rev, face_weighted=fw, metric_weighted=mw),
                lambda D: D.vertical_velocity(nu, nv, *mus, _full(a3, nd), px, py, pz, fill["X"], fill["Y"], fill["Z"], rev),
                lambda: (TV._want(nu, nv, px, py, pz, rev, faces=TV._face_areas(ds, faces) if fw else None, area=a, fill=fill),),
                [dims + ("ZL", "YC", "XC")])


def b_ke(s):
    px, py = s.pads
    pad, fill = _xy(s)
    grid, ds, dims = TM._grid(s.lead, s.ny, s.nx, s.dtype, pad)
    (u, v), (nu, nv) = _edited(s, TM._fields(s.lead, s.ny, s.nx, s.dtype, dims))
    return _run("kinetic_energy", lambda: grid.kinetic_energy(u, v, fill_value=fill),
                lambda D: D.kinetic_energy(nu, nv, px, py, fill["X"], fill["Y"]),
                lambda: (TM._want_ke(nu, nv, px, py, fill=fill),), [dims + ("YC", "XC")])


def b_madv(s):
    from xgcm_amd import DataArray

    px, py = s.pads
    weighted, cform = (s.k // 3) % 2 == 0, s.k % 3          # Coriolis: a (YG, XG) plane, none, f(YG) alone
    pad, fill = _xy(s)
    grid, ds, dims = TM._grid(s.lead, s.ny, s.nx, s.dtype, pad)
    (u, v), (nu, nv) = _edited(s, TM._fields(s.lead, s.ny, s.nx, s.dtype, dims))
    cor = cor_np = None
    if cform == 0:
        cor, cor_np = ds["f"], np.asarray(ds["f"].values)
    elif cform == 2:
        row = (TM.R.synthetic_field((s.ny,), 66) * 2.0).astype(s.dtype)
        cor, cor_np = DataArray(row, ("YG",)), row[:, None]
    mets = [_full(ds[k].values, nu.ndim) if weighted else None for k in ("rAz", "dxC", "dyC")]
    return _run("momentum_advection", lambda: grid.momentum_advection(u, v, cor, fill_value=fill, metric_weighted=weighted),
                lambda D: D.momentum_advection(nu, nv, _full(cor_np, nu.ndim), *mets, px, py, fill["X"], fill["Y"]),
                lambda: TM._want(nu, nv, px, py, ds if weighted else None, cor_np, fill=fill),
                [dims + ("YC", "XG"), dims + ("YG", "XC")])


def b_pgrad(s):
    px, py, pz = s.pads
    weighted, weight = s.k % 3 != 1, ("drF", "full")[s.k % 2]
    planes = "lead" if s.lead and (s.k // 2) % 2 else "plane"
    pad, fill = _xyz(s)
    grid, ds, dims = TP._grid(s.lead, s.nz, s.ny, s.nx, s.dtype, pad, weight=weight, planes=planes)
    (b,), (nb,) = _edited(s, [TP._field(s.lead, s.nz, s.ny, s.nx, s.dtype, dims)])
    w = _aligned(ds["drF"], b.dims)
    mx = _aligned(ds["dxC"], dims + ("ZC", "YC", "XG")) if weighted else None
    my = _aligned(ds["dyC"], dims + ("ZC", "YG", "XC")) if weighted else None
    return _run("hydrostatic_pressure_gradient",
                lambda: grid.hydrostatic_pressure_gradient(b, fill_value=fill, metric_weighted=weighted),
                lambda D: D.hydrostatic_pressure_gradient(nb, _full(w), _full(mx), _full(my), px, py, pz, fill["X"], fill["Y"],
                                                          fill["Z"]),
                lambda: TP._want(nb, w, px, py, pz, fill=fill, mx=mx, my=my),
                [dims + ("ZC", "YC", "XG"), dims + ("ZC", "YG", "XC")])


def b_vmadv(s):
    px, py, pz = s.pads
    metric = ("drF", "full", "lead" if s.lead else "full", None)[s.k % 4]
    weighted = metric is not None and (s.k // 4) % 3 != 1
    pad, fill = _xyz(s)
    grid, ds, dims = TJ._grid(s.lead, s.nz, s.ny, s.nx, s.dtype, pad, metric=metric)
    f, n = _edited(s, TJ._fields(s.lead, s.nz, s.ny, s.nx, s.dtype, dims))
    mu, mv = TJ._metrics_of(ds, metric, s.lead) if weighted else (None, None)
    return _run("vertical_momentum_advection",
                lambda: grid.vertical_momentum_advection(*f, fill_value=fill, metric_weighted=weighted),
                lambda D: D.vertical_momentum_advection(*n, _full(mu, n[0].ndim), _full(mv, n[0].ndim), px, py, pz, fill["X"],
                                                        fill["Y"], fill["Z"]),
                lambda: TJ._want(*n, px, py, pz, fill=fill, mu=mu, mv=mv),
                [dims + ("ZC", "YC", "XG"), dims + ("ZC", "YG", "XC")])


def b_hvisc(s):
    px, py = s.pads
    form, weighted = ("none", "planes", "rows", "full")[s.k % 4], (s.k // 4) % 2 == 0
    pad, fill = _xy(s)
    grid, ds, dims = TH._grid(s.lead, s.ny, s.nx, s.dtype, pad)
    (u, v), (nu, nv) = _edited(s, TH._fields(s.lead, s.ny, s.nx, s.dtype, dims))
    coef, coef_np = TH._coefficients(form, s.lead, s.ny, s.nx, s.dtype, dims, ds)
    planes = [_full(ds[k].values, nu.ndim) if weighted else None for k in ("rA", "rAz", "dxC", "dyC", "dyG", "dxG")]
    planes += [_full(c, nu.ndim) for c in coef_np]
    return _run("horizontal_viscosity", lambda: grid.horizontal_viscosity(u, v, *coef, fill_value=fill, metric_weighted=weighted),
                lambda D: D.horizontal_viscosity(nu, nv, *planes, px, py, fill["X"], fill["Y"]),
                lambda: TH._want(nu, nv, px, py, ds if weighted else None, coef_np, fill=fill),
                [dims + ("YC", "XG"), dims + ("YG", "XC")])


def b_vdiff(s):
    pz, to = s.pads
    metric = ("1d", "full", "lead" if s.lead else "full", None)[s.k % 4]
    kform = ("3d", "1d", None, "lead")[(s.k // 2) % 4]
    hpos = "cuv"[s.k % 3]
    weighted = metric is not None and (s.k // 4) % 3 != 1
    fz = s.fill["Z"]
    grid, ds, dims = TD._grid(s.lead, s.nz, s.ny, s.nx, s.dtype, pz, metric=metric, hpos=hpos)
    (a,), (na,) = _edited(s, [TD._field(s.lead, s.nz, s.ny, s.nx, s.dtype, dims, hpos)])
    kappa = TD._kappa(kform, s.lead, s.nz, s.ny, s.nx, s.dtype, dims, to, hpos)
    f_dims = a.dims[:-3] + (TD.ZDIM[to],) + a.dims[-2:]
    mf = _aligned(ds[{"left": "drCl", "outer": "drCo"}[to]], f_dims) if weighted else None
    mc = _aligned(ds["drF"], a.dims) if weighted else None
    kap = None if kappa is None else _aligned(kappa, f_dims)
    return _run("vertical_diffusion", lambda: grid.vertical_diffusion(a, kappa, to=to, fill_value=fz, metric_weighted=weighted),
                lambda D: D.vertical_diffusion(na, _full(kap), _full(mf), _full(mc), to == "outer", pz, fz),
                lambda: (TD._want_of(grid, ds, a, kappa, to, pz, fz, weighted),), [a.dims])


def _full(m, ndim=None):
    """a plane of the numpy statement as `xgcm_amd.device` takes it: contiguous, the field's number of dims, extent 1 where
    it is broadcast"""
    if m is None:
        return None
    m = np.asarray(m)
    return np.ascontiguousarray(m.reshape((1,) * ((ndim or m.ndim) - m.ndim) + m.shape))


PADS2 = list(itertools.product(BCS, BCS))
PADS3 = list(itertools.product(BCS, BCS, BCS))
# K7f: upward from a Z pad (`fill`, `extend`) or downward (`reverse`, under any Z boundary)
PADS_W = [p + z for p in PADS2 for z in (("fill", False), ("extend", False), ("fill", True), ("extend", True), ("periodic", True))]
PADS_I = list(itertools.product(BCS, BCS, ["fill", "extend"]))          # K7i refuses a periodic Z
PADS_L = list(itertools.product(BCS, ["left", "outer"]))                # K7l: the Z boundary and where the flux sits


class Op:
    def __init__(self, build, nfields, pads, zdims=False, lead2=True, banded=False, column=True):
        self.build, self.nfields, self.pads, self.zdims, self.banded = build, nfields, pads, zdims, banded
        self.lead2 = lead2      # do the CPU suite's grids take two leading dims?
        self.column = column    # does the one-pass entry serve a single column (ny * nx == 1)?

    def legal(self, s):
        if not self.column and s.ny * s.nx == 1:
            return False
        if self.build is b_wvel and s.pads[2] == "extend" and s.nz == 1 and not s.pads[3]:
            return False
        return True


OPS = {"fdiv": Op(b_fdiv, 3, PADS2, banded=True), "lap": Op(b_lap, 1, PADS2, banded=True),
       "fdiv3": Op(b_fdiv3, 4, PADS3, zdims=True, lead2=False), "wvel": Op(b_wvel, 2, PADS_W, zdims=True, lead2=False, column=False),
       "ke": Op(b_ke, 2, PADS2, lead2=False), "madv": Op(b_madv, 2, PADS2, lead2=False, banded=True),
       "pgrad": Op(b_pgrad, 1, PADS_I, zdims=True, column=False), "vmadv": Op(b_vmadv, 3, PADS3, zdims=True),
       "hvisc": Op(b_hvisc, 2, PADS2, lead2=False, banded=True), "vdiff": Op(b_vdiff, 1, PADS_L, zdims=True)}
OPNAMES = pytest.mark.parametrize("opname", list(OPS))
# operators whose running sum along Z counts a NaN as zero: planted NaNs need not reach the result
SKIPNA = ("wvel", "pgrad")


# ---- running a table ------------------------------------------------------------------------------------------------------
def _guard(monkeypatch, entry):
    """count the calls of the one-pass `entry` and bar the chain's device functions"""
    import xgcm_amd.device as D

    n = [0]
    real = getattr(D, entry)

    def counted(*a, **k):
        n[0] += 1
        return real(*a, **k)

    def refuse(*a, **k):
        raise AssertionError("a device function of the chain ran")

    monkeypatch.setattr(D, entry, counted)
    for name in CHAIN:
        monkeypatch.setattr(D, name, refuse)
    return n


def compare(run):
    """both call paths of one case against the numpy statement; returns the statement's results"""
    import xgcm_amd.device as D

    with np.errstate(all="ignore"):
        want = run.want()
    got = run.grid()
    got = got if isinstance(got, tuple) else (got,)
    assert len(got) == len(want) == len(run.dims)
    for g, w, d in zip(got, want, run.dims):
        assert tuple(g.dims) == tuple(d), ("Grid", g.dims, d)
        try:
            _same_bits(np.asarray(g.values), w)
        except AssertionError as err:
            raise AssertionError("through Grid") from err
    got = run.direct(D)
    got = got if isinstance(got, tuple) else (got,)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        try:
            _same_bits(D.tohost(g), w)
        except AssertionError as err:
            raise AssertionError("through xgcm_amd.device directly") from err
    return want


def solid(want, nan_planted=False, zeros=False):
    """does the numpy result prove anything?  A finite non-zero value (and a NaN where NaNs were planted); for all-zero
    inputs: that (a finite fill value reaches the result), or zeros of both signs"""
    flat = np.concatenate([np.asarray(w).reshape(-1) for w in want])
    ok = bool((np.isfinite(flat) & (flat != 0)).any())
    if zeros:
        z = flat[flat == 0]
        return ok or bool(np.signbit(z).any() and not np.signbit(z).all())
    return ok and (not nan_planted or bool(np.isnan(flat).any()))


def run_table(monkeypatch, opname, specs, judge=solid):
    """every spec of the table on both call paths, counted; returns (cases, solid cases)"""
    op = OPS[opname]
    specs = [s for s in specs if op.legal(s)]
    runs = [op.build(s) for s in specs]
    n = _guard(monkeypatch, runs[0].entry)
    good = 0
    for s, run in zip(specs, runs):
        try:
            want = compare(run)
        except AssertionError as err:
            raise AssertionError(f"{opname}: {s}") from err
        good += bool(judge(want, **getattr(s, "judge", {})))
    assert n[0] == 2 * len(specs)   # the Grid call and the direct call of every case, none through the chain
    return len(specs), good


# ---- 1. the smallest shapes at which it can go wrong ----------------------------------------------------------------------
# ny: one row (the row above is the pad), one full 2-row segment, a partial one; nz: fewer levels than the 3-level window of
# K7f / K7i, exactly it, one more, two windows and one; nx: the X pad beside every column (1, 2, 3), one lane vector (8), the
# narrow form with lane 63's neighbour in the next tile (129, 257), the vector form with a partial last tile (130 / 260 in
# float64, 260 / 516 in float32)
NYS, NZS, NXS = [1, 2, 3, 9], [1, 2, 3, 4, 7], [1, 2, 3, 8, 129, 130, 257, 260, 516]


def nan_every(period, field):
    def edit(vals):
        vals[field % len(vals)].reshape(-1)[1::period] = np.nan
    return edit


def shape_specs(opname, nx, dtype):
    """every ny (and nz) with this nx; the boundary tuple, the fills, the variant and the NaNs rotate"""
    op = OPS[opname]
    out = []
    for n, (nz, ny) in enumerate(itertools.product(NZS if op.zdims else [3], NYS)):
        k = n + 5 * NXS.index(nx) + 3 * (dtype is np.float32)
        nan = (nz + ny + k) % 4 == 0
        s = Spec((), nz, ny, nx, dtype, op.pads[(7 * k) % len(op.pads)], FILLS[(k // 2) % 4 if k % 3 == 0 else 0], k=k,
                 edit=nan_every(7, k) if nan else None, note="nan" if nan else "")
        s.judge = dict(nan_planted=nan and opname not in SKIPNA)
        out.append(s)
    return out


# solid cases per (operator, dtype), summed over NXS; computed from the numpy statements alone (tools in the docstring of
# `test_the_tables_are_mostly_solid`)
SOLID_SHAPES = {   # (operator, dtype) -> (cases, solid cases) per nx of NXS
    ('fdiv', 'float64'): [(4, 2), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4)],
    ('fdiv', 'float32'): [(4, 3), (4, 3), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4)],
    ('lap', 'float64'): [(4, 2), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4)],
    ('lap', 'float32'): [(4, 3), (4, 3), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4)],
    ('fdiv3', 'float64'): [(20, 18), (20, 20), (20, 20), (20, 20), (20, 20), (20, 19), (20, 19), (20, 19), (20, 20)],
    ('fdiv3', 'float32'): [(20, 20), (20, 20), (20, 20), (20, 20), (20, 20), (20, 20), (20, 19), (20, 18), (20, 19)],
    ('wvel', 'float64'): [(14, 13), (19, 19), (19, 19), (19, 18), (19, 19), (19, 19), (19, 18), (19, 18), (19, 19)],
    ('wvel', 'float32'): [(15, 14), (19, 19), (19, 18), (19, 19), (19, 19), (19, 18), (19, 19), (19, 19), (19, 17)],
    ('ke', 'float64'): [(4, 3), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4)],
    ('ke', 'float32'): [(4, 4), (4, 3), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4)],
    ('madv', 'float64'): [(4, 3), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4)],
    ('madv', 'float32'): [(4, 4), (4, 3), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4)],
    ('pgrad', 'float64'): [(15, 15), (20, 20), (20, 19), (20, 20), (20, 20), (20, 20), (20, 20), (20, 19), (20, 20)],
    ('pgrad', 'float32'): [(15, 15), (20, 20), (20, 20), (20, 20), (20, 20), (20, 20), (20, 19), (20, 20), (20, 20)],
    ('vmadv', 'float64'): [(20, 17), (20, 18), (20, 17), (20, 17), (20, 18), (20, 17), (20, 17), (20, 18), (20, 17)],
    ('vmadv', 'float32'): [(20, 17), (20, 18), (20, 17), (20, 17), (20, 18), (20, 17), (20, 17), (20, 18), (20, 17)],
    ('hvisc', 'float64'): [(4, 3), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4)],
    ('hvisc', 'float32'): [(4, 3), (4, 3), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4), (4, 4)],
    ('vdiff', 'float64'): [(20, 15), (20, 17), (20, 18), (20, 18), (20, 18), (20, 17), (20, 16), (20, 17), (20, 18)],
    ('vdiff', 'float32'): [(20, 18), (20, 18), (20, 17), (20, 16), (20, 17), (20, 18), (20, 18), (20, 18), (20, 17)],
}
SOLID_SHAPES = {k + (nx,): v for k, row in SOLID_SHAPES.items() for nx, v in zip(NXS, row)}


@OPNAMES
@DTYPES
@pytest.mark.parametrize("nx", NXS)
def test_small_shapes(leg, monkeypatch, opname, dtype, nx):
    n, good = run_table(monkeypatch, opname, shape_specs(opname, nx, dtype))
    assert (n, good) == SOLID_SHAPES[opname, np.dtype(dtype).name, nx]


# ---- 2. every boundary combination ----------------------------------------------------------------------------------------
# (lead, nz, ny, nx): no leading dim, one, two (where the CPU suite's grid takes two); the variant number walks through the
# metric forms -- absent, (Y, X) planes, with a leading dim, a profile along Z -- of each builder
LEADS = [((), 4, 5, 8), ((2,), 3, 5, 6), ((2, 2), 3, 4, 5), ((3,), 5, 3, 12)]


def matrix_specs(opname, dtype):
    op = OPS[opname]
    out = []
    for n, (pads, (lead, nz, ny, nx)) in enumerate(itertools.product(op.pads, LEADS)):
        if len(lead) == 2 and not op.lead2:
            lead = lead[:1]
        nan = n % 5 == 4
        s = Spec(lead, nz, ny, nx, dtype, pads, FILLS[n % 4 if n % 3 == 0 else 0], k=n, edit=nan_every(7, n) if nan else None,
                 note="nan" if nan else "")
        s.judge = dict(nan_planted=nan and opname not in SKIPNA)
        out.append(s)
    return out


SOLID_MATRIX = {   # (operator, dtype) -> (cases, solid cases)
    ('fdiv', 'float64'): (36, 36), ('fdiv', 'float32'): (36, 36), ('lap', 'float64'): (36, 36), ('lap', 'float32'): (36, 36),
    ('fdiv3', 'float64'): (108, 108), ('fdiv3', 'float32'): (108, 108), ('wvel', 'float64'): (180, 180),
    ('wvel', 'float32'): (180, 180), ('ke', 'float64'): (36, 36), ('ke', 'float32'): (36, 36), ('madv', 'float64'): (36, 36),
    ('madv', 'float32'): (36, 36), ('pgrad', 'float64'): (72, 72), ('pgrad', 'float32'): (72, 72),
    ('vmadv', 'float64'): (108, 108), ('vmadv', 'float32'): (108, 108), ('hvisc', 'float64'): (36, 36),
    ('hvisc', 'float32'): (36, 36), ('vdiff', 'float64'): (24, 24), ('vdiff', 'float32'): (24, 24),
}


@OPNAMES
@DTYPES
def test_every_boundary_combination(leg, monkeypatch, opname, dtype):
    specs = matrix_specs(opname, dtype)
    assert {s.pads for s in specs} == set(OPS[opname].pads)
    n, good = run_table(monkeypatch, opname, specs)
    assert (n, good) == SOLID_MATRIX[opname, np.dtype(dtype).name]


# ---- 3. band-major order --------------------------------------------------------------------------------------------------
BAND_NX = {np.float64: 260, np.float32: 516}
BANDED = [k for k, op in OPS.items() if op.banded]
# variants that weight the operator with (Y, X) planes (K7h: Coriolis as a plane, as f(Y), absent; K7k: the coefficient forms)
BAND_K = {"fdiv": (0, 3, 0, 3), "lap": (0, 3, 0, 3), "madv": (0, 8, 7, 1), "hvisc": (1, 8, 2, 9)}


@pytest.mark.parametrize("opname", BANDED)
@DTYPES
def test_band_major_order(leg, monkeypatch, opname, dtype):
    """planes shared by all outer indices under three levels, ny = 33 (two 16-row bands and a ragged row), several wave tiles
    with a partial last one: the launcher's band-major order.  Then the same values with one plane per level -- the plain
    order -- through `xgcm_amd.device` directly: the same numpy result."""
    import xgcm_amd.device as D

    ks = BAND_K[opname]
    specs = [Spec((3,), 1, 33, BAND_NX[dtype], dtype, pads, FILLS[n % 4], k=ks[n], edit=nan_every(31, n) if n == 1 else None)
             for n, pads in enumerate([("periodic", "extend"), ("fill", "periodic"), ("extend", "fill"), ("fill", "fill")])]
    n, good = run_table(monkeypatch, opname, specs)
    assert (n, good) == (4, 4)
    runs = [OPS[opname].build(s) for s in specs]
    count = _guard(monkeypatch, runs[0].entry)
    counted, spread_planes = getattr(D, runs[0].entry), [0]

    def spread(x):   # a plane with a leading extent of 1 under the (3, Y, X) fields: one copy per level
        if isinstance(x, np.ndarray) and x.shape == (1, 33, BAND_NX[dtype]):
            spread_planes[0] += 1
            return np.ascontiguousarray(np.broadcast_to(x, (3,) + x.shape[1:]))
        return x

    monkeypatch.setattr(D, runs[0].entry, lambda *a: counted(*[spread(x) for x in a]))
    for s, run in zip(specs, runs):
        before = spread_planes[0]
        with np.errstate(all="ignore"):
            want = run.want()
        got = run.direct(D)
        got = got if isinstance(got, tuple) else (got,)
        assert spread_planes[0] > before, f"{opname}: {s}: no shared plane in the call"
        for g, w in zip(got, want):
            _same_bits(D.tohost(g), w)
    assert count[0] == len(specs)


# ---- 4. fills and zeros ---------------------------------------------------------------------------------------------------
def zero_fields(vals):
    """all-zero fields whose signs alternate with period 3, each field from its own phase"""
    for k, a in enumerate(vals):
        a[...] = 0.0
        a.reshape(-1)[k % 3::3] = -0.0


def two_of_three_negative(vals):
    zero_fields(vals)
    for a in vals:
        np.negative(a, out=a)


def fill_specs(opname, dtype, zeros):
    """every fill set over the boundary tuples that hold a `fill`, three variants each, at two shapes (nx no multiple of the
    zeros' period of 3: the signs then differ from row to row)"""
    op = OPS[opname]
    with_fill = [p for p in op.pads if "fill" in p]
    out = []
    for n, (fill, (lead, nz, ny, nx)) in enumerate(itertools.product(FILLS, [((2,), 3, 5, 7), ((), 4, 3, 8)])):
        for j in range(3):
            pads = with_fill[(7 * (3 * n + j) + n // 2) % len(with_fill)]
            edit = None if not zeros else (zero_fields, two_of_three_negative)[j % 2]
            s = Spec(lead, nz, ny, nx, dtype, pads, fill, k=n + j, edit=edit, note="zeros" if zeros else "")
            s.judge = dict(zeros=zeros)
            out.append(s)
    return out


SOLID_FILLS = {   # (operator, dtype, all-zero fields?) -> (cases, solid cases)
    ('fdiv', 'float64', False): (24, 24), ('fdiv', 'float64', True): (24, 18), ('fdiv', 'float32', False): (24, 24),
    ('fdiv', 'float32', True): (24, 18), ('lap', 'float64', False): (24, 24), ('lap', 'float64', True): (24, 22),
    ('lap', 'float32', False): (24, 24), ('lap', 'float32', True): (24, 22), ('fdiv3', 'float64', False): (24, 24),
    ('fdiv3', 'float64', True): (24, 7), ('fdiv3', 'float32', False): (24, 24), ('fdiv3', 'float32', True): (24, 7),
    ('wvel', 'float64', False): (24, 24), ('wvel', 'float64', True): (24, 18), ('wvel', 'float32', False): (24, 24),
    ('wvel', 'float32', True): (24, 18), ('ke', 'float64', False): (24, 24), ('ke', 'float64', True): (24, 6),
    ('ke', 'float32', False): (24, 24), ('ke', 'float32', True): (24, 6), ('madv', 'float64', False): (24, 24),
    ('madv', 'float64', True): (24, 24), ('madv', 'float32', False): (24, 24), ('madv', 'float32', True): (24, 24),
    ('pgrad', 'float64', False): (24, 24), ('pgrad', 'float64', True): (24, 20), ('pgrad', 'float32', False): (24, 24),
    ('pgrad', 'float32', True): (24, 20), ('vmadv', 'float64', False): (24, 24), ('vmadv', 'float64', True): (24, 21),
    ('vmadv', 'float32', False): (24, 24), ('vmadv', 'float32', True): (24, 21), ('hvisc', 'float64', False): (24, 24),
    ('hvisc', 'float64', True): (24, 17), ('hvisc', 'float32', False): (24, 24), ('hvisc', 'float32', True): (24, 17),
    ('vdiff', 'float64', False): (24, 24), ('vdiff', 'float64', True): (24, 23), ('vdiff', 'float32', False): (24, 24),
    ('vdiff', 'float32', True): (24, 23),
}


@OPNAMES
@DTYPES
@pytest.mark.parametrize("zeros", [False, True], ids=["values", "zeros"])
def test_fills_and_zeros(leg, monkeypatch, opname, dtype, zeros):
    n, good = run_table(monkeypatch, opname, fill_specs(opname, dtype, zeros))
    assert (n, good) == SOLID_FILLS[opname, np.dtype(dtype).name, zeros]


# ---- 5. NaN inputs --------------------------------------------------------------------------------------------------------
def nan_specs(opname, dtype):
    """one NaN every 3, 7 and 31 elements in each field in turn"""
    op = OPS[opname]
    out = []
    for n, (period, field) in enumerate(itertools.product((3, 7, 31), range(op.nfields))):
        s = Spec((2,), 4, 7, 10, dtype, op.pads[(7 * n + 2) % len(op.pads)], FILL, k=n, edit=nan_every(period, field),
                 note=f"a NaN every {period} in field {field}")
        s.judge = dict(nan_planted=True)
        s.period = period
        out.append(s)
    return out


SOLID_NANS = {   # (operator, dtype) -> (cases, cases whose NaN mask is neither empty nor full)
    ('fdiv', 'float64'): (9, 9), ('fdiv', 'float32'): (9, 9), ('lap', 'float64'): (3, 3), ('lap', 'float32'): (3, 3),
    ('fdiv3', 'float64'): (12, 12), ('fdiv3', 'float32'): (12, 12), ('wvel', 'float64'): (6, 0), ('wvel', 'float32'): (6, 0),
    ('ke', 'float64'): (6, 6), ('ke', 'float32'): (6, 6), ('madv', 'float64'): (6, 6), ('madv', 'float32'): (6, 6),
    ('pgrad', 'float64'): (3, 0), ('pgrad', 'float32'): (3, 0), ('vmadv', 'float64'): (9, 9), ('vmadv', 'float32'): (9, 9),
    ('hvisc', 'float64'): (6, 6), ('hvisc', 'float32'): (6, 6), ('vdiff', 'float64'): (3, 3), ('vdiff', 'float32'): (3, 3),
}


def partial_nan(want, nan_planted=True):
    """the statement's NaN mask is neither empty nor full"""
    flat = np.concatenate([np.isnan(np.asarray(w)).reshape(-1) for w in want])
    return bool(flat.any() and not flat.all()) and solid(want, nan_planted=True)


@OPNAMES
@DTYPES
def test_nan_inputs(leg, monkeypatch, opname, dtype):
    """`_same_bits` compares the NaN masks; the count is of the cases whose mask is neither empty nor full"""
    n, good = run_table(monkeypatch, opname, nan_specs(opname, dtype), judge=partial_nan)
    assert (n, good) == SOLID_NANS[opname, np.dtype(dtype).name]


# ---- 6. the tables themselves ---------------------------------------------------------------------------------------------
# all-zero inputs cannot be solid in three quarters of their cases for these two: a kinetic energy is a sum of squares, +0.0 under
# every fill but a finite one, and the 3-D divergence adds three differences, -0.0 only where all three are
FEW_SIGNED_ZEROS = ("ke", "fdiv3")


def test_the_tables_are_mostly_solid():
    """at least three quarters of every table are solid cases, by the constants above (`python tests/test_one_pass_numpy.py`
    prints them from the numpy statements alone); the shape tables meet every boundary tuple, every fill set and both dtypes.
    The NaN table counts masks that are neither empty nor full: K7f and K7i count a NaN as zero in their running sums, so
    with finite fills their masks are empty and their count is 0."""
    for name, table in (("shapes", SOLID_SHAPES), ("matrix", SOLID_MATRIX), ("fills", SOLID_FILLS)):
        per_op = {}
        for key, (n, good) in table.items():
            a, b = per_op.get(key[:2], (0, 0))
            per_op[key[:2]] = (a + n, b + good)
        for key, (n, good) in per_op.items():
            assert 4 * good >= 3 * n or (name == "fills" and key[0] in FEW_SIGNED_ZEROS), (name, key, n, good)
    for key, (n, good) in SOLID_FILLS.items():
        assert good == n or key[2], key   # ordinary fields: every case is solid
    for key, (n, good) in SOLID_NANS.items():
        assert (n, good) == (3 * OPS[key[0]].nfields, 0 if key[0] in SKIPNA else 3 * OPS[key[0]].nfields), key
    for opname, op in OPS.items():
        specs = [s for dtype in (np.float64, np.float32) for nx in NXS for s in shape_specs(opname, nx, dtype) if op.legal(s)]
        assert {s.pads for s in specs} == set(op.pads), opname
        assert {repr(sorted(s.fill.items())) for s in specs} == {repr(sorted(f.items())) for f in FILLS}, opname
        assert {bool(s.edit) for s in specs} == {True, False}


# ---- 7. the comparison is live --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plant", ["a zero's sign flipped", "one cell off by one ulp", "X and Y boundary modes swapped"])
def test_the_comparison_is_live(leg, monkeypatch, plant):
    """value plants on `device.flux_divergence`: each makes the comparison fail, on both call paths (nothing here touches
    memory outside an array)"""
    import torch

    import xgcm_amd.device as D

    zeros = plant.startswith("a zero")
    s = Spec((2,), 1, 5, 7, np.float64, ("fill", "periodic"), NEG0 if zeros else FILL, k=0, edit=zero_fields if zeros else None)
    run = b_fdiv(s)
    compare(run)   # the control: as it is, the case passes
    real = D.flux_divergence

    def planted(u, v, t, area, bc_x, bc_y, *fills):
        if plant.startswith("X and Y"):
            return real(u, v, t, area, bc_y, bc_x, *fills)
        out = real(u, v, t, area, bc_x, bc_y, *fills)
        flat = (out if isinstance(out, torch.Tensor) else torch.from_numpy(out)).reshape(-1)
        if zeros:
            i = int((flat == 0).nonzero()[0])
            flat[i] = -flat[i]
        else:
            i = int((torch.isfinite(flat) & (flat != 0)).nonzero()[0])
            flat[i] = torch.nextafter(flat[i], torch.full_like(flat[i], float("inf")))
        return out

    monkeypatch.setattr(D, "flux_divergence", planted)
    with pytest.raises(AssertionError, match="through Grid"):
        compare(run)
    grid_call, run.grid = run.grid, lambda: (monkeypatch.setattr(D, "flux_divergence", real), grid_call(),
                                             monkeypatch.setattr(D, "flux_divergence", planted))[1]
    with pytest.raises(AssertionError, match="directly"):
        compare(run)
    print(f"liveness [{leg}] {plant}: the comparison failed through Grid and through xgcm_amd.device, as it must")


def _statement_counts():
    """the constants, from the numpy statements alone"""
    def count(opname, specs, judge=solid):
        op = OPS[opname]
        specs = [s for s in specs if op.legal(s)]
        good = 0
        for s in specs:
            with np.errstate(all="ignore"):
                good += bool(judge(op.build(s).want(), **getattr(s, "judge", {})))
        return len(specs), good

    out = {"SOLID_SHAPES": {}, "SOLID_MATRIX": {}, "SOLID_FILLS": {}, "SOLID_NANS": {}}
    for opname, dtype in itertools.product(OPS, (np.float64, np.float32)):
        d = np.dtype(dtype).name
        for nx in NXS:
            out["SOLID_SHAPES"][opname, d, nx] = count(opname, shape_specs(opname, nx, dtype))
        out["SOLID_MATRIX"][opname, d] = count(opname, matrix_specs(opname, dtype))
        for zeros in (False, True):
            out["SOLID_FILLS"][opname, d, zeros] = count(opname, fill_specs(opname, dtype, zeros))
        out["SOLID_NANS"][opname, d] = count(opname, nan_specs(opname, dtype), judge=partial_nan)
    return out


if __name__ == "__main__":
    for name, table in _statement_counts().items():
        print(f"{name} = {table!r}")
