"""Every `Grid` operator held to its CONTINUOUS meaning on a smoothly stretched grid (`tests/analytic_grid.py`).

The rest of the suite proves that each kernel reproduces a chain of one-axis operators bit for bit, over random positive
metrics.  It cannot see a chain that divides by the metric of the wrong position, averages to the wrong point, has a sign
wrong or is fed a velocity where a circulation belongs: kernel, host twin, chain and numpy statement then agree on the same
wrong bits.  Here every metric is geometry, every input is an analytic field sampled at its C-grid points, and every result is
compared with the analytic value of the term the docstring names, at the result's own points.

Each case is evaluated at n = 16, 32, 64 in float64 through the public `Grid` method with `metric_weighted=True` (unless
the case says otherwise), numpy in and numpy out.  E(n) is the max-norm error of one result and the assertion is on the
observed order p = log2(E(32) / E(64)).

THE BAR is derived, not measured: every operator here is centred differences and two-point means on a smooth map, so the
asymptotic order is 2.  p >= 1.75 passes; a first-order defect (a metric half a cell off) measures about 1, a zeroth-order one
(a sign, a point, a missing factor) about 0 or below.  `MEASURED` holds the three errors of every result as the host build
gave them; E(64) must stay within a factor 2 of its entry, and on the GPU every E(n) must equal its entry to 1e-12 relative
(the two builds are bit-identical by other tests: this ties the analytic check to the kernel that ran).  The one exception is
stated where it is made (`reassociated`): a sum along the contiguous axis is added up in another order by contract.

Z is a closed column.  Each case passes the Z padding its operator's docstring prescribes for that, and may leave out the
outermost face or level at each end where the operator's own pad makes that value a boundary condition and not an
approximation; each such omission is named where it is made (`omit=`), and nothing else is left out.  X and Y are periodic:
no horizontal point is left out.

Where a one-pass kernel is documented to serve the call, the case names its device entry and the number of calls; both
backends assert that count, so no case silently measures the fallback chain.

float32 runs n = 32 only: `F32_RATIO` holds E32(32) / E64(32) as measured on the host build, asserted at 1.5 times that.

`SWAPPED` shows that the test can fail: for each metric an operator reads, the same case on the variant grid that registers
a metric of another position in its place must measure p < 1.5 (CPU only).

`momentum_advection` and `horizontal_viscosity` with `metric_weighted=True` compute zeta and D in index space over the area
(they difference the raw velocities), so they are right only on a grid of unit spacing: the true statement is a strict
expected failure (to be flipped by the change that gives the kernels circulations and transports), and the uniform-grid cases
hold what they do compute.  The measured figures are in each reason and in profiles/EXPERIMENTS.md, "Convergence".
`integrate` over (X, Z) at the cell centre in one call is first order with this metric set by the reference's own rule for
a metric it has to interpolate: behaviour kept on purpose, pinned by a passing test of its own."""

import types
import warnings

import numpy as np
import pytest

import analytic_grid as AG
from analytic_grid import ONE, AnalyticGrid, Cos, Field, Poly, Sin

BAR = 1.75
LIVE_BAR = 1.5
PI = np.pi

C3, U3, V3 = ("ZC", "YC", "XC"), ("ZC", "YC", "XG"), ("ZC", "YG", "XC")
L3, O3 = ("ZL", "YC", "XC"), ("ZO", "YC", "XC")
C2, U2, V2, Q2 = ("YC", "XC"), ("YC", "XG"), ("YG", "XC"), ("YG", "XG")
ZFACE = {"left": "ZL", "outer": "ZO"}
DX, DY, DZ = (0, 0, 1), (0, 1, 0), (1, 0, 0)

# ---- the fields --------------------------------------------------------------------------------------------------------
# a tracer with no flux through z = 0 and z = 1 (cos m pi z), wavenumbers 1-2 in x and y
A = Field((Cos(PI), Cos(2), Sin(1)), (Cos(2 * PI, 0.4), Sin(1), Cos(1)), (Poly(0.7), Cos(1), Sin(2)))
# a tracer whose first three Z derivatives vanish at both ends: cos(3 pi z) / 9 - cos(pi z) in z, a_z = (4 pi / 3) sin^3(pi z)
# (see `vertical_diffusion` below)
AFLAT = Field((Cos(PI, -1.0), Cos(2), Sin(1)), (Cos(3 * PI, 1.0 / 9.0), Cos(2), Sin(1)), (Poly(0.7), Cos(1), Sin(2)))
# a tracer with a gradient through the ends (the one-axis operators, the advected tracer)
T = Field((Poly(1.0, 0.5, -0.8), Cos(1), Sin(2)), (Sin(2.0, 0.6), Sin(2), Cos(1)), (Poly(0.3, 1.0), ONE, ONE))
# a smoother tracer (wavenumber 1) for the advection and Redi cases, whose own truncation error would otherwise hide a metric
TL = Field((Poly(1.0, 0.5, -0.8), Cos(1), Sin(1)), (Sin(1.0, 0.6), Sin(1), Cos(1)), (Poly(0.3, 1.0), ONE, ONE))
# the field of the sums over whole periods: T with terms that are odd in one coordinate and constant in the other -- the
# whole-period sums of T's own waves vanish by symmetry whatever the weights, these feel a horizontal metric of the wrong position
TM = T + Field((Poly(0.2, 0.5), ONE, Sin(1)), (Poly(0.4, -0.3), Sin(1), ONE))
# buoyancy: a background stratification b_z >= 5 - 0.3 pi under a wave
B = Field((Poly(0.0, 5.0), ONE, ONE), (Cos(PI, 0.3), Cos(2), Sin(1)))
# a solenoidal velocity with w = 0 at z = 0 and z = 1: u = P_x G', v = Q_y G', w = -(P_xx + Q_yy) G with G = sin(pi z)
U = Field((Cos(PI, PI), Cos(1), Cos(1)))
V = Field((Cos(PI, PI), Cos(1), Sin(1)))
W = Field((Sin(PI), Cos(1), Sin(1)), (Sin(PI), Sin(1), Sin(1)))
# a sheared velocity with u_z^2 + v_z^2 >= 1 (the Richardson number's denominator)
UR = Field((Poly(0.0, 2.0), ONE, ONE), (Cos(PI, 0.3), Cos(2), Sin(1)))
VR = Field((Poly(0.0, -1.0), ONE, ONE), (Cos(PI, 0.2), Sin(1), Cos(2)))
# the horizontal velocity of the 2-D operators (not solenoidal: D and zeta both matter)
UH = Field((ONE, Cos(2), Sin(1)), (ONE, Sin(1), Cos(1, 0.3)))
VH = Field((ONE, Sin(1), Cos(2)), (ONE, Cos(2), Sin(1, 0.4)))
FCOR = Field((ONE, ONE, ONE), (ONE, Sin(1, 0.5), Cos(1)))                 # f at the vorticity point
NUD = Field((ONE, Poly(1.0), ONE), (ONE, Cos(1, 0.3), Sin(2)))           # viscosities, positive
NUZ = Field((ONE, Poly(1.2), ONE), (ONE, Sin(2, 0.4), Cos(1)))
# diffusivities at the faces of Z, positive
KZ = Field((Poly(0.05, 0.04, -0.03), ONE, ONE))
K3 = Field((Poly(0.05, 0.04, -0.03), ONE, ONE), (Cos(PI, 0.015), Cos(1), Sin(2)))
# the off-diagonal Redi components: zero at z = 0 and z = 1, as a tensor of a closed column is
KWX = Field((Sin(PI, 0.05), Cos(1), Sin(2)), (Sin(2 * PI, 0.02), ONE, ONE))
KWY = Field((Sin(PI, 0.04), Sin(2), Cos(1)), (Sin(PI, 0.03), ONE, ONE))
ALL_FIELDS = dict(A=A, AFLAT=AFLAT, T=T, TL=TL, TM=TM, B=B, U=U, V=V, W=W, UR=UR, VR=VR, UH=UH, VH=VH, FCOR=FCOR, NUD=NUD,
                  NUZ=NUZ, KZ=KZ, K3=K3, KWX=KWX, KWY=KWY)
DT = 2.0                     # the implicit solves' time step: dt kappa / drF^2 is about 25 at n = 16 and 400 at n = 64
PP = dict(nu0=5e-3, alpha=5.0, nu_b=1e-4, kappa_b=1e-5)


@pytest.fixture(params=["host-abi", pytest.param("hip", marks=pytest.mark.gpu)])
def cbackend(request, monkeypatch):
    if request.param == "host-abi":
        import host_abi_device

        host_abi_device.install(monkeypatch)
    return request.param


# ---- the cases ---------------------------------------------------------------------------------------------------------
CASES = {}


def case(name, entry=None, calls=1, ns=(16, 32, 64), reads=(), f32_n=32, xfail=None, interpolated=False, cpu_double=(),
         reassociated=False):
    """registers `fn(ag) -> [(label, result, analytic value, omit)]`.  `entry`: the one-pass device entry documented to serve
    the call, `calls` of it per evaluation; `reads` {metric: the metric of another position that SWAPPED registers in its
    place}; `omit`: None, or (index, words) -- the index that keeps everything but the named outermost faces / levels.
    `interpolated`: MITgcm's set has no metric at the result's points (no dxF, dxV, dyF, dyU), so `get_metric` warns and
    interpolates the last one registered for the axis (dxG, dyG) with `extend`: to the centre along the OTHER axis, which
    is exact on a separable map; to the corner (YG, XG) along the axis itself, a two-point mean that is second order inside
    (at the wrap `extend` repeats the first cell where a periodic axis has the last one: first order in general, hidden
    here because this map has x'' = 0 at xi = 0).  Every other case must find its metric without that warning.  `cpu_double`: device entries the host build of the ABI does not have
    (it returns "not part of the host build"): on the CPU they are the oracle double's numpy statements of the same entry.
    `reassociated`: the result is a sum along the contiguous axis, which the two builds add up in different orders by contract
    (results within 1e-12 of their value, `Grid._weight_factors`), so one ulp of a total of 30 moves an E of 1e-3 by 3e-12 of
    itself: on the GPU these E(n) are held to the recorded ones within 1e-12 of the RESULT's max-norm, not of E"""
    def deco(fn):
        CASES[name] = types.SimpleNamespace(name=name, fn=fn, entry=entry, calls=calls, ns=ns, reads=dict(reads), f32_n=f32_n,
                                            xfail=xfail, interpolated=interpolated, cpu_double=tuple(cpu_double),
                                            reassociated=reassociated)
        return fn
    return deco


INNER_FACES = (np.s_[1:-1], "faces 0 and nz: the operator's pad of the level beyond the end")
NOT_FACE_0 = (np.s_[1:], "face 0: the operator's pad of the level above level 0")
NOT_LAST_LEVEL = (np.s_[:-1], "level nz-1: the operator's pad of the flux beyond it")
NOT_LAST_LEVEL_PAD = (np.s_[:-1], "level nz-1: the operator's pad of the face beyond it (ZL has no face nz)")
NOT_LAST_LEVEL_W = (np.s_[:-1], "level nz-1: the flux beyond it is the operator's pad, exactly 0 = w(1), where the w diagnosed "
                    "from sampled analytic transports would continue with the column's discrete divergence, O(h^2) and not 0: "
                    "over drF that difference is O(h), in this one level")
ZFILL0 = dict(padding={"Z": "fill"}, fill_value={"Z": 0.0})
ZEXTEND = dict(padding={"Z": "extend"})


def evaluate(c, n, dtype=np.float64, swap=None, counter=None, scales=None, **grid_kw):
    """{label: E(n)} of one case; asserts that the analytic values kept are finite and not trivial, that at most two of the
    positions along Z are left out, and (with `counter`) the number of calls of the one-pass entry"""
    ag = AnalyticGrid(n, dtype=dtype, swap=swap, **{**getattr(c, "grid_kw", {}), **grid_kw})
    before = len(counter) if counter is not None else 0
    out = {}
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        results = c.fn(ag)
    told = [w for w in caught if "being interpolated from metrics" in str(w.message)]
    assert bool(told) == c.interpolated and len(told) == len(caught), (c.name, [str(w.message) for w in caught])
    for label, got, want, omit in results:
        got = np.asarray(got.values if hasattr(got, "values") else got)
        want = np.asarray(want)
        assert got.shape == want.shape, (c.name, label, got.shape, want.shape)
        assert got.dtype == np.dtype(dtype), (c.name, label, got.dtype)
        if omit is not None:
            assert got.ndim == 3 and got[omit[0]].shape[0] >= got.shape[0] - 2 and omit[1], (c.name, label)
            got, want = got[omit[0]], want[omit[0]]
        assert np.isfinite(want).all() and np.abs(want).max() > 1e-3, (c.name, label)
        assert np.isfinite(got).all(), (c.name, label, "the result is not finite where the analytic value is")
        out[label] = float(np.abs(got.astype(np.float64) - want).max())
        if scales is not None:
            scales.setdefault(label, []).append(float(np.abs(want).max()))
    if counter is not None and c.entry is not None:
        assert len(counter) - before == c.calls, (c.name, "one-pass entry calls", len(counter) - before, "expected", c.calls)
    return out


def counted(monkeypatch, c, backend="host-abi"):
    """the calls of the case's one-pass device entry"""
    import xgcm_amd.device as D

    if backend == "host-abi":
        from oracle import fake_device

        for name in c.cpu_double:
            monkeypatch.setattr(D, name, getattr(fake_device, name))
    if c.entry is None:
        return None

    calls = []
    real = getattr(D, c.entry)
    monkeypatch.setattr(D, c.entry, lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def order(e_coarse, e_fine):
    return float(np.log2(e_coarse / e_fine))


# -- one-axis operators: this pins `get_metric`'s choice of position --------------------------------------------------------
def _one_axis(op, axis, src, dst, field, want_d, omit=None, to=None, kw=None, reads=(), interpolated=False, tag=""):
    k = "ZYX".index(axis)
    pos = f"{src[k]}-{dst[k]}{tag}"

    @case(f"{op}/{axis}/{pos}", reads=reads, interpolated=interpolated and op == "derivative")
    def _(ag):
        a = ag.array(field, src, name="a")
        args = dict(kw or {})
        if to is not None:
            args["to"] = to
        got = getattr(ag.grid, op)(a, axis, **args)
        assert tuple(got.dims) == tuple(dst)
        return [(op, got, ag.value(field, dst, d=want_d), omit)]


for _op, _d in (("derivative", 1), ("interp", 0)):
    _dd = lambda v: tuple(_d * x for x in v)    # noqa: E731
    _one_axis(_op, "X", C3, U3, T, _dd(DX), reads={"dxC": "dxG"} if _d else ())
    _one_axis(_op, "X", U3, C3, T, _dd(DX), reads={"dxG": "dxC"} if _d else (), interpolated=True)
    _one_axis(_op, "X", V3, ("ZC", "YG", "XG"), T, _dd(DX), reads={"dxG": "dxC"} if _d else (), interpolated=True, tag="@YG")
    _one_axis(_op, "Y", C3, V3, T, _dd(DY), reads={"dyC": "dyG"} if _d else ())
    _one_axis(_op, "Y", V3, C3, T, _dd(DY), reads={"dyG": "dyC"} if _d else (), interpolated=True)
    _one_axis(_op, "Y", U3, ("ZC", "YG", "XG"), T, _dd(DY), reads={"dyG": "dyC"} if _d else (), interpolated=True, tag="@XG")
    _one_axis(_op, "Z", C3, O3, T, _dd(DZ), omit=INNER_FACES, to="outer", kw=ZEXTEND, reads={"drCo": "drF"} if _d else ())
    _one_axis(_op, "Z", C3, L3, T, _dd(DZ), omit=NOT_FACE_0, to="left", kw=ZEXTEND, reads={"drCl": "drF"} if _d else ())
    _one_axis(_op, "Z", O3, C3, T, _dd(DZ), to="center", reads={"drF": "drCl"} if _d else ())
    _one_axis(_op, "Z", L3, C3, T, _dd(DZ), omit=NOT_LAST_LEVEL_PAD, to="center", kw=ZEXTEND, reads={"drF": "drCl"} if _d else ())


@case("cumint/X/center-left", reads={"dxG": "dxC"}, interpolated=True)
def _(ag):
    got = ag.grid.cumint(ag.array(T, C3), "X", to="left", padding={"X": "fill"}, fill_value={"X": 0.0})
    return [("cumint", got, ag.value(T, U3, d=(0, 0, -1)), None)]


@case("cumint/Y/left-center", reads={"dyC": "dyG"})
def _(ag):
    # v's points: cell j of the dual grid spans YC[j-1] .. YC[j], so the running integral to YC[j] starts at YC[-1], which is
    # YC[ny-1] - 2 pi
    got = ag.grid.cumint(ag.array(T, V3), "Y", to="center")
    y0 = ag.pts["YC"][-1] - AG.TWO_PI
    z, y, x = ag.points(C3)
    return [("cumint", got, T(z, y, x, d=(0, -1, 0)) - T(z, [y0], x, d=(0, -1, 0)), None)]


@case("cumint/Z/center-outer", reads={"drF": "drCl"})
def _(ag):
    got = ag.grid.cumint(ag.array(T, C3), "Z", to="outer", **ZFILL0)
    return [("cumint", got, ag.value(T, O3, d=(-1, 0, 0)), None)]


@case("cumsum-weighted/Z/center-left", reads={"drF": "drCl"})
def _(ag):
    """`cumsum(metric_weighted=Z)` is cumsum(a drF) / drC at the faces: times the exact drC it is the running integral"""
    got = ag.grid.cumsum(ag.array(T, C3), "Z", to="left", metric_weighted=("Z",), **ZFILL0)
    return [("cumsum", got.values * ag.exact["drCl"][:, None, None].astype(ag.dtype), ag.value(T, L3, d=(-1, 0, 0)), None)]


def _total(ag, field, dims, d):
    """the field integrated from 0 to the end of each axis with d = -1, at the points of `dims` along the others"""
    z, y, x = ag.points(dims)
    ends = [np.array([1.0]), np.array([AG.TWO_PI]), np.array([AG.TWO_PI])]
    pts = [ends[k] if d[k] == -1 else p for k, p in enumerate((z, y, x))]
    out = field(*pts, d=d)
    return out.reshape([n for k, n in enumerate(out.shape) if d[k] != -1])


@case("integrate/Z", reads={"drF": "drCl"})
def _(ag):
    return [("integrate", ag.grid.integrate(ag.array(T, C3), "Z"), _total(ag, T, C3, (-1, 0, 0)), None)]


@case("average/Z", reads={"drF": "drCl"})
def _(ag):
    return [("average", ag.grid.average(ag.array(T, C3), "Z"), _total(ag, T, C3, (-1, 0, 0)) / 1.0, None)]


@case("integrate/X-then-Z", reads={"dxG": "dxC"}, interpolated=True, reassociated=True)
def _(ag):
    """over a whole period the midpoint rule converges faster than any power, so X rides with Z: the order is Z's, and a
    metric of the wrong position along X still costs an order (SWAPPED).  One axis at a time: in one call the centre has no exact (X, Z) metric, see
    `test_integrate_over_x_and_z_at_the_centre_is_first_order_with_this_metric_set`"""
    got = ag.grid.integrate(ag.grid.integrate(ag.array(TM, C3), "X"), "Z")
    return [("integrate", got, _total(ag, TM, C3, (-1, 0, -1)), None)]


@case("integrate/YZ/u", reads={"dyG": "dyC"})
def _(ag):
    return [("integrate", ag.grid.integrate(ag.array(TM, U3), ["Y", "Z"]), _total(ag, TM, U3, (-1, -1, 0)), None)]


@case("average/XYZ", reads={"rA": "rAz"})
def _(ag):
    got = ag.grid.average(ag.array(TM, C3), ["X", "Y", "Z"])
    return [("average", np.asarray(got.values).reshape(1), _total(ag, TM, C3, (-1, -1, -1)).reshape(1) / AG.TWO_PI ** 2, None)]


@case("integrate/XYZ/no-area", reads={"dxC": "dxG"}, reassociated=True)
def _(ag):
    """no (X, Y) metric is registered: at u's points `get_metric` forms the area as dxC * dyG"""
    assert frozenset(("X", "Y")) not in ag.grid._own_metrics
    got = ag.grid.integrate(ag.array(TM, U3), ["X", "Y", "Z"])
    return [("integrate", np.asarray(got.values).reshape(1), _total(ag, TM, U3, (-1, -1, -1)).reshape(1), None)]


CASES["integrate/XYZ/no-area"].grid_kw = dict(omit=("rA", "rAz", "rAw", "rAs"))


# -- the remaining pairs of positions of the running and the whole integrals ------------------------------------------------
@case("cumint/X/left-center", reads={"dxC": "dxG"})
def _(ag):
    # u's points: cell i of the dual grid spans XC[i-1] .. XC[i]; the running integral to XC[i] starts at XC[nx-1] - 2 pi
    got = ag.grid.cumint(ag.array(T, U3), "X", to="center")
    z, y, x = ag.points(C3)
    return [("cumint", got, T(z, y, x, d=(0, 0, -1)) - T(z, y, [ag.pts["XC"][-1] - AG.TWO_PI], d=(0, 0, -1)), None)]


@case("cumint/Y/center-left", reads={"dyG": "dyC"}, interpolated=True)
def _(ag):
    got = ag.grid.cumint(ag.array(T, C3), "Y", to="left", padding={"Y": "fill"}, fill_value={"Y": 0.0})
    return [("cumint", got, ag.value(T, V3, d=(0, -1, 0)), None)]


@case("cumint/Z/center-left", reads={"drF": "drCl"})
def _(ag):
    got = ag.grid.cumint(ag.array(T, C3), "Z", to="left", **ZFILL0)
    return [("cumint", got, ag.value(T, L3, d=(-1, 0, 0)), None)]


for _src, _m in ((O3, "drCo"), (L3, "drCl")):
    @case(f"cumint/Z/{_src[0]}-ZC", reads={_m: "drF"})
    def _(ag, src=_src):
        """faces -> levels: face k carries drC[k], the half cell at face 0, so the sum through face k is the integral from 0 to
        level k"""
        got = ag.grid.cumint(ag.array(T, src), "Z", to="center")
        return [("cumint", got, ag.value(T, C3, d=(-1, 0, 0)), None)]


for _ax, _m, _dst, _d in (("X", "dxC", U3, (0, 0, -1)), ("Y", "dyC", V3, (0, -1, 0))):
    @case(f"cumsum-weighted/{_ax}/center-left", reads={_m: _m[:2] + "G"}, interpolated=True)
    def _(ag, ax=_ax, m=_m, dst=_dst, d=_d):
        """cumsum(a dxF) / dxC at the left points: times the exact dxC it is the running integral (Y likewise)"""
        got = ag.grid.cumsum(ag.array(T, C3), ax, to="left", metric_weighted=(ax,), padding={ax: "fill"}, fill_value={ax: 0.0})
        return [("cumsum", got.values * ag.exact[m][None].astype(ag.dtype), ag.value(T, dst, d=d), None)]


def _z_integral(ag, field, dims, top):
    """the field integrated from z = 0 to `top`, at the points of `dims` along Y and X"""
    _, y, x = ag.points(dims)
    return field([top], y, x, d=(-1, 0, 0))[0]


@case("integrate/Z/outer", reads={"drCo": "drF"})
def _(ag):
    """faces with drC, the half cells at both ends: the whole column"""
    return [("integrate", ag.grid.integrate(ag.array(T, O3), "Z"), _z_integral(ag, T, O3, 1.0), None)]


@case("average/Z/outer", reads={"drCo": "drF"})
def _(ag):
    return [("average", ag.grid.average(ag.array(T, O3), "Z"), _z_integral(ag, T, O3, 1.0) / 1.0, None)]


@case("integrate/Z/left", reads={"drCl": "drF"})
def _(ag):
    """ZL has no face nz: its drC cover z = 0 .. ZC[nz-1]"""
    return [("integrate", ag.grid.integrate(ag.array(T, L3), "Z"), _z_integral(ag, T, L3, ag.pts["ZC"][-1]), None)]


@case("integrate/XZ/u", reads={"dxC": "dxG"}, reassociated=True)
def _(ag):
    """at u's points the (X, Z) metric is the product dxC * drF of registered metrics; X rides with Z as in integrate/X-then-Z,
    and the sum along X of the same field is re-associated as there"""
    return [("integrate", ag.grid.integrate(ag.array(TM, U3), ["X", "Z"]), _total(ag, TM, U3, (-1, 0, -1)), None)]


@case("integrate/YZ/v", reads={"dyC": "dyG"})
def _(ag):
    return [("integrate", ag.grid.integrate(ag.array(TM, V3), ["Y", "Z"]), _total(ag, TM, V3, (-1, -1, 0)), None)]


@case("average/YZ/v", reads={"dyC": "dyG"})
def _(ag):
    got = ag.grid.average(ag.array(TM, V3), ["Y", "Z"])
    return [("average", got, _total(ag, TM, V3, (-1, -1, 0)) / AG.TWO_PI, None)]


# -- the horizontal operators ---------------------------------------------------------------------------------------------
def _uv2(ag, u=UH, v=VH, mu=None, mv=None):
    """(u, v) at their points, times the exact metrics named"""
    return (ag.array(u, U2, "u", times=None if mu is None else ag.exact[mu]),
            ag.array(v, V2, "v", times=None if mv is None else ag.exact[mv]))


def _zeta(ag, dims):
    return ag.value(VH, dims, DX) - ag.value(UH, dims, DY)


def _div(ag, dims):
    return ag.value(UH, dims, DX) + ag.value(VH, dims, DY)


@case("vorticity", entry="vorticity", reads={"rAz": "rA"})
def _(ag):
    """the documented convention: circulations u dxC, v dyC in"""
    return [("zeta", ag.grid.vorticity(*_uv2(ag, mu="dxC", mv="dyC")), _zeta(ag, Q2), None)]


@case("divergence", entry="divergence", reads={"rA": "rAz"})
def _(ag):
    """the documented convention: transports u dyG, v dxG in"""
    return [("div", ag.grid.divergence(*_uv2(ag, mu="dyG", mv="dxG")), _div(ag, C2), None)]


@case("gradient", entry="gradient", cpu_double=("gradient",), reads={"dxC": "dxG", "dyC": "dyG"})
def _(ag):
    gx, gy = ag.grid.gradient(ag.array(A, C2), metric_weighted=True)
    return [("gx", gx, ag.value(A, U2, DX), None), ("gy", gy, ag.value(A, V2, DY), None)]


@case("laplacian", entry="laplacian", reads={"dxC": "dxG", "dyC": "dyG", "dyG": "dyC", "dxG": "dxC", "rA": "rAz"})
def _(ag):
    return [("lap", ag.grid.laplacian(ag.array(A, C2)), ag.value(A, C2, (0, 0, 2)) + ag.value(A, C2, (0, 2, 0)), None)]


@case("flux", entry="flux", cpu_double=("flux",))
def _(ag):
    fx, fy = ag.grid.flux(*_uv2(ag), ag.array(T, C2))
    return [("fx", fx, ag.value(UH, U2) * ag.value(T, U2), None), ("fy", fy, ag.value(VH, V2) * ag.value(T, V2), None)]


@case("flux_divergence", entry="flux_divergence", reads={"rA": "rAz"})
def _(ag):
    got = ag.grid.flux_divergence(*_uv2(ag, mu="dyG", mv="dxG"), ag.array(T, C2))
    want = _div(ag, C2) * ag.value(T, C2) + ag.value(UH, C2) * ag.value(T, C2, DX) + ag.value(VH, C2) * ag.value(T, C2, DY)
    return [("div_uT", got, want, None)]


@case("kinetic_energy", entry="kinetic_energy")
def _(ag):
    return [("ke", ag.grid.kinetic_energy(*_uv2(ag)), 0.5 * (ag.value(UH, C2) ** 2 + ag.value(VH, C2) ** 2), None)]


def _momadv_true(ag, cor):
    f_u, f_v = (ag.value(FCOR, U2), ag.value(FCOR, V2)) if cor else (0.0, 0.0)
    kex = lambda d: ag.value(UH, d) * ag.value(UH, d, DX) + ag.value(VH, d) * ag.value(VH, d, DX)     # noqa: E731
    key = lambda d: ag.value(UH, d) * ag.value(UH, d, DY) + ag.value(VH, d) * ag.value(VH, d, DY)     # noqa: E731
    return ((_zeta(ag, U2) + f_u) * ag.value(VH, U2) - kex(U2), -(_zeta(ag, V2) + f_v) * ag.value(UH, V2) - key(V2))


def _hvisc_true(ag, nu):
    """d/dx(nu_d D) - d/dy(nu_z zeta) at u's points, d/dy(nu_d D) + d/dx(nu_z zeta) at v's"""
    def parts(dims):
        v = lambda f, d=(0, 0, 0): ag.value(f, dims, d)       # noqa: E731
        D, Dx, Dy = v(UH, DX) + v(VH, DY), v(UH, (0, 0, 2)) + v(VH, (0, 1, 1)), v(UH, (0, 1, 1)) + v(VH, (0, 2, 0))
        Z, Zx, Zy = v(VH, DX) - v(UH, DY), v(VH, (0, 0, 2)) - v(UH, (0, 1, 1)), v(VH, (0, 1, 1)) - v(UH, (0, 2, 0))
        if not nu:
            return Dx, Dy, Zx, Zy
        return (v(NUD, DX) * D + v(NUD) * Dx, v(NUD, DY) * D + v(NUD) * Dy, v(NUZ, DX) * Z + v(NUZ) * Zx,
                v(NUZ, DY) * Z + v(NUZ) * Zy)
    dx_u, _, _, zy_u = parts(U2)
    _, dy_v, zx_v, _ = parts(V2)
    return dx_u - zy_u, dy_v + zx_v


KNOWN = ("computes zeta and D in index space over the area (raw velocities differenced, not circulations / transports): "
         "on the stretched grid E(16, 32, 64) = {}")


@case("momentum_advection/true", entry="momentum_advection",
      xfail=KNOWN.format("gu 2.7, 9.1, 22.0; gv 2.6, 9.0, 21.9 (p = -1.28)"))
def _(ag):
    gu, gv = ag.grid.momentum_advection(*_uv2(ag))
    wu, wv = _momadv_true(ag, False)
    return [("gu", gu, wu, None), ("gv", gv, wv, None)]


@case("momentum_advection/true/coriolis", entry="momentum_advection",
      xfail=KNOWN.format("gu 2.6, 9.1, 22.0; gv 2.6, 9.0, 21.9 (p = -1.28)"))
def _(ag):
    gu, gv = ag.grid.momentum_advection(*_uv2(ag), coriolis=ag.array(FCOR, Q2, "f"))
    wu, wv = _momadv_true(ag, True)
    return [("gu", gu, wu, None), ("gv", gv, wv, None)]


@case("horizontal_viscosity/true", entry="horizontal_viscosity",
      xfail=KNOWN.format("gu 7.4, 20.3, 45.8; gv 8.6, 25.5, 58.9 (p = -1.2)"))
def _(ag):
    gu, gv = ag.grid.horizontal_viscosity(*_uv2(ag))
    wu, wv = _hvisc_true(ag, False)
    return [("gu", gu, wu, None), ("gv", gv, wv, None)]


@case("horizontal_viscosity/true/nu", entry="horizontal_viscosity",
      xfail=KNOWN.format("gu 9.9, 27.0, 60.9; gv 12.6, 34.0, 76.0 (p = -1.2)"))
def _(ag):
    gu, gv = ag.grid.horizontal_viscosity(*_uv2(ag), viscosity_d=ag.array(NUD, C2, "nud"), viscosity_z=ag.array(NUZ, Q2, "nuz"))
    wu, wv = _hvisc_true(ag, True)
    return [("gu", gu, wu, None), ("gv", gv, wv, None)]


# what the two compute today, on a uniform square grid dx = dy = h
UNIFORM = dict(ex=0.0, ey=0.0)


def _uniform(name, entry, weighted, power, fn, want):
    @case(name, entry=entry)
    def _(ag):
        h = ag.h[0]
        assert ag.h[0] == ag.h[1] and np.allclose(ag.exact["dxC"], h, rtol=1e-12, atol=0) and np.allclose(ag.exact["rAz"], h * h)
        gu, gv = fn(ag, weighted)
        wu, wv = want(ag, h)
        s = ag.dtype.type(h ** power)
        return [("gu", gu.values * s, wu, None), ("gv", gv.values * s, wv, None)]
    CASES[name].grid_kw = UNIFORM


def _momadv_weighted_today(ag, h):
    """weighted, zeta is the true one over h but the gradient of KE is the true one: (zeta / h) v - KE_x.  The two terms
    scale differently, so no power of h turns the result into the statement; times h it is zeta v - h KE_x, and that is
    what the case holds it to"""
    wu, wv = _momadv_true(ag, False)
    kex = ag.value(UH, U2) * ag.value(UH, U2, DX) + ag.value(VH, U2) * ag.value(VH, U2, DX)
    key = ag.value(UH, V2) * ag.value(UH, V2, DY) + ag.value(VH, V2) * ag.value(VH, V2, DY)
    return wu + (1.0 - h) * kex, wv + (1.0 - h) * key


# momentum advection, unweighted: every difference is h times a derivative, so zeta is h times the true one and the result
# h (zeta v - KE_x): / h
_uniform("momentum_advection/uniform/unweighted-over-h", "momentum_advection", False, -1,
         lambda ag, w: ag.grid.momentum_advection(*_uv2(ag), metric_weighted=w), lambda ag, h: _momadv_true(ag, False))
_uniform("momentum_advection/uniform/weighted-times-h", "momentum_advection", True, 1,
         lambda ag, w: ag.grid.momentum_advection(*_uv2(ag), metric_weighted=w), _momadv_weighted_today)
# horizontal viscosity, unweighted: D and zeta are h times the true ones and their differences h times a derivative: h^2
# times the statement, so / h^2.  weighted: D and zeta are the true ones over h (differences h times a derivative, over the
# area h^2) and the derivatives after them true: times h
_uniform("horizontal_viscosity/uniform/unweighted-over-h2", "horizontal_viscosity", False, -2,
         lambda ag, w: ag.grid.horizontal_viscosity(*_uv2(ag), metric_weighted=w), lambda ag, h: _hvisc_true(ag, False))
_uniform("horizontal_viscosity/uniform/weighted-times-h", "horizontal_viscosity", True, 1,
         lambda ag, w: ag.grid.horizontal_viscosity(*_uv2(ag), metric_weighted=w), lambda ag, h: _hvisc_true(ag, False))


# -- the three-dimensional operators --------------------------------------------------------------------------------------
def _transports(ag):
    """(u dyG drF, v dxG drF, w rA) of the solenoidal velocity"""
    drf = ag.exact["drF"][:, None, None]
    return (ag.array(U, U3, "u", times=ag.exact["dyG"][None] * drf), ag.array(V, V3, "v", times=ag.exact["dxG"][None] * drf),
            ag.array(W, L3, "w", times=ag.exact["rA"][None]))


def _velocities(ag):
    return ag.array(U, U3, "u"), ag.array(V, V3, "v"), ag.array(W, L3, "w")


for _rev in (False, True):
    for _fw in (False, True):
        @case(f"vertical_velocity/{'reverse' if _rev else 'forward'}/{'face_weighted' if _fw else 'transports'}",
              entry="vertical_velocity", reads=dict({"rA": "rAz"}, **({"dyG": "dyC", "dxG": "dxC", "drF": "drCl"} if _fw else {})))
        def _(ag, rev=_rev, fw=_fw):
            """forward: w[k] = -(d[0] + .. + d[k-1]) with w[0] the Z pad, 0: the analytic w, which is 0 at z = 0.  reverse:
            w[k] = -(d[nz-1] + .. + d[k]) = -w, the docstring's 'pass -w' convention, from w = 0 at z = 1"""
            u, v = (_velocities(ag) if fw else _transports(ag))[:2]
            got = ag.grid.vertical_velocity(u, v, reverse=rev, face_weighted=fw, **ZFILL0)
            return [("w", got, (-1.0 if rev else 1.0) * ag.value(W, L3), NOT_FACE_0 if not rev else None)]



def _udotgrad(ag, f, dims):
    return (ag.value(U, dims) * ag.value(f, dims, DX) + ag.value(V, dims) * ag.value(f, dims, DY)
            + ag.value(W, dims) * ag.value(f, dims, DZ))


@case("flux_divergence_3d", entry="flux_divergence_3d", reads={"rA": "rAz", "drF": "drCl"})
def _(ag):
    """div(uT) = u . grad T for the solenoidal velocity, transports in (analytic w: its own error is not in this case).  Z
    `fill` with 0: the flux through z = 0 is w[0] * pad = 0 * 0 and the flux beyond the last level the fill itself, 0 = w(1)"""
    got = ag.grid.flux_divergence_3d(*_transports(ag), ag.array(TL, C3), **ZFILL0)
    return [("div_uT", got, _udotgrad(ag, TL, C3), None)]


@case("flux_divergence_3d/w-from-continuity", entry="flux_divergence_3d", reads={"rA": "rAz", "drF": "drCl"})
def _(ag):
    """the same with w diagnosed by `vertical_velocity` (transport form: metric_weighted=False), as a model would"""
    u, v, _ = _transports(ag)
    w = ag.grid.vertical_velocity(u, v, metric_weighted=False, **ZFILL0)
    got = ag.grid.flux_divergence_3d(u, v, w, ag.array(TL, C3), **ZFILL0)
    return [("div_uT", got, _udotgrad(ag, TL, C3), NOT_LAST_LEVEL_W)]


@case("hydrostatic_pressure_gradient", entry="hydrostatic_pressure_gradient", reads={"dxC": "dxG", "dyC": "dyG", "drF": "drCl"})
def _(ag):
    """Z `fill` with 0: p[0] = 0 at z = 0, where the integral starts"""
    gx, gy = ag.grid.hydrostatic_pressure_gradient(ag.array(B + T, C3), **ZFILL0)
    return [("gx", gx, ag.value(B + T, U3, (-1, 0, 1)), None), ("gy", gy, ag.value(B + T, V3, (-1, 1, 0)), None)]


@case("vertical_momentum_advection", entry="vertical_momentum_advection", reads={"drF": "drCl"})
def _(ag):
    """the docstring's form and sign: gu = -w du/dz, gv = -w dv/dz in index space; here the Z index grows with z, so w is the
    analytic w as it is.  Z `fill` with 0: the products at face 0 are w[0] * (..) = 0 and beyond level nz-1 the fill, 0 = w(1)"""
    gu, gv = ag.grid.vertical_momentum_advection(ag.array(UR, U3), ag.array(VR, V3), ag.array(W, L3), **ZFILL0)
    return [("gu", gu, -ag.value(W, U3) * ag.value(UR, U3, DZ), None), ("gv", gv, -ag.value(W, V3) * ag.value(VR, V3, DZ), None)]


def _mix(ag, kfield, kdims, dims, f):
    """d/dz(kappa df/dz) at `dims`"""
    return ag.value(kfield, dims, DZ) * ag.value(f, dims, DZ) + ag.value(kfield, dims) * ag.value(f, dims, (2, 0, 0))


for _to in ("outer", "left"):
    for _kn, _kf in (("kappa(z)", KZ), ("kappa(x,y,z)", K3)):
        @case(f"vertical_diffusion/{_to}/{_kn}", entry="vertical_diffusion",
              reads={"drF": "drCl", ("drCo" if _to == "outer" else "drCl"): "drF"})
        def _(ag, to=_to, kf=_kf):
            """`extend`: the flux at face 0 (and at face nz with "outer") is exactly 0, the no-flux condition the field
            meets.  "left" pads the flux beyond level nz-1 with the flux at nz-1, not with 0: that level is left out.

            The field is AFLAT, not A.  On a stretched column face k lies z'' ds^2 / 8 off the middle between levels k-1 and
            k, so the flux carries an error e(z) h^2 with a term in kappa a_zz z'' and one in kappa a_zzz, smooth in z.
            In the interior the difference of two such errors over drF is O(h^2); at levels 0 and nz-1 one of the two
            fluxes is the exact 0 of the wall, so the result carries e(wall) h^2 / drF = O(h) unless e vanishes there: the
            finite-volume operator is first-order CONSISTENT at the two wall levels of a stretched column (and MITgcm's
            is; the implicit solve, whose ERROR is what counts, stays second order, see its case).  That is a property of
            the scheme and not a defect of the chain: AFLAT has a_zz = a_zzz = 0 at both ends, so e(wall) = 0, and
            `test_vertical_diffusion_is_first_order_at_the_walls_of_a_stretched_column` holds the derived behaviour with A.

            SWAPPED, drCl registered as drF: that run alone takes A.  drCl[0] is the half cell, half of drF[0], and AFLAT makes
            the result at level 0 itself O(h^2), which hid the swap (p = 1.54 with kappa(x, y, z)); A does not vanish there"""
            return _vdiff(ag, to, kf, A if "drF" in ag.swap else AFLAT)


def _vdiff(ag, to, kf, field):
    fdims = (ZFACE[to], "YC", "XC")
    kappa = ag.array(kf, fdims, "kappa")
    if kf is KZ:
        kappa = ag.wrap(kappa.values[:, 0, 0], fdims[:1], "kappa")
    got = ag.grid.vertical_diffusion(ag.array(field, C3), kappa, to=to, **ZEXTEND)
    return [("da", got, _mix(ag, kf, fdims, C3, field), NOT_LAST_LEVEL if to == "left" else None)]


for _to in ("outer", "left"):
    @case(f"implicit_vertical_diffusion/{_to}", entry="implicit_vertical_diffusion",
          reads={"drF": "drCl", ("drCo" if _to == "outer" else "drCl"): "drF"})
    def _(ag, to=_to):
        """x analytic with x_z = 0 at both ends, a = x - dt d/dz(kappa dx/dz) exactly: the solve must return x"""
        fdims = (ZFACE[to], "YC", "XC")
        a = ag.wrap(ag.value(A, C3) - DT * _mix(ag, K3, fdims, C3, A), C3, "a")
        got = ag.grid.implicit_vertical_diffusion(a, ag.array(K3, fdims, "kappa"), DT, to=to)
        return [("x", got, ag.value(A, C3), None)]


@case("implicit_vertical_viscosity", entry="implicit_vertical_viscosity", reads={"drF": "drCl", "drCo": "drF"})
def _(ag):
    """nu at the centre points of the faces; u, v analytic with no shear at the ends, right-hand sides exact at their points"""
    fu = Field(*A.terms[:2])
    fv = Field(*A.terms[1:])
    u = ag.wrap(ag.value(fu, U3) - DT * _mix(ag, K3, None, U3, fu), U3, "u")
    v = ag.wrap(ag.value(fv, V3) - DT * _mix(ag, K3, None, V3, fv), V3, "v")
    xu, xv = ag.grid.implicit_vertical_viscosity(u, v, ag.array(K3, O3, "nu"), DT, to="outer")
    return [("xu", xu, ag.value(fu, U3), None), ("xv", xv, ag.value(fv, V3), None)]


def _s2(ag, dims):
    return ag.value(UR, dims, DZ) ** 2 + ag.value(VR, dims, DZ) ** 2


def _buv(ag):
    return ag.array(B, C3, "b"), ag.array(UR, U3, "u"), ag.array(VR, V3, "v")


@case("vertical_shear_squared", entry="richardson_number", reads={"drCo": "drF"})
def _(ag):
    """`extend` on Z: the differences at faces 0 and nz are the pad's, exactly 0"""
    got = ag.grid.vertical_shear_squared(*_buv(ag)[1:], to="outer", **ZEXTEND)
    return [("s2", got, _s2(ag, O3), INNER_FACES)]


@case("richardson_number", entry="richardson_number")
def _(ag):
    """Ri = b_z / S2 is a ratio of two Z derivatives: the Z metric cancels, so no swap of it can show (none is listed)"""
    got = ag.grid.richardson_number(*_buv(ag), to="outer", **ZEXTEND)
    return [("ri", got, ag.value(B, O3, DZ) / _s2(ag, O3), INNER_FACES)]


@case("richardson_number/left", entry="richardson_number")
def _(ag):
    got = ag.grid.richardson_number(*_buv(ag), to="left", **ZEXTEND)
    return [("ri", got, ag.value(B, L3, DZ) / _s2(ag, L3), NOT_FACE_0)]


@case("richardson_mixing", entry="richardson_mixing", reads={"drCo": "drF"})
def _(ag):
    """Pacanowski-Philander of the analytic Ri (> 0 everywhere here)"""
    nu, kappa = ag.grid.richardson_mixing(*_buv(ag), to="outer", **PP, **ZEXTEND)
    den = 1.0 + PP["alpha"] * (ag.value(B, O3, DZ) / _s2(ag, O3))
    wnu = PP["nu0"] / den ** 2 + PP["nu_b"]
    # (the analytic values are ~1e-4: scaled to O(1) so that `evaluate`'s triviality floor applies to them as to the rest)
    return [("nu", nu.values * ag.dtype.type(1e4), wnu * 1e4, INNER_FACES),
            ("kappa", kappa.values * ag.dtype.type(1e4), (wnu / den + PP["kappa_b"]) * 1e4, INNER_FACES)]


def _slopes(ag, dims):
    bz = ag.value(B, dims, DZ)
    return -ag.value(B, dims, DX) / bz, -ag.value(B, dims, DY) / bz


@case("isopycnal_slope", entry="isopycnal_slope", reads={"dxC": "dxG", "dyC": "dyG", "drCo": "drF"})
def _(ag):
    sx, sy = ag.grid.isopycnal_slope(ag.array(B, C3), to="outer", **ZEXTEND)
    wx, wy = _slopes(ag, O3)
    return [("sx", sx, wx, INNER_FACES), ("sy", sy, wy, INNER_FACES)]


for _name, _smax in (("below-slope_max", 0.5), ("tapered", 0.06)):
    @case(f"redi_tensor/{_name}", entry="redi_tensor", reads={"dxC": "dxG", "dyC": "dyG", "drCo": "drF"})
    def _(ag, smax=_smax):
        """kappa = 1: Kwx, Kwy = taper S, Kwz = taper |S|^2, taper = min(1, (Smax / |S|)^2); the outermost faces are NaN by the
        docstring (db/dz == 0 under `extend`).  Analytic max |S| is about 0.12: 0.5 tapers nowhere, 0.06 more than a tenth of
        the faces, the steepest ones, where the taper contracts the error"""
        kx, ky, kz = ag.grid.redi_tensor(ag.array(B, C3), kappa=1.0, slope_max=smax, to="outer", **ZEXTEND)
        wx, wy = _slopes(ag, O3)
        s2 = wx * wx + wy * wy
        taper = np.minimum(1.0, smax * smax / s2)
        tapered = float((taper[1:-1] < 1).mean())     # the share of the kept faces above the limit: none, or at least a tenth
        assert tapered == 0.0 if smax > 0.2 else tapered > 0.1, tapered
        # (Kwz ~ 1e-3: scaled to O(1) for the triviality floor)
        ten, hundred = ag.dtype.type(10), ag.dtype.type(100)
        return [("kwx", kx.values * ten, 10 * taper * wx, INNER_FACES), ("kwy", ky.values * ten, 10 * taper * wy, INNER_FACES),
                ("kwz", kz.values * hundred, 100 * taper * s2, INNER_FACES)]


for _closed in (True, False):
    @case(f"redi_vertical_flux_divergence/{'closed' if _closed else 'open'}", entry="redi_vertical_flux_divergence",
          reads={"dxC": "dxG", "dyC": "dyG", "drF": "drCl"})
    def _(ag, closed=_closed):
        """d/dz(Kwx da/dx + Kwy da/dy), Kwx and Kwy analytic and 0 at z = 0 and z = 1, so the closed and the open form
        approximate the same term"""
        got = ag.grid.redi_vertical_flux_divergence(ag.array(TL, C3), ag.array(KWX, O3, "kwx"), ag.array(KWY, O3, "kwy"),
                                                    to="outer", closed=closed, **ZEXTEND)
        v = lambda f, d=(0, 0, 0): ag.value(f, C3, d)       # noqa: E731
        want = v(KWX, DZ) * v(TL, DX) + v(KWX) * v(TL, (1, 0, 1)) + v(KWY, DZ) * v(TL, DY) + v(KWY) * v(TL, (1, 1, 0))
        return [("out", got.values * ag.dtype.type(10), want * 10, None)]    # (~0.05: scaled to O(1))


# ---- what the host build measured ------------------------------------------------------------------------------------------
# "case:label" -> (E(n0), E(n1), E(n2)) for the case's ns (16, 32, 64 unless the case says otherwise), float64, host build
MEASURED = {
    "derivative/X/XC-XG:derivative": (0.09117062389300301, 0.023256032914568348, 0.005843927872177357),   # p = 1.97, 1.99
    "derivative/X/XG-XC:derivative": (0.07702746848093689, 0.02232711388197428, 0.005785071154465804),   # p = 1.79, 1.95
    "derivative/X/XC-XG@YG:derivative": (0.08302539669326814, 0.020949673768147825, 0.005250160546304894),   # p = 1.99, 2.00
    "derivative/Y/YC-YG:derivative": (0.047018025369245375, 0.011975297796094075, 0.0030073776098165084),   # p = 1.97, 1.99
    "derivative/Y/YG-YC:derivative": (0.04098162777170322, 0.011578756519839528, 0.0029822770931342557),   # p = 1.82, 1.96
    "derivative/Y/YC-YG@XG:derivative": (0.0430473315920612, 0.01085996051521354, 0.0027208178262458915),   # p = 1.99, 2.00
    "derivative/Z/ZC-ZO:derivative": (0.0016806948598079574, 0.0004649249745372064, 0.0001216098473209859),   # p = 1.85, 1.93
    "derivative/Z/ZC-ZL:derivative": (0.0016806948598079574, 0.0004649249745372064, 0.0001216098473209859),   # p = 1.85, 1.93
    "derivative/Z/ZO-ZC:derivative": (0.0018583104988753596, 0.00048549892699134567, 0.00012423492374136202),   # p = 1.94, 1.97
    "derivative/Z/ZL-ZC:derivative": (0.0018583104988753596, 0.00048549892699134567, 0.00012423492374136202),   # p = 1.94, 1.97
    "interp/X/XC-XG:interp": (0.11620717069992414, 0.032491652819843564, 0.008158805074137243),   # p = 1.84, 1.99
    "interp/X/XG-XC:interp": (0.12759943604597734, 0.032202607734274746, 0.008194997167771279),   # p = 1.99, 1.97
    "interp/X/XC-XG@YG:interp": (0.11537344735391697, 0.032468808408592675, 0.008158156869094046),   # p = 1.83, 1.99
    "interp/Y/YC-YG:interp": (0.06988743403569875, 0.01858634006558102, 0.004687367920500618),   # p = 1.91, 1.99
    "interp/Y/YG-YC:interp": (0.07319948809001342, 0.018645016702007466, 0.004705623266497483),   # p = 1.97, 1.99
    "interp/Y/YC-YG@XG:interp": (0.07008931887906877, 0.018569333979916003, 0.004688003021991349),   # p = 1.92, 1.99
    "interp/Z/ZC-ZO:interp": (0.0026799422761951686, 0.0006838375828055465, 0.00017074616314616264),   # p = 1.97, 2.00
    "interp/Z/ZC-ZL:interp": (0.0026799422761951686, 0.0006838375828055465, 0.00017074616314616264),   # p = 1.97, 2.00
    "interp/Z/ZO-ZC:interp": (0.0026856573276081708, 0.0006836844746267445, 0.00017075021780055266),   # p = 1.97, 2.00
    "interp/Z/ZL-ZC:interp": (0.0026856573276081708, 0.0006836844746267445, 0.00017075021780055266),   # p = 1.97, 2.00
    "cumint/X/center-left:cumint": (0.041733617229027686, 0.01019990678841598, 0.002536989970514991),   # p = 2.03, 2.01
    "cumint/Y/left-center:cumint": (0.023467408570768455, 0.006480723854791037, 0.0016698197307820628),   # p = 1.86, 1.96
    "cumint/Z/center-outer:cumint": (0.0010854244173590377, 0.00027091869464945795, 6.79064401933882e-05),   # p = 2.00, 2.00
    "cumsum-weighted/Z/center-left:cumsum": (0.001081316563814383, 0.0002704574425247408, 6.785185047153419e-05),   # p = 2.00, 1.99
    "integrate/Z:integrate": (0.0010854244173590377, 0.00027091869464945795, 6.79064401933882e-05),   # p = 2.00, 2.00
    "average/Z:average": (0.0010854244173590377, 0.00027091869464945795, 6.79064401933882e-05),   # p = 2.00, 2.00
    "integrate/X-then-Z:integrate": (0.006205924110560979, 0.0015704787144668053, 0.00039148335708638626),   # p = 1.98, 2.00
    "integrate/YZ/u:integrate": (0.009055047480470257, 0.002265329504818503, 0.0005686933160093943),   # p = 2.00, 1.99
    "average/XYZ:average": (0.000488281249999889, 0.0001220703125, 3.0517578125e-05),   # p = 2.00, 2.00
    "integrate/XYZ/no-area:integrate": (0.019276571095879547, 0.004819142773971663, 0.0012047856934955803),   # p = 2.00, 2.00
    "cumint/X/left-center:cumint": (0.036826493575420116, 0.009921549613733927, 0.002521738264453788),   # p = 1.89, 1.98
    "cumint/Y/center-left:cumint": (0.027430006795822415, 0.006831175699450576, 0.001705005400407078),   # p = 2.01, 2.00
    "cumint/Z/center-left:cumint": (0.001081316563814383, 0.0002704574425247408, 6.785185047153419e-05),   # p = 2.00, 1.99
    "cumint/Z/ZO-ZC:cumint": (0.0025302886077166117, 0.0006396301107901223, 0.00016136512053097594),   # p = 1.98, 1.99
    "cumint/Z/ZL-ZC:cumint": (0.0025302886077166117, 0.0006396301107901223, 0.00016136512053097594),   # p = 1.98, 1.99
    "cumsum-weighted/X/center-left:cumsum": (0.041733617229027686, 0.01019990678841598, 0.002536989970514991),   # p = 2.03, 2.01
    "cumsum-weighted/Y/center-left:cumsum": (0.027430006795822415, 0.006831175699450132, 0.001705005400407078),   # p = 2.01, 2.00
    "integrate/Z/outer:integrate": (0.001522852425885679, 0.00038286787682695334, 9.567754304340426e-05),   # p = 1.99, 2.00
    "average/Z/outer:average": (0.001522852425885679, 0.00038286787682695334, 9.567754304340426e-05),   # p = 1.99, 2.00
    "integrate/Z/left:integrate": (0.0015162149204903663, 0.00037864392378139655, 9.472684855982294e-05),   # p = 2.00, 2.00
    "integrate/XZ/u:integrate": (0.00620592411056009, 0.0015704787144645849, 0.00039148335708683035),   # p = 1.98, 2.00
    "integrate/YZ/v:integrate": (0.00898110380469408, 0.0022743711680028866, 0.0005687512808068007),   # p = 1.98, 2.00
    "average/YZ/v:average": (0.0014293870649382256, 0.00036197741381327475, 9.051957773009711e-05),   # p = 1.98, 2.00
    "vorticity:zeta": (0.09883499444156119, 0.026723115107951667, 0.00672843848564586),   # p = 1.89, 1.99
    "divergence:div": (0.036890537004300894, 0.009907250883440355, 0.0024943110891089137),   # p = 1.90, 1.99
    "gradient:gx": (0.06184056573778984, 0.01607260013366507, 0.004057167536297923),   # p = 1.94, 1.99
    "gradient:gy": (0.028726905570208183, 0.008023679485390955, 0.0020234258606350863),   # p = 1.84, 1.99
    "laplacian:lap": (0.3210552135831346, 0.0844493239818851, 0.02197259050472944),   # p = 1.93, 1.94
    "flux:fx": (0.08756967702850726, 0.022627133652079967, 0.005942916554767974),   # p = 1.95, 1.93
    "flux:fy": (0.0324883625953567, 0.008261846962409974, 0.002138210614462399),   # p = 1.98, 1.95
    "flux_divergence:div_uT": (0.3266438239654881, 0.09710412447704408, 0.02503438764436572),   # p = 1.75, 1.96
    "kinetic_energy:ke": (0.09394951977578425, 0.02543783214452411, 0.006329086398064732),   # p = 1.88, 2.01
    "momentum_advection/true:gu": (2.6826829486468964, 9.062160937125011, 21.987656686732034),   # p = -1.76, -1.28
    "momentum_advection/true:gv": (2.6271148184650683, 9.025539432432518, 21.859965238170957),   # p = -1.78, -1.28
    "momentum_advection/true/coriolis:gu": (2.5954774284352924, 9.07867928171804, 21.982282722180344),   # p = -1.81, -1.28
    "momentum_advection/true/coriolis:gv": (2.585865753204489, 9.013622620154944, 21.85643039202626),   # p = -1.80, -1.28
    "horizontal_viscosity/true:gu": (7.400833623723813, 20.275054961993508, 45.768876257532504),   # p = -1.45, -1.17
    "horizontal_viscosity/true:gv": (8.638591541685422, 25.519283675818436, 58.930386789180325),   # p = -1.56, -1.21
    "horizontal_viscosity/true/nu:gu": (9.908377178937265, 26.95422011131257, 60.866438743691496),   # p = -1.44, -1.18
    "horizontal_viscosity/true/nu:gv": (12.56900635521782, 34.04216285052435, 75.99370097333447),   # p = -1.44, -1.16
    "momentum_advection/uniform/unweighted-over-h:gu": (0.34460939853471184, 0.0934102610472678, 0.023938033287396854),   # p = 1.88, 1.96
    "momentum_advection/uniform/unweighted-over-h:gv": (0.3481810075591165, 0.09663747923861088, 0.024727440737077),   # p = 1.85, 1.97
    "momentum_advection/uniform/weighted-times-h:gu": (0.33883062980667145, 0.10567514093931374, 0.027359050715943578),   # p = 1.68, 1.95
    "momentum_advection/uniform/weighted-times-h:gv": (0.3481810075591183, 0.09813712234928218, 0.025605706152002305),   # p = 1.83, 1.94
    "horizontal_viscosity/uniform/unweighted-over-h2:gu": (0.19791380145601867, 0.05330500608098987, 0.013571808105158567),   # p = 1.89, 1.97
    "horizontal_viscosity/uniform/unweighted-over-h2:gv": (0.28195546984500197, 0.07494004851765546, 0.01902022784251134),   # p = 1.91, 1.98
    "horizontal_viscosity/uniform/weighted-times-h:gu": (0.19791380145602133, 0.05330500608099786, 0.013571808105140803),   # p = 1.89, 1.97
    "horizontal_viscosity/uniform/weighted-times-h:gv": (0.2819554698450073, 0.07494004851765812, 0.01902022784252555),   # p = 1.91, 1.98
    "vertical_velocity/forward/transports:w": (0.013227582451604825, 0.003289730163464233, 0.000830689447619104),   # p = 2.01, 1.99
    "vertical_velocity/forward/face_weighted:w": (0.013227582451604825, 0.003289730163464233, 0.000830689447619104),   # p = 2.01, 1.99
    "vertical_velocity/reverse/transports:w": (0.011870149045219991, 0.002970336919275729, 0.0007479205691334201),   # p = 2.00, 1.99
    "vertical_velocity/reverse/face_weighted:w": (0.011870149045219991, 0.002970336919275729, 0.0007479205691334201),   # p = 2.00, 1.99
    "flux_divergence_3d:div_uT": (0.2867780944823456, 0.07920264652336828, 0.02026268658668995),   # p = 1.86, 1.97
    "flux_divergence_3d/w-from-continuity:div_uT": (0.26017029957384197, 0.07475034170341166, 0.019153941046638145),   # p = 1.80, 1.96
    "hydrostatic_pressure_gradient:gx": (0.0827759611720702, 0.02124818303132625, 0.005354787599478827),   # p = 1.96, 1.99
    "hydrostatic_pressure_gradient:gy": (0.032202865608160436, 0.008284734040251318, 0.002091280720222466),   # p = 1.96, 1.99
    "vertical_momentum_advection:gu": (0.114744124078892, 0.029833705945733868, 0.007476876294721713),   # p = 1.94, 2.00
    "vertical_momentum_advection:gv": (0.06154853449305109, 0.015783337246655815, 0.003941546076976499),   # p = 1.96, 2.00
    "vertical_diffusion/outer/kappa(z):da": (0.028832574090256635, 0.007253881199498213, 0.0018508524117568648),   # p = 1.99, 1.97
    "vertical_diffusion/outer/kappa(x,y,z):da": (0.028869646238226965, 0.0075920659028752, 0.0019566123753600724),   # p = 1.93, 1.96
    "vertical_diffusion/left/kappa(z):da": (0.028832574090256635, 0.007253881199498213, 0.0018508524117568648),   # p = 1.99, 1.97
    "vertical_diffusion/left/kappa(x,y,z):da": (0.028869646238226965, 0.0075920659028752, 0.0019566123753600724),   # p = 1.93, 1.96
    "implicit_vertical_diffusion/outer:x": (0.01078258093137685, 0.002798313873242919, 0.0007099676686570522),   # p = 1.95, 1.98
    "implicit_vertical_diffusion/left:x": (0.01078258093137685, 0.002798313873242919, 0.0007099676686570522),   # p = 1.95, 1.98
    "implicit_vertical_viscosity:xu": (0.013003304167849561, 0.0033729413231072813, 0.0008542632893219215),   # p = 1.95, 1.98
    "implicit_vertical_viscosity:xv": (0.009781249802302494, 0.0025960866249579717, 0.0006581646074833025),   # p = 1.91, 1.98
    "vertical_shear_squared:s2": (0.18421457407157504, 0.048352679430619716, 0.012159986952589463),   # p = 1.93, 1.99
    "richardson_number:ri": (0.13350860078025129, 0.03766351786094768, 0.009799294432131234),   # p = 1.83, 1.94
    "richardson_number/left:ri": (0.13350860078025129, 0.03766351786094768, 0.009799294432131234),   # p = 1.83, 1.94
    "richardson_mixing:nu": (0.08778071617585148, 0.023098598950734406, 0.0058010420443244115),   # p = 1.93, 1.99
    "richardson_mixing:kappa": (0.03784298547667242, 0.010194120058769185, 0.002582995166020119),   # p = 1.89, 1.98
    "isopycnal_slope:sx": (0.00284599019049938, 0.0007786355979708601, 0.00020099787752843323),   # p = 1.87, 1.95
    "isopycnal_slope:sy": (0.017323686134866276, 0.0046137985061346365, 0.0011953247902092567),   # p = 1.91, 1.95
    "redi_tensor/below-slope_max:kwx": (0.028459901904993812, 0.007786355979708559, 0.0020099787752843046),   # p = 1.87, 1.95
    "redi_tensor/below-slope_max:kwy": (0.17323686134866279, 0.046137985061346365, 0.011953247902092734),   # p = 1.91, 1.95
    "redi_tensor/below-slope_max:kwz": (0.3752617747008906, 0.10489486844358531, 0.02811450475326227),   # p = 1.84, 1.90
    "redi_tensor/tapered:kwx": (0.04204053770120386, 0.017099795590810374, 0.004705259142539608),   # p = 1.30, 1.86
    "redi_tensor/tapered:kwy": (0.09292765926451785, 0.025107222324835643, 0.006445892326093494),   # p = 1.89, 1.96
    "redi_tensor/tapered:kwz": (0.09723927124194695, 0.029120946528803482, 0.007483275126579536),   # p = 1.74, 1.96
    "redi_vertical_flux_divergence/closed:out": (0.10900571613368948, 0.03026230223143811, 0.007698607571179128),   # p = 1.85, 1.97
    "redi_vertical_flux_divergence/open:out": (0.10900571613368948, 0.03026230223143811, 0.007698607571179128),   # p = 1.85, 1.97
}
# "case:label" -> E32(n) / E64(n) at n = 32, host build
F32_RATIO = {
    "derivative/X/XC-XG:derivative": 1.0000,
    "derivative/X/XG-XC:derivative": 1.0000,
    "derivative/X/XC-XG@YG:derivative": 1.0000,
    "derivative/Y/YC-YG:derivative": 1.0000,
    "derivative/Y/YG-YC:derivative": 1.0000,
    "derivative/Y/YC-YG@XG:derivative": 1.0000,
    "derivative/Z/ZC-ZO:derivative": 1.0005,
    "derivative/Z/ZC-ZL:derivative": 1.0005,
    "derivative/Z/ZO-ZC:derivative": 1.0000,
    "derivative/Z/ZL-ZC:derivative": 1.0000,
    "interp/X/XC-XG:interp": 1.0000,
    "interp/X/XG-XC:interp": 1.0000,
    "interp/X/XC-XG@YG:interp": 1.0000,
    "interp/Y/YC-YG:interp": 1.0000,
    "interp/Y/YG-YC:interp": 1.0000,
    "interp/Y/YC-YG@XG:interp": 1.0000,
    "interp/Z/ZC-ZO:interp": 0.9999,
    "interp/Z/ZC-ZL:interp": 0.9999,
    "interp/Z/ZO-ZC:interp": 0.9999,
    "interp/Z/ZL-ZC:interp": 0.9999,
    "cumint/X/center-left:cumint": 1.0000,
    "cumint/Y/left-center:cumint": 0.9999,
    "cumint/Z/center-outer:cumint": 0.9999,
    "cumsum-weighted/Z/center-left:cumsum": 0.9998,
    "integrate/Z:integrate": 0.9999,
    "average/Z:average": 0.9999,
    "integrate/X-then-Z:integrate": 0.9999,
    "integrate/YZ/u:integrate": 0.9998,
    "average/XYZ:average": 0.9986,
    "integrate/XYZ/no-area:integrate": 0.9996,
    "cumint/X/left-center:cumint": 1.0000,
    "cumint/Y/center-left:cumint": 1.0000,
    "cumint/Z/center-left:cumint": 0.9998,
    "cumint/Z/ZO-ZC:cumint": 1.0000,
    "cumint/Z/ZL-ZC:cumint": 1.0000,
    "cumsum-weighted/X/center-left:cumsum": 1.0000,
    "cumsum-weighted/Y/center-left:cumsum": 1.0000,
    "integrate/Z/outer:integrate": 0.9999,
    "average/Z/outer:average": 0.9999,
    "integrate/Z/left:integrate": 0.9998,
    "integrate/XZ/u:integrate": 0.9999,
    "integrate/YZ/v:integrate": 1.0001,
    "average/YZ/v:average": 1.0007,
    "vorticity:zeta": 1.0000,
    "divergence:div": 1.0000,
    "gradient:gx": 1.0000,
    "gradient:gy": 1.0000,
    "laplacian:lap": 1.0000,
    "flux:fx": 1.0000,
    "flux:fy": 1.0000,
    "flux_divergence:div_uT": 1.0000,
    "kinetic_energy:ke": 1.0000,
    "momentum_advection/uniform/unweighted-over-h:gu": 1.0000,
    "momentum_advection/uniform/unweighted-over-h:gv": 1.0000,
    "momentum_advection/uniform/weighted-times-h:gu": 1.0000,
    "momentum_advection/uniform/weighted-times-h:gv": 1.0000,
    "horizontal_viscosity/uniform/unweighted-over-h2:gu": 1.0000,
    "horizontal_viscosity/uniform/unweighted-over-h2:gv": 1.0000,
    "horizontal_viscosity/uniform/weighted-times-h:gu": 1.0000,
    "horizontal_viscosity/uniform/weighted-times-h:gv": 1.0000,
    "vertical_velocity/forward/transports:w": 1.0000,
    "vertical_velocity/forward/face_weighted:w": 1.0001,
    "vertical_velocity/reverse/transports:w": 1.0000,
    "vertical_velocity/reverse/face_weighted:w": 1.0000,
    "flux_divergence_3d:div_uT": 1.0000,
    "flux_divergence_3d/w-from-continuity:div_uT": 1.0000,
    "hydrostatic_pressure_gradient:gx": 1.0001,
    "hydrostatic_pressure_gradient:gy": 1.0000,
    "vertical_momentum_advection:gu": 1.0000,
    "vertical_momentum_advection:gv": 1.0000,
    "vertical_diffusion/outer/kappa(z):da": 0.9997,
    "vertical_diffusion/outer/kappa(x,y,z):da": 1.0001,
    "vertical_diffusion/left/kappa(z):da": 0.9997,
    "vertical_diffusion/left/kappa(x,y,z):da": 1.0001,
    "implicit_vertical_diffusion/outer:x": 1.0000,
    "implicit_vertical_diffusion/left:x": 1.0000,
    "implicit_vertical_viscosity:xu": 0.9999,
    "implicit_vertical_viscosity:xv": 1.0001,
    "vertical_shear_squared:s2": 1.0001,
    "richardson_number:ri": 1.0002,
    "richardson_number/left:ri": 1.0002,
    "richardson_mixing:nu": 1.0001,
    "richardson_mixing:kappa": 1.0000,
    "isopycnal_slope:sx": 1.0000,
    "isopycnal_slope:sy": 1.0000,
    "redi_tensor/below-slope_max:kwx": 1.0000,
    "redi_tensor/below-slope_max:kwy": 1.0000,
    "redi_tensor/below-slope_max:kwz": 1.0000,
    "redi_tensor/tapered:kwx": 1.0000,
    "redi_tensor/tapered:kwy": 1.0000,
    "redi_tensor/tapered:kwz": 1.0000,
    "redi_vertical_flux_divergence/closed:out": 1.0000,
    "redi_vertical_flux_divergence/open:out": 1.0000,
}
# (case, metric registered wrongly, the metric whose values it gets) -> {label: p(32 -> 64)}; the label that must fall is the first
SWAPPED = {
    ("derivative/X/XC-XG", "dxC", "dxG"): {'derivative': 1.11},
    ("derivative/X/XG-XC", "dxG", "dxC"): {'derivative': 1.11},
    ("derivative/X/XC-XG@YG", "dxG", "dxC"): {'derivative': 1.1},
    ("derivative/Y/YC-YG", "dyC", "dyG"): {'derivative': 1.09},
    ("derivative/Y/YG-YC", "dyG", "dyC"): {'derivative': 1.07},
    ("derivative/Y/YC-YG@XG", "dyG", "dyC"): {'derivative': 1.08},
    ("derivative/Z/ZC-ZO", "drCo", "drF"): {'derivative': 0.95},
    ("derivative/Z/ZC-ZL", "drCl", "drF"): {'derivative': 0.95},
    ("derivative/Z/ZO-ZC", "drF", "drCl"): {'derivative': -0.02},
    ("derivative/Z/ZL-ZC", "drF", "drCl"): {'derivative': -0.02},
    ("cumint/X/center-left", "dxG", "dxC"): {'cumint': 1.0},
    ("cumint/Y/left-center", "dyC", "dyG"): {'cumint': 0.99},
    ("cumint/Z/center-outer", "drF", "drCl"): {'cumint': 1.01},
    ("cumsum-weighted/Z/center-left", "drF", "drCl"): {'cumsum': 1.01},
    ("integrate/Z", "drF", "drCl"): {'integrate': 0.98},
    ("average/Z", "drF", "drCl"): {'average': 0.98},
    ("integrate/X-then-Z", "dxG", "dxC"): {'integrate': 1.01},
    ("integrate/YZ/u", "dyG", "dyC"): {'integrate': 1.12},
    ("average/XYZ", "rA", "rAz"): {'average': 1.01},
    ("integrate/XYZ/no-area", "dxC", "dxG"): {'integrate': 0.98},
    ("cumint/X/left-center", "dxC", "dxG"): {'cumint': 0.99},
    ("cumint/Y/center-left", "dyG", "dyC"): {'cumint': 1.01},
    ("cumint/Z/center-left", "drF", "drCl"): {'cumint': 1.01},
    ("cumint/Z/ZO-ZC", "drCo", "drF"): {'cumint': 0.98},
    ("cumint/Z/ZL-ZC", "drCl", "drF"): {'cumint': 0.98},
    ("cumsum-weighted/X/center-left", "dxC", "dxG"): {'cumsum': 0.95},
    ("cumsum-weighted/Y/center-left", "dyC", "dyG"): {'cumsum': 0.95},
    ("integrate/Z/outer", "drCo", "drF"): {'integrate': 1.02},
    ("average/Z/outer", "drCo", "drF"): {'average': 0.98},
    ("integrate/Z/left", "drCl", "drF"): {'integrate': 1.0},
    ("integrate/XZ/u", "dxC", "dxG"): {'integrate': 0.99},
    ("integrate/YZ/v", "dyC", "dyG"): {'integrate': 1.09},
    ("average/YZ/v", "dyC", "dyG"): {'average': 1.09},
    ("vorticity", "rAz", "rA"): {'zeta': 1.03},
    ("divergence", "rA", "rAz"): {'div': 1.03},
    ("gradient", "dxC", "dxG"): {'gx': 1.12, 'gy': 1.99},
    ("gradient", "dyC", "dyG"): {'gy': 1.08, 'gx': 1.99},
    ("laplacian", "dxC", "dxG"): {'lap': 1.2},
    ("laplacian", "dyC", "dyG"): {'lap': 1.39},
    ("laplacian", "dyG", "dyC"): {'lap': 1.42},
    ("laplacian", "dxG", "dxC"): {'lap': 1.45},
    ("laplacian", "rA", "rAz"): {'lap': 1.11},
    ("flux_divergence", "rA", "rAz"): {'div_uT': 1.27},
    ("vertical_velocity/forward/transports", "rA", "rAz"): {'w': 1.01},
    ("vertical_velocity/forward/face_weighted", "rA", "rAz"): {'w': 1.01},
    ("vertical_velocity/forward/face_weighted", "dyG", "dyC"): {'w': 1.0},
    ("vertical_velocity/forward/face_weighted", "dxG", "dxC"): {'w': 1.03},
    ("vertical_velocity/forward/face_weighted", "drF", "drCl"): {'w': 0.99},
    ("vertical_velocity/reverse/transports", "rA", "rAz"): {'w': 1.02},
    ("vertical_velocity/reverse/face_weighted", "rA", "rAz"): {'w': 1.02},
    ("vertical_velocity/reverse/face_weighted", "dyG", "dyC"): {'w': 0.99},
    ("vertical_velocity/reverse/face_weighted", "dxG", "dxC"): {'w': 1.02},
    ("vertical_velocity/reverse/face_weighted", "drF", "drCl"): {'w': 1.0},
    ("flux_divergence_3d", "rA", "rAz"): {'div_uT': 1.2},
    ("flux_divergence_3d", "drF", "drCl"): {'div_uT': -0.02},
    ("flux_divergence_3d/w-from-continuity", "rA", "rAz"): {'div_uT': 1.1},
    ("flux_divergence_3d/w-from-continuity", "drF", "drCl"): {'div_uT': -0.02},
    ("hydrostatic_pressure_gradient", "dxC", "dxG"): {'gx': 1.1, 'gy': 1.99},
    ("hydrostatic_pressure_gradient", "dyC", "dyG"): {'gy': 1.07, 'gx': 1.99},
    ("hydrostatic_pressure_gradient", "drF", "drCl"): {'gy': 0.99, 'gx': 1.0},
    ("vertical_momentum_advection", "drF", "drCl"): {'gu': 0.96, 'gv': 1.02},
    ("vertical_diffusion/outer/kappa(z)", "drF", "drCl"): {'da': -0.02},
    ("vertical_diffusion/outer/kappa(z)", "drCo", "drF"): {'da': 0.95},
    ("vertical_diffusion/outer/kappa(x,y,z)", "drF", "drCl"): {'da': -0.01},
    ("vertical_diffusion/outer/kappa(x,y,z)", "drCo", "drF"): {'da': 0.95},
    ("vertical_diffusion/left/kappa(z)", "drF", "drCl"): {'da': -0.02},
    ("vertical_diffusion/left/kappa(z)", "drCl", "drF"): {'da': 0.95},
    ("vertical_diffusion/left/kappa(x,y,z)", "drF", "drCl"): {'da': -0.01},
    ("vertical_diffusion/left/kappa(x,y,z)", "drCl", "drF"): {'da': 0.95},
    ("implicit_vertical_diffusion/outer", "drF", "drCl"): {'x': 0.99},
    ("implicit_vertical_diffusion/outer", "drCo", "drF"): {'x': 0.96},
    ("implicit_vertical_diffusion/left", "drF", "drCl"): {'x': 0.99},
    ("implicit_vertical_diffusion/left", "drCl", "drF"): {'x': 0.96},
    ("implicit_vertical_viscosity", "drF", "drCl"): {'xv': 0.98, 'xu': 0.99},
    ("implicit_vertical_viscosity", "drCo", "drF"): {'xv': 0.93, 'xu': 0.97},
    ("vertical_shear_squared", "drCo", "drF"): {'s2': 1.0},
    ("richardson_mixing", "drCo", "drF"): {'kappa': 0.83, 'nu': 0.98},
    ("isopycnal_slope", "dxC", "dxG"): {'sx': 1.15, 'sy': 1.95},
    ("isopycnal_slope", "dyC", "dyG"): {'sy': 1.46, 'sx': 1.95},
    ("isopycnal_slope", "drCo", "drF"): {'sx': 1.15, 'sy': 1.4},
    ("redi_tensor/below-slope_max", "dxC", "dxG"): {'kwx': 1.15, 'kwy': 1.95, 'kwz': 1.9},
    ("redi_tensor/below-slope_max", "dyC", "dyG"): {'kwz': 1.45, 'kwx': 1.95, 'kwy': 1.46},
    ("redi_tensor/below-slope_max", "drCo", "drF"): {'kwx': 1.15, 'kwy': 1.4, 'kwz': 1.36},
    ("redi_tensor/tapered", "dxC", "dxG"): {'kwx': 1.47, 'kwy': 1.76, 'kwz': 1.67},
    ("redi_tensor/tapered", "dyC", "dyG"): {'kwz': 1.36, 'kwx': 1.38, 'kwy': 1.4},
    ("redi_tensor/tapered", "drCo", "drF"): {'kwx': 1.16, 'kwy': 1.4, 'kwz': 1.31},
    ("redi_vertical_flux_divergence/closed", "dxC", "dxG"): {'out': 1.18},
    ("redi_vertical_flux_divergence/closed", "dyC", "dyG"): {'out': 1.26},
    ("redi_vertical_flux_divergence/closed", "drF", "drCl"): {'out': -0.01},
    ("redi_vertical_flux_divergence/open", "dxC", "dxG"): {'out': 1.18},
    ("redi_vertical_flux_divergence/open", "dyC", "dyG"): {'out': 1.26},
    ("redi_vertical_flux_divergence/open", "drF", "drCl"): {'out': -0.01},
}

GOOD = [n for n, c in CASES.items() if c.xfail is None]
KNOWN_FAILURES = [n for n, c in CASES.items() if c.xfail is not None]


# ---- the tests -----------------------------------------------------------------------------------------------------------
def test_every_derivative_of_every_field_matches_a_fourth_order_difference():
    """a typo in a formula must not pass as a finding: about 1e-10 by the difference formula's own error"""
    for name, f in ALL_FIELDS.items():
        assert AG.check_derivatives(f) < 2e-9, name


def test_the_solenoidal_velocity_is_solenoidal_and_closed():
    ag = AnalyticGrid(8)
    div = ag.value(U, C3, DX) + ag.value(V, C3, DY) + ag.value(W, C3, DZ)
    assert np.abs(div).max() < 1e-14
    z = np.array([0.0, 1.0])
    assert np.abs(W(z, ag.pts["YC"], ag.pts["XC"])).max() < 1e-15 and np.abs(ag.value(U, C3)).max() > 1
    for f in (A, ):    # no flux through the ends
        assert np.abs(f(z, ag.pts["YC"], ag.pts["XC"], d=DZ)).max() < 1e-14
    for f in (KWX, KWY):
        assert np.abs(f(z, ag.pts["YC"], ag.pts["XC"])).max() < 1e-16


def test_the_metrics_are_the_geometry():
    """sums of lengths are the period, of thicknesses the depth; areas are products; the half cells are halves"""
    ag = AnalyticGrid((6, 7, 9))
    m = {k: np.asarray(ag.ds[k].values) for k in AG.METRIC_DIMS}
    for k in ("dxC", "dxG"):
        assert np.allclose(m[k].sum(axis=1), AG.TWO_PI, rtol=1e-14) and (m[k] > 0).all()
    for k in ("dyC", "dyG"):
        assert np.allclose(m[k].sum(axis=0), AG.TWO_PI, rtol=1e-14) and (m[k] > 0).all()
    assert np.isclose(m["drF"].sum(), 1.0) and np.isclose(m["drCo"].sum(), 1.0) and np.array_equal(m["drCl"], m["drCo"][:-1])
    assert np.isclose(m["drCo"][0], ag.pts["ZC"][0]) and np.isclose(m["drCo"][-1], 1.0 - ag.pts["ZC"][-1])
    assert np.allclose(m["rA"], m["dxG"] * m["dyG"]) and np.allclose(m["rAz"], m["dxC"] * m["dyC"])
    assert np.allclose(m["rAw"], m["dxC"] * m["dyG"]) and np.allclose(m["rAs"], m["dxG"] * m["dyC"])
    assert not np.allclose(m["dxC"], m["dxG"], rtol=1e-2) and not np.allclose(m["dyC"], m["dyG"], rtol=1e-2)
    # the variant builder changes the registered values and nothing else
    sw = AnalyticGrid((6, 7, 9), swap={"dxC": "dxG", "drCo": "drF"})
    assert np.array_equal(sw.ds["dxC"].values, m["dxG"]) and sw.ds["dxC"].dims == ("YC", "XG")
    assert np.array_equal(sw.ds["drCo"].values[:-1], m["drF"]) and sw.ds["drCo"].shape == (7,)
    assert np.array_equal(sw.ds["dxG"].values, m["dxG"]) and np.array_equal(sw.exact["dxC"], ag.exact["dxC"])


@pytest.mark.parametrize("name", GOOD)
def test_second_order(cbackend, monkeypatch, name):
    c = CASES[name]
    calls = counted(monkeypatch, c, cbackend)
    scales = {}
    errs = [evaluate(c, n, counter=calls, scales=scales) for n in c.ns]
    for label in errs[0]:
        e = [x[label] for x in errs]
        p = order(e[1], e[2])
        print(f"{name}:{label} E = {e[0]:.3e} {e[1]:.3e} {e[2]:.3e}  p = {order(e[0], e[1]):.2f} {p:.2f}")
        assert p >= BAR, (name, label, e, p)
        rec = MEASURED[f"{name}:{label}"]
        assert rec[2] / 2 <= e[2] <= rec[2] * 2, (name, label, e, rec)
        if cbackend == "hip" and c.reassociated:
            assert all(abs(a - b) <= 1e-12 * s for a, b, s in zip(e, rec, scales[label])), (name, label, e, rec, scales[label])
        elif cbackend == "hip":
            assert np.allclose(e, rec, rtol=1e-12, atol=0), (name, label, e, rec)


@pytest.mark.parametrize("name", KNOWN_FAILURES)
def test_known_failures_against_the_true_statement(cbackend, monkeypatch, request, name):
    """everything but the order is asserted as in every other case -- the entry count, the warnings, shapes, dtypes, finite
    values: a failure there is a failure.  Only the order against the true statement is expected to fail, strictly"""
    c = CASES[name]
    calls = counted(monkeypatch, c, cbackend)
    errs = [evaluate(c, n, counter=calls) for n in c.ns]
    orders = {}
    for label in errs[0]:
        e = [x[label] for x in errs]
        orders[label] = order(e[1], e[2])
        print(f"{name}:{label} E = {e[0]:.3e} {e[1]:.3e} {e[2]:.3e}  p = {order(e[0], e[1]):.2f} {orders[label]:.2f}")
    request.applymarker(pytest.mark.xfail(strict=True, raises=AssertionError, reason=c.xfail))
    assert all(p >= BAR for p in orders.values()), (name, orders)


@pytest.mark.parametrize("name", GOOD)
def test_float32_error_ratio(cbackend, monkeypatch, name):
    c = CASES[name]
    calls = counted(monkeypatch, c, cbackend)
    e32, e64 = evaluate(c, c.f32_n, np.float32, counter=calls), evaluate(c, c.f32_n, counter=calls)
    for label in e32:
        ratio = e32[label] / e64[label]
        print(f"{name}:{label} n = {c.f32_n} E32 / E64 = {ratio:.4f}")
        assert ratio <= F32_RATIO[f"{name}:{label}"] * 1.5, (name, label, ratio)


@pytest.mark.parametrize("key", sorted(SWAPPED), ids=lambda k: "-".join(k))
def test_a_metric_of_another_position_costs_an_order(host_abi, monkeypatch, key):
    name, metric, other = key
    c = CASES[name]
    counted(monkeypatch, c)   # (installs the case's CPU doubles)
    e32, e64 = (evaluate(c, n, swap={metric: other}) for n in (32, 64))
    ps = {label: order(e32[label], e64[label]) for label in e32}
    print(f"{name} with {other} registered as {metric}: p = {ps}")
    label = next(iter(SWAPPED[key]))
    assert ps[label] < LIVE_BAR, (key, ps)


def test_every_metric_an_operator_reads_has_a_swapped_case():
    want = {(n, m, o) for n, c in CASES.items() for m, o in c.reads.items()}
    assert want == set(SWAPPED) and len(want) > 40
    stages = {m for _, m, _ in want}
    assert {"dxC", "dxG", "dyC", "dyG", "rA", "rAz", "drF", "drCl", "drCo"} <= stages


def test_integrate_over_x_and_z_at_the_centre_is_first_order_with_this_metric_set(host_abi):
    """Kept on purpose, so pinned and not expected to fail: `get_metric(centre field, (X, Z))` with MITgcm's set.  No product
    of registered metrics sits at the centre (there is no dxF), and condition 4 -- the reference's rule, reproduced for parity
    and pinned by its own suite -- interpolates the LAST product of the first candidate, dxG * drC(ZO), not dxG * drF.  drC
    averaged to the levels with `extend` is (half cell + whole) / 2, three quarters of drF to O(h), at the two end levels:
    an O(1) error of the weight in 2 of n levels, so the integral is first order.  One axis at a time
    (`integrate/X-then-Z`) finds dxG and drF and is second order"""
    errs = []
    for n in (16, 32, 64):
        ag = AnalyticGrid(n)
        a = ag.array(TM, C3)
        with pytest.warns(UserWarning, match="being interpolated from metrics"):
            m = ag.grid.get_metric(a, ("X", "Z"))
            got = ag.grid.integrate(a, ["X", "Z"])
        drc = ag.exact["drCo"]
        weight = np.asarray(m.transpose("ZC", "YC", "XC").values if set(m.dims) == set(C3) else m.values)
        assert np.allclose(weight.reshape(n, -1, n)[:, 0, :], 0.5 * (drc[:-1] + drc[1:])[:, None] * ag.exact["dxG"][0][None, :], rtol=1e-13)
        assert abs(0.5 * (drc[0] + drc[1]) / ag.exact["drF"][0] - 0.75) < 1.0 / n
        errs.append(float(np.abs(got.values - _total(ag, TM, C3, (-1, 0, -1))).max()))
    p = order(errs[1], errs[2])
    print(f"integrate(centre, [X, Z]): E = {errs}, p = {p:.2f}")
    assert 0.75 < p < 1.25     # first order, derived; a second-order result here means the rule changed: update this test


def test_vertical_diffusion_is_first_order_at_the_walls_of_a_stretched_column(host_abi):
    """the derivation in the `vertical_diffusion` cases, held with A (a_zz != 0 at the walls): on the stretched column the
    interior levels are second order and the two wall levels fall below it; with cz = 0 the faces are midway between the
    levels, the flux error is kappa a_zzz h^2 / 24, which A = cos(m pi z) makes 0 at the walls, and every level is second order"""
    c = types.SimpleNamespace(name="vertical_diffusion/walls", entry=None, interpolated=False)

    def orders(cz, keep):
        c.fn = lambda ag: [(lab, got.values[keep], want[keep], None) for lab, got, want, _ in _vdiff(ag, "outer", K3, A)]
        e = [evaluate(c, n, cz=cz)["da"] for n in (16, 32, 64)]
        return order(e[0], e[1]), order(e[1], e[2])

    walls, interior, whole = orders(0.15, np.s_[[0, -1]]), orders(0.15, np.s_[1:-1]), orders(0.0, np.s_[:])
    print(f"vertical_diffusion with A: p(16->32), p(32->64) = {walls} at the walls, {interior} inside, {whole} with cz = 0")
    assert interior[1] >= BAR and whole[1] >= BAR
    # an O(h) term coming out from under an O(h^2) one: the observed order at the walls falls with n (1.81, 1.73, and 1.58 at
    # 64 -> 128, measured once), while inside it rises towards 2
    assert walls[1] < walls[0] and walls[1] < interior[1] and interior[1] > interior[0]


def test_constant_tracer_has_no_tendency(cbackend):
    """div(u c) = c div(u): exactly 0 to rounding with w from continuity, whatever the grid"""
    ag = AnalyticGrid(16)
    drf = ag.exact["drF"][:, None, None]
    u, v = (ag.array(U, U3, "u", times=ag.exact["dyG"][None] * drf), ag.array(V, V3, "v", times=ag.exact["dxG"][None] * drf))
    w = ag.grid.vertical_velocity(u, v, metric_weighted=False, **ZFILL0)
    ones = ag.wrap(np.full((16, 16, 16), 3.0), C3, "T")
    # the last level closes only as well as the column's transports sum to 0: the analytic u, v do to truncation, O(h^2),
    # so it is the levels below that must vanish to rounding (the flux beyond nz-1 is the pad, not w from continuity)
    got = ag.grid.flux_divergence_3d(u, v, w, ones, **ZFILL0).values
    scale = 3.0 * np.abs(ag.value(U, U3)).max() / ag.exact["dxC"].min()
    assert np.abs(got[:-1]).max() <= 64 * np.finfo(np.float64).eps * scale
