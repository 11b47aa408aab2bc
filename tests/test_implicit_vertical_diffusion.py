"""Implicit vertical mixing, `Grid.implicit_vertical_diffusion`: the backward-Euler solve (I - dt D) x = a per column, on CPU.

`statement` below is the specification: the Thomas recurrence over whole planes in numpy, every operation in the field's
dtype and in the order the kernel, the host build and the level loop of `xgcm_amd/grid.py` keep.  Everything is compared
with it bit for bit (NaN = NaN); `statement` itself is compared with `np.linalg.solve` on the assembled matrices.  The
one-pass path runs through the `host_abi` fixture (the product's `xgcm_amd.device` over libxgcm_host.so); a counter on
`device.implicit_vertical_diffusion` shows that every case meant for it reached it.  The tables, the statement, the NaN
cases and the direct-ABI cases are shared with the GPU suite."""

import itertools

import numpy as np
import pytest
import torch

import test_vertical_diffusion as TD
from oracle import refimpl as R
from test_fused_layouts import ALIGNED, _contig, _strided
from xgcm_amd import DataArray, Dataset, Grid, _hip
from xgcm_amd.chunked import BlockArray
from xgcm_amd.grid import _DimsOnly

TOS = ["left", "outer"]
DTYPES = [np.float64, np.float32]
KFORMS = [None, "1d", "3d", "lead"]
MFORMS = ["1d", "full", "lead", None]      # None: no metric enters (`metric_weighted=False`)
DT = 3600.0   # with kappa <= 1e4 and thicknesses of 1000 .. 2000 the coupling dt * kappa / (mf * mc) stays below 36
DT_PLAIN = DT * 1e-6   # without the metrics: dt * kappa <= 36 as well (at 3.6e7 a float32 pivot cancels to zero)
_same_bits = TD._same_bits


# ---- the definition -------------------------------------------------------------------------------------------------------
def statement(a, kappa, mf, mc, dt):
    """x of (I - dt D) x = a per column.  `a` (.., n, ny, nx); `kappa`, `mf` (indexed by face: n or n + 1 along Z, or 1:
    the same plane at every face) and `mc` (by level) broadcast against it or are None.  Faces 0 and n are never read."""
    T = a.dtype.type
    n = a.shape[-3]
    dt, one = T(dt), T(1)
    at = lambda m, k: m[..., k if m.shape[-3] > 1 else 0, :, :]  # noqa: E731
    c, d, w = np.empty_like(a), np.empty_like(a), {}
    lo = up = None
    with np.errstate(all="ignore"):
        for k in range(1, n):
            g = one if kappa is None else at(kappa, k)
            if mf is not None:
                g = g / at(mf, k)
            w[k] = dt * g
        for k in range(n):
            b = one
            if k > 0:
                lo = w[k] if mc is None else w[k] / at(mc, k)
                b = b + lo
            if k < n - 1:
                up = w[k + 1] if mc is None else w[k + 1] / at(mc, k)
                b = b + up
            m = b if k == 0 else b - lo * c[..., k - 1, :, :]
            r = one / m
            if k < n - 1:
                c[..., k, :, :] = up * r
            d[..., k, :, :] = (a[..., k, :, :] if k == 0 else a[..., k, :, :] + lo * d[..., k - 1, :, :]) * r
        x = d.copy()
        for k in range(n - 2, -1, -1):
            x[..., k, :, :] = d[..., k, :, :] + c[..., k, :, :] * x[..., k + 1, :, :]
    assert x.dtype == a.dtype
    return x


def dense_solve(a, kappa, mf, mc, dt):
    """the same system assembled as one (n, n) matrix per column from kappa, mf, mc and dt in float64, by np.linalg.solve;
    all four arrays (n, ny, nx), kappa and mf indexed by face 0 .. n-1 (face 0 unused)"""
    a, kappa, mf, mc = (np.asarray(v, np.float64) for v in (a, kappa, mf, mc))
    n, ny, nx = a.shape
    x = np.empty_like(a)
    for j, i in itertools.product(range(ny), range(nx)):
        A = np.eye(n)
        for k in range(1, n):   # the flux through face k leaves level k-1 and enters level k, or the other way round
            q = dt * kappa[k, j, i] / mf[k, j, i]
            A[k, k] += q / mc[k, j, i]
            A[k, k - 1] -= q / mc[k, j, i]
            A[k - 1, k - 1] += q / mc[k - 1, j, i]
            A[k - 1, k] -= q / mc[k - 1, j, i]
        x[:, j, i] = np.linalg.solve(A, a[:, j, i])
    return x


def _random_system(nz, dtype, seed):
    """(a, kappa, mf, mc, dt) over (nz, 3, 5): kappa >= 0 with exact zeros, coupling dt * kappa / (mf * mc) <= 320"""
    rng = np.random.default_rng(seed)
    shape = (nz, 3, 5)
    a = rng.standard_normal(shape)
    kappa = rng.uniform(0.0, 1.0, shape) * (rng.random(shape) > 0.2)
    mf, mc = rng.uniform(0.5, 2.0, shape), rng.uniform(0.5, 2.0, shape)
    return tuple(v.astype(dtype) for v in (a, kappa, mf, mc)) + (80.0,)


def _rel(got, want):
    """max-norm difference relative to the max norm of `want`"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


# measured on CPU on exactly these inputs (printed by the test): 3.044e-15 (float64), 1.602e-6 (float32); a wrong coefficient
# gives errors of order 1.  16 x the measured value: the margin is for other BLAS builds.
SOLVE_MEASURED = {np.float64: 3.044e-15, np.float32: 1.602e-6}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_the_definition_solves_the_system(dtype):
    worst = 0.0
    for n, nz in enumerate((1, 2, 3, 5, 17, 90)):
        a, kappa, mf, mc, dt = _random_system(nz, dtype, 40 + n)
        assert (kappa == 0).any() or nz == 1
        assert float((dt * kappa.astype(np.float64) / (mf * mc)).max()) <= 320.0
        worst = max(worst, _rel(statement(a, kappa, mf, mc, dt), dense_solve(a, kappa, mf, mc, dt)))
    print(f"statement against np.linalg.solve, {np.dtype(dtype)}: {worst:.3e}")
    assert worst <= 16 * SOLVE_MEASURED[dtype]


# ---- helpers over TD's grids -------------------------------------------------------------------------------------------------
def _grid(lead, nz, ny, nx, dtype, metric="1d", hpos="c", **kw):
    return TD._grid(lead, nz, ny, nx, dtype, "extend", metric=metric, hpos=hpos, **kw)


def _kappa(form, lead, nz, ny, nx, dtype, dims, to, hpos="c", seed=75):
    """TD's kappa forms with values in [0, 1e4], exact zeros among them"""
    k = TD._kappa(form, lead, nz, ny, nx, dtype, dims, to, hpos, seed)
    if k is None:
        return None
    v = np.abs(k.values.astype(np.float64)) * 2e4
    v[v < 2e3] = 0.0
    return k._replace(data=v.astype(dtype))


def _want_of(ds, a, kappa, to, weighted, dt=DT):
    """`statement` for labelled inputs: the metrics are the dataset's own arrays at the flux' and at the field's Z position"""
    f_dims = a.dims[:-3] + (TD.ZDIM[to],) + a.dims[-2:]
    mf = TD._aligned(ds[{"left": "drCl", "outer": "drCo"}[to]], f_dims) if weighted else None
    mc = TD._aligned(ds["drF"], a.dims) if weighted else None
    return statement(np.asarray(a.values), None if kappa is None else TD._aligned(kappa, f_dims), mf, mc, dt)


def _counted(monkeypatch):
    import xgcm_amd.device as D

    calls = []
    real = D.implicit_vertical_diffusion
    monkeypatch.setattr(D, "implicit_vertical_diffusion", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def _no_fused(monkeypatch):
    import xgcm_amd.device as D

    monkeypatch.setattr(D, "implicit_vertical_diffusion", lambda *a, **k: pytest.fail("one-pass entry called"))


# ---- 2. bit for bit at the smallest shapes that can go wrong --------------------------------------------------------------
NZS, NYS, NXS = [1, 2, 3, 5], [1, 2, 3, 9], [1, 2, 3, 8, 129, 130, 257]
LEADS = [(), (2,), (2, 2)]


def shape_table(nx):
    """(lead, nz, ny, nx, to, dtype, kappa form, metric form, where `a` sits): every nz and ny with this nx -- one level, one
    row, one column, nx across one x-tile, the narrow form, a ragged last segment, a second tile.  Case number k of the whole
    table picks combination (27 k + 5) mod 64 of (to, dtype, kappa form, metric form): 64 consecutive cases meet all 64, and
    no form is tied to one nz or ny.  A form with a leading dim gets one; the leading dims rotate otherwise."""
    out = []
    for n, (nz, ny) in enumerate(itertools.product(NZS, NYS)):
        k = n + len(NZS) * len(NYS) * NXS.index(nx)
        c = (27 * k + 5) % 64
        to, dtype, kform, mform = TOS[c % 2], DTYPES[(c // 2) % 2], KFORMS[(c // 4) % 4], MFORMS[c // 16]
        lead = LEADS[1 + k % 2] if "lead" in (kform, mform) else LEADS[k % 3]
        out.append((lead, nz, ny, nx, to, dtype, kform, mform, "cuv"[k % 3]))
    return out


def shape_cases(nx):
    """(grid, (a, kappa), kwargs, ds) of the table; the metric-free cases alternate between a grid that has Z metrics and
    one that has none"""
    cases = []
    for n, (lead, nz, ny, nx_, to, dtype, kform, mform, hpos) in enumerate(shape_table(nx)):
        grid, ds, dims = _grid(lead, nz, ny, nx_, dtype, metric=mform or (None, "1d")[n % 2], hpos=hpos)
        a = TD._field(lead, nz, ny, nx_, dtype, dims, hpos, nan=(nz + ny) % 4 == 0)
        kappa = _kappa(kform, lead, nz, ny, nx_, dtype, dims, to, hpos)
        cases.append((grid, (a, kappa), dict(dt=DT if mform else DT_PLAIN, to=to, metric_weighted=mform is not None), ds))
    return cases


def test_the_shape_table_meets_every_combination():
    rows = [r for nx in NXS for r in shape_table(nx)]
    seen = {(to, np.dtype(dt).name, kf, mf) for _, _, _, _, to, dt, kf, mf, _ in rows}
    assert seen == set(itertools.product(TOS, ("float64", "float32"), KFORMS, MFORMS))
    assert {r[0] for r in rows} == set(LEADS) and {r[8] for r in rows} == set("cuv")
    assert {r[1:4] for r in rows} == set(itertools.product(NZS, NYS, NXS))


def run_cases(monkeypatch, cases):
    calls = _counted(monkeypatch)
    for n, (grid, (a, kappa), kw, ds) in enumerate(cases):
        got = grid.implicit_vertical_diffusion(a, kappa, **kw)
        assert got.dims == a.dims and got.name == a.name and list(got.coords) == list(a.coords)
        _same_bits(got.values, _want_of(ds, a, kappa, kw["to"], kw["metric_weighted"], kw["dt"]))
        assert len(calls) == n + 1   # the one-pass entry served it


@pytest.mark.parametrize("nx", NXS)
def test_small_shapes(host_abi, monkeypatch, nx):
    cases = shape_cases(nx)
    assert len(cases) == len(NZS) * len(NYS)
    run_cases(monkeypatch, cases)


def long_column_cases():
    out = []
    for dtype, to in ((np.float64, "outer"), (np.float32, "left")):
        grid, ds, dims = _grid((), 90, 3, 130, dtype)
        out.append((grid, (TD._field((), 90, 3, 130, dtype, dims), _kappa("3d", (), 90, 3, 130, dtype, dims, to)),
                    dict(dt=DT, to=to, metric_weighted=True), ds))
    return out


def test_one_long_column(host_abi, monkeypatch):
    run_cases(monkeypatch, long_column_cases())


# ---- 3. properties at moderate coupling -----------------------------------------------------------------------------------
# measured on CPU on these inputs (printed by the test), relative to max|a| per test; asserted at 16 x the measured value
PROPERTY_MEASURED = {np.float64: {"constant": 1.332e-15, "budget": 2.322e-16, "residual": 1.779e-15},
                     np.float32: {"constant": 6.358e-7, "budget": 9.095e-8, "residual": 1.493e-6}}


def _property_case(dtype, to="outer"):
    nz, ny, nx = 17, 3, 5
    grid, ds, dims = _grid((), nz, ny, nx, dtype)
    return grid, ds, TD._field((), nz, ny, nx, dtype, dims), _kappa("3d", (), nz, ny, nx, dtype, dims, to)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_dt_zero_returns_the_field(host_abi, dtype):
    grid, ds, a, kappa = _property_case(dtype)
    assert (a.values != 0).all()   # (a -0.0 below level 0 becomes +0.0: -0.0 + 0 * d)
    for k in (kappa, None):
        _same_bits(grid.implicit_vertical_diffusion(a, k, dt=0.0).values, a.values)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_constants_stay_and_the_column_budget_holds(host_abi, dtype):
    grid, ds, a, kappa = _property_case(dtype)
    bound = PROPERTY_MEASURED[dtype]
    flat = grid.implicit_vertical_diffusion(a._replace(data=np.full(a.shape, 0.75, dtype)), kappa, dt=DT)
    e_const = _rel(flat.values, np.full(a.shape, 0.75))
    x = grid.implicit_vertical_diffusion(a, kappa, dt=DT).values.astype(np.float64)
    drf = ds["drF"].values.astype(np.float64)[:, None, None]
    total = (a.values.astype(np.float64) * drf).sum(axis=0)
    e_budget = float(np.abs((x * drf).sum(axis=0) - total).max() / np.abs(a.values.astype(np.float64) * drf).sum(axis=0).max())
    print(f"{np.dtype(dtype)}: constant {e_const:.3e}, budget {e_budget:.3e}")
    assert e_const <= 16 * bound["constant"] and e_budget <= 16 * bound["budget"]
    # the M-matrix: no new extremum in any column
    assert (np.abs(x).max(axis=0) <= np.abs(a.values).max(axis=0).astype(np.float64) * (1 + 16 * bound["constant"])).all()
    assert not np.array_equal(x, a.values)   # (and the solve did mix)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_the_explicit_operator_undoes_it(host_abi, dtype):
    """x - dt * vertical_diffusion(x, kappa, to="outer", padding="extend") is `a` again: the operator this one inverts"""
    grid, ds, a, kappa = _property_case(dtype)
    x = grid.implicit_vertical_diffusion(a, kappa, dt=DT)
    back = x.values - dtype(DT) * grid.vertical_diffusion(x, kappa, to="outer", padding="extend").values
    err = _rel(back, a.values)
    print(f"{np.dtype(dtype)}: residual {err:.3e}")
    assert err <= 16 * PROPERTY_MEASURED[dtype]["residual"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_left_is_outer_without_the_bottom_face(host_abi, monkeypatch, dtype):
    """faces 0 and n are never read: `left` equals `outer` with one more, arbitrary or NaN, bottom face, and a NaN in face 0
    changes nothing"""
    calls, dt = _counted(monkeypatch), 0.01   # unweighted: the coupling is dt * kappa <= 100
    grid, ds, a, kl = _property_case(dtype, "left")
    ref = grid.implicit_vertical_diffusion(a, kl, dt=dt, to="left", metric_weighted=False).values
    for bottom in (np.nan, 7.0):
        ko = DataArray(np.concatenate([kl.values, np.full((1,) + kl.shape[1:], bottom, dtype)]), ("ZO",) + kl.dims[1:])
        _same_bits(grid.implicit_vertical_diffusion(a, ko, dt=dt, to="outer", metric_weighted=False).values, ref)
        ko.values[0] = np.nan
        kl0 = kl._replace(data=np.concatenate([np.full((1,) + kl.shape[1:], np.nan, dtype), kl.values[1:]]))
        _same_bits(grid.implicit_vertical_diffusion(a, ko, dt=dt, to="outer", metric_weighted=False).values, ref)
        _same_bits(grid.implicit_vertical_diffusion(a, kl0, dt=dt, to="left", metric_weighted=False).values, ref)
    assert not np.isnan(ref).any() and len(calls) == 7


# ---- 4. NaN and Inf (device level: shared with the GPU suite) --------------------------------------------------------------
def nan_cases(dtype):
    """a NaN in `a` at one cell, in kappa at one interior face, in mc at one cell: exactly that column turns NaN -- at the
    first column, the last of the first x-tile's vector lanes, the first of the second tile and the last column of nx = 130"""
    import xgcm_amd.device as D

    nz, ny, nx = 5, 3, 130
    f = lambda shape, seed: R.synthetic_field(shape, seed).astype(dtype)  # noqa: E731
    base = {"a": f((nz, ny, nx), 201), "kappa": np.abs(f((nz + 1, ny, nx), 202)) * dtype(2e4),
            "mf": R.synthetic_metric((nz + 1, 1, 1), 203).astype(dtype), "mc": R.synthetic_metric((nz, ny, nx), 204).astype(dtype)}
    checked = 0
    for i, (name, k) in itertools.product((0, 127, 128, 129), (("a", 0), ("a", 4), ("kappa", 2), ("mc", 3))):
        arrays = {n: v.copy() for n, v in base.items()}
        arrays[name][k, 1, i] = np.nan
        got = D.tohost(D.implicit_vertical_diffusion(arrays["a"], arrays["kappa"], arrays["mf"], arrays["mc"], True, DT))
        mask = np.zeros((nz, ny, nx), bool)
        mask[:, 1, i] = True
        assert np.array_equal(np.isnan(got), mask), (name, k, i)
        _same_bits(got, statement(arrays["a"], arrays["kappa"], arrays["mf"], arrays["mc"], DT))
        checked += 1
    # an infinite kappa at one interior face: whatever the statement gives (the column's neighbours stay finite)
    arrays = {n: v.copy() for n, v in base.items()}
    arrays["kappa"][2, 1, 128] = np.inf
    got = D.tohost(D.implicit_vertical_diffusion(arrays["a"], arrays["kappa"], arrays["mf"], arrays["mc"], True, DT))
    _same_bits(got, statement(arrays["a"], arrays["kappa"], arrays["mf"], arrays["mc"], DT))
    assert np.isfinite(np.delete(got, 128, axis=2)).all()
    return checked


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_a_nan_poisons_exactly_its_column(host_abi, dtype):
    assert nan_cases(dtype) == 16


# ---- 5. the entry of the C ABI called directly, with views ----------------------------------------------------------------
NVS = {np.float64: 2, np.float32: 4}
TORCH = {np.float64: torch.float64, np.float32: torch.float32}
CODE = {np.float64: _hip.DTYPE["float64"], np.float32: _hip.DTYPE["float32"]}
ABI_NX = {np.float64: 132, np.float32: 264}   # one full 64-lane tile and a partial one
SENTINEL = 12345.5


def abi_dt(planes):
    """the coupling dt * kappa / (mf * mc) stays near 36 whichever of the metrics (1000 .. 2000 each) are there"""
    return DT * (1.0 if planes.get("mf") is not None else 1e-3) * (1.0 if planes.get("mc") is not None else 1e-3)


def _abi_call(D, dtype, shape, a, planes, to, out_off=ALIGNED, work_off=ALIGNED):
    """one call of xg_implicit_vertical_diffusion: `a` a contiguous view, `planes` {kappa, mf, mc} views or None; the result and
    the workspace are written `out_off` / `work_off` elements into allocations full of SENTINEL, which must still surround
    both afterwards"""
    fshape = shape[:-3] + [TD._nf(shape[-3], to)] + shape[-2:]
    args = [CODE[dtype], a.data_ptr()]
    for name, against in (("kappa", fshape), ("mf", fshape), ("mc", shape)):
        m = planes.get(name)
        if m is None:
            args += [None, None]
        else:
            assert all(n in (1, s) for n, s in zip(m.shape, against))
            args += [m.data_ptr(), _hip.i64([0 if n == 1 else m.stride(d) for d, n in enumerate(m.shape)])]
    n, dt = int(np.prod(shape)), abi_dt(planes)
    bufs = [torch.full((off + n + ALIGNED,), SENTINEL, dtype=TORCH[dtype], device=D._MEM.device) for off in (work_off, out_off)]
    work, out = (b[off:off + n] for b, off in zip(bufs, (work_off, out_off)))
    args += [work.data_ptr(), out.data_ptr(), _hip.i64(shape), len(shape), int(to == "outer"), dt]
    D._check(D._MEM.lib().xg_implicit_vertical_diffusion(*args, D._stream()))
    for b, off in zip(bufs, (work_off, out_off)):
        whole = b.cpu().numpy()
        assert (whole[:off] == SENTINEL).all() and (whole[off + n:] == SENTINEL).all()
    return whole[out_off:out_off + n].reshape(shape)


def abi_layout_cases(dtype):
    """Runs the direct-ABI table on whatever library `xgcm_amd.device._MEM` serves.  Every input view lives in a NaN-filled
    allocation, so a read outside it shows in the result; the contiguous, aligned control of each set of planes is compared
    with the statement, every other layout with that control."""
    import xgcm_amd.device as D

    nv = NVS[dtype]
    shape = [2, 5, 7, ABI_NX[dtype]]
    lead, nz, ny, nx = shape
    av = R.synthetic_field(tuple(shape), 101).astype(dtype)
    av.reshape(-1)[5::1700] = np.nan
    put = lambda x, st=None, off=ALIGNED: _strided(D, x, st or _contig(x.shape), off)  # noqa: E731
    for to in TOS:
        nf = TD._nf(nz, to)
        levels = {"kappa": nf, "mf": nf, "mc": nz}

        def vals(name, form, seed):
            n = levels[name]
            sh = {"z": (1, n, 1, 1), "p": (1, 1, ny, nx), "v3": (1, n, ny, nx), "vl": (lead, n, ny, nx)}[form]
            if name == "kappa":
                return (np.abs(R.synthetic_field(sh, seed)) * 2e4).astype(dtype)
            return R.synthetic_metric(sh, seed).astype(dtype)

        a = put(av)
        assert a.is_contiguous() and a.data_ptr() % 16 == 0
        for present in ({"kappa": "v3"}, {"kappa": "z"}, {"kappa": "vl", "mf": "z", "mc": "z"}, {"mf": "v3", "mc": "p"},
                        {"kappa": "p", "mc": "vl"}, {"kappa": "v3", "mf": "vl", "mc": "v3"}, {}):
            pv = {n: vals(n, form, 111 + i) for i, (n, form) in enumerate(present.items())}
            aligned = {n: put(x) for n, x in pv.items()}
            control = _abi_call(D, dtype, shape, a, aligned, to)
            want = statement(av, pv.get("kappa"), pv.get("mf"), pv.get("mc"), abi_dt(pv))
            assert control.dtype == want.dtype == np.dtype(dtype) and np.array_equal(control, want, equal_nan=True), (to, present)
            assert np.isnan(control).sum() == np.isnan(av).any(axis=1).sum() * nz   # whole columns, and only they
            views = []
            # the field, the result, the workspace one element into their allocations, each alone and all three together:
            # any of them takes the narrow form
            a1 = put(av, off=1)
            assert a1.data_ptr() % 16 == av.dtype.itemsize
            views += [(a1, aligned, ALIGNED, ALIGNED), (a, aligned, 1, ALIGNED), (a, aligned, ALIGNED, 1), (a1, aligned, 1, 1)]
            # the planes one element in; with an odd row pitch; with an odd level pitch (volumes)
            views.append((a, {n: put(x, off=1) for n, x in pv.items()}, ALIGNED, ALIGNED))
            pitched = {}
            for n, x in pv.items():
                s = list(x.shape)
                st = _contig(s[:-1] + [s[-1] + 1]) if s[-1] > 1 else _contig(s)
                pitched[n] = put(x, st)
                assert s[-1] == 1 or (pitched[n].stride(-2) == nx + 1 and pitched[n].stride(-1) == 1)
            views.append((a, pitched, ALIGNED, ALIGNED))
            for n, form in present.items():
                x = pv[n]
                if form in ("v3", "vl"):
                    st = [(x.shape[1] * (ny * nx + 1)) * (x.shape[0] > 1), ny * nx + 1, nx, 1]
                    lev = put(x, [s or 1 for s in st])
                    assert lev.stride(1) == ny * nx + 1
                    views.append((a, dict(aligned, **{n: lev}), ALIGNED, ALIGNED))
                if form == "z":   # the Z-only array three elements apart
                    views.append((a, dict(aligned, **{n: put(x, [3 * x.shape[1], 3, 1, 1], 1)}), ALIGNED, ALIGNED))
                if form == "p":   # the plane stored (X, Y): a transposed view
                    t = put(np.ascontiguousarray(x.transpose(0, 1, 3, 2))).permute(0, 1, 3, 2)
                    assert t.stride(-1) == ny and t.stride(-2) == 1
                    views.append((a, dict(aligned, **{n: t}), ALIGNED, ALIGNED))
            for fa, planes, out_off, work_off in views:
                got = _abi_call(D, dtype, shape, fa, planes, to, out_off, work_off)
                assert np.array_equal(got, control, equal_nan=True), (to, present, out_off, work_off)
        # stride 0 along X and Y: one value per level, expanded over the whole volume, equals the Z-only array
        for name in ("kappa", "mf", "mc"):
            z = vals(name, "z", 121)
            flat = put(z).expand(1, levels[name], ny, nx)
            assert flat.stride(-1) == 0 and flat.stride(-2) == 0
            full = put(np.ascontiguousarray(np.broadcast_to(z, (1, levels[name], ny, nx))))
            assert np.array_equal(_abi_call(D, dtype, shape, a, {name: flat}, to), _abi_call(D, dtype, shape, a, {name: full}, to),
                                  equal_nan=True)
    assert nx % nv == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_abi_layouts(host_abi, dtype):
    abi_layout_cases(dtype)


# ---- 6. bad calls ---------------------------------------------------------------------------------------------------------
def abi_bad_calls():
    """bad calls return the header's codes and write nothing; runs on whatever library `_MEM` serves"""
    import xgcm_amd.device as D

    lib = D._MEM.lib()
    shape = [2, 3, 4]
    t = torch.ones(shape, dtype=torch.float64, device=D._MEM.device)
    out, work = torch.full_like(t, SENTINEL), torch.full_like(t, SENTINEL)
    P = lambda x: None if x is None else x.data_ptr()  # noqa: E731

    def call(code=CODE[np.float64], a=t, o=out, w=work, shp=shape, ndim=3, outer=0, dt=1.0, kappa=None, ks=None):
        return lib.xg_implicit_vertical_diffusion(code, P(a), P(kappa), ks, None, None, None, None, P(w), P(o),
                                                  None if shp is None else _hip.i64(shp), ndim, outer, dt, D._stream())

    def untouched():
        return bool((out == SENTINEL).all()) and bool((work == SENTINEL).all())

    for code in (-1, _hip.DTYPE["float16"], _hip.DTYPE["int64"], _hip.DTYPE["int32"], 12, 99):
        assert call(code=code) == -1                                          # any other element type: XG_ERR_INVALID
    assert call(a=None) == -1 and call(o=None) == -1 and call(w=None) == -1 and call(shp=None) == -1   # NULL arguments
    assert call(outer=2) == -1 and call(outer=-1) == -1                       # unknown flux position
    assert call(kappa=t, ks=None) == -1                                       # a plane without strides
    for dt in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        assert call(dt=dt) == -1                                              # dt negative, NaN or infinite
    assert call(ndim=2) < 0 and call(ndim=2) != -1                            # XG_ERR_UNSUPPORTED
    assert untouched()
    assert call(shp=[2, 0, 4]) == 0 and call(shp=[0, 3, 4]) == 0 and untouched()   # an empty extent: XG_OK, nothing touched
    assert call() == 0 and call(outer=1, dt=0.0) == 0 and call(kappa=t, ks=_hip.i64([12, 4, 1])) == 0 and not untouched()


def test_abi_refuses_bad_calls(host_abi):
    abi_bad_calls()


# ---- 7. the Grid surface ----------------------------------------------------------------------------------------------------
def _case(lead=(2,), nz=4, ny=5, nx=6, dtype=np.float64, to="outer", kform="3d", **gk):
    grid, ds, dims = _grid(lead, nz, ny, nx, dtype, **gk)
    return grid, ds, TD._field(lead, nz, ny, nx, dtype, dims), _kappa(kform, lead, nz, ny, nx, dtype, dims, to)


def test_xarray_in_xarray_out(host_abi, monkeypatch):
    import xarray_standin

    xarray_standin.install(monkeypatch)
    import xarray as xr

    grid, ds, a, kappa = _case(lead=())
    got = grid.implicit_vertical_diffusion(*(xr.DataArray(x.values, dims=x.dims, name=x.name) for x in (a, kappa)), dt=DT)
    assert type(got).__module__.split(".")[0] == "xarray"
    assert tuple(got.dims) == a.dims and got.name == "T"
    _same_bits(np.asarray(got.values), _want_of(ds, a, kappa, "outer", True))


def test_dims_coords_and_name_are_the_fields(host_abi, monkeypatch):
    calls = _counted(monkeypatch)
    for name, to, mw in (("T", "outer", True), (None, "left", True), ("drF", "outer", False)):
        grid, ds, a, kappa = _case(to=to)
        a = a._replace(name=name).assign_coords({"lon": (("YC", "XC"), np.ones((5, 6))), "t2": (("time",), np.arange(2) + 7.0),
                                                 "depth": (("ZC",), np.arange(4) * 10.0)})
        kappa = kappa.assign_coords({"depth_f": ((TD.ZDIM[to],), np.arange(TD._nf(4, to)) * 10.0)})
        dt = DT if mw else DT_PLAIN
        got = grid.implicit_vertical_diffusion(a, kappa, dt=dt, to=to, metric_weighted=mw)
        TD._same_labelled(got, a._replace(data=_want_of(ds, a, kappa, to, mw, dt)))
    assert len(calls) == 3


def test_kappa_with_its_dims_in_another_order_is_read_in_place(host_abi, monkeypatch):
    calls = _counted(monkeypatch)
    grid, ds, a, kappa = _case(kform="lead", to="left")
    got = grid.implicit_vertical_diffusion(a, kappa.transpose("XC", "ZL", "time", "YC"), dt=DT, to="left")
    _same_bits(got.values, _want_of(ds, a, kappa, "left", True))
    yx = DataArray(np.abs(R.synthetic_field((5, 6), 77)) * 1e4, ("YC", "XC"), name="kappa")   # no Z dim: the same plane at every face
    got = grid.implicit_vertical_diffusion(a, yx, dt=DT)
    _same_bits(got.values, statement(a.values, yx.values[None, None], ds["drCo"].values[None, :, None, None],
                                     ds["drF"].values[None, :, None, None], DT))
    assert len(calls) == 2


def test_to_defaults_to_outer_when_the_axis_has_it_else_left(host_abi, monkeypatch):
    calls = _counted(monkeypatch)
    grid, ds, a, ko = _case()
    _same_bits(grid.implicit_vertical_diffusion(a, ko, dt=DT).values, _want_of(ds, a, ko, "outer", True))
    axes = dict(TD.AXES, Z={"center": "ZC", "left": "ZL"})
    g2, ds2, dims = _grid((2,), 4, 5, 6, np.float64, axes=axes, metric=None)
    kl = _kappa("3d", (2,), 4, 5, 6, np.float64, dims, "left")
    _same_bits(g2.implicit_vertical_diffusion(a, kl, dt=DT_PLAIN, metric_weighted=False).values,
               statement(a.values, kl.values, None, None, DT_PLAIN))
    assert len(calls) == 2


def test_the_fused_entry_runs_alone(host_abi, monkeypatch):
    """one call of the one-pass device entry and none of the one-axis operators"""
    import xgcm_amd.device as D

    grid, ds, a, kappa = _case()
    calls = {"fused": 0, "other": 0}

    def counted(fn, key):
        def wrapped(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(D, "implicit_vertical_diffusion", counted(D.implicit_vertical_diffusion, "fused"))
    for name in ("binary", "stencil1d"):
        monkeypatch.setattr(D, name, counted(getattr(D, name), "other"))
    out = grid.implicit_vertical_diffusion(a, kappa, dt=DT)
    _same_bits(out.values, _want_of(ds, a, kappa, "outer", True))
    assert calls == {"fused": 1, "other": 0}


# the level loop: everything the kernel does not serve, bit for bit the statement
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_z_elsewhere_or_fewer_than_three_dims_run_the_level_loop(host_abi, monkeypatch, dtype):
    _no_fused(monkeypatch)
    grid, ds, a, kappa = _case(dtype=dtype)
    want = _want_of(ds, a, kappa, "outer", True)
    for order in (("ZC", "time", "YC", "XC"), ("time", "YC", "ZC", "XC"), ("XC", "YC", "time", "ZC")):
        got = grid.implicit_vertical_diffusion(a.transpose(*order), kappa, dt=DT)
        assert got.dims == order and got.name == "T"
        _same_bits(got.transpose(*a.dims).values, want)
    # (Z, Y): the column of every row; (Z,): one column, a profile kappa
    zy = DataArray(np.ascontiguousarray(a.values[0, :, :, 0]), ("ZC", "YC"), name="T")
    kzy = DataArray(np.ascontiguousarray(kappa.values[:, :, 0]), ("ZO", "YC"), name="kappa")
    mf, mc = ds["drCo"].values[:, None, None], ds["drF"].values[:, None, None]
    for weighted in (True, False):
        dt = DT if weighted else DT_PLAIN
        got = grid.implicit_vertical_diffusion(zy, kzy, dt=dt, metric_weighted=weighted)
        assert got.dims == ("ZC", "YC") and np.isfinite(got.values).all()
        _same_bits(got.values[:, :, None], statement(zy.values[:, :, None], kzy.values[:, :, None],
                                                     mf if weighted else None, mc if weighted else None, dt))
    z1 = DataArray(np.ascontiguousarray(a.values[0, :, 0, 0]), ("ZC",), name="T")
    k1 = _kappa("1d", (), 4, 5, 6, dtype, (), "outer")
    for k in (k1, None):
        got = grid.implicit_vertical_diffusion(z1, k, dt=DT)
        _same_bits(got.values[:, None, None], statement(z1.values[:, None, None], None if k is None else k.values[:, None, None], mf, mc, DT))


def test_a_kappa_or_a_metric_with_a_dim_the_field_lacks_runs_the_level_loop(host_abi, monkeypatch):
    """the result has that dim in front of the field's"""
    _no_fused(monkeypatch)
    grid, ds, a, kappa = _case(lead=())
    extra = DataArray(np.stack([kappa.values, kappa.values * 0.5]), ("member",) + kappa.dims, name="kappa")
    got = grid.implicit_vertical_diffusion(a, extra, dt=DT)
    assert got.dims == ("member",) + a.dims and got.name == "T"
    for n in range(2):
        _same_bits(got.values[n], _want_of(ds, a, extra._replace(data=extra.values[n], dims=kappa.dims), "outer", True))
    coords = {k: (k, np.asarray(ds.coords[k].values)) for k in ("XC", "XG", "YC", "YG", "ZC", "ZL", "ZO")}
    coords["time"] = ("time", np.arange(2) * 2.0)
    data = {"drF": (("ZC", "time"), R.synthetic_metric((4, 2), 66)), "drCo": (("ZO", "time"), R.synthetic_metric((5, 2), 67))}
    g2 = Grid(Dataset(data, coords), coords=TD.AXES, metrics={("Z",): ["drF", "drCo"]},
              padding={"X": "periodic", "Y": "periodic", "Z": "extend"}, autoparse_metadata=False)
    got = g2.implicit_vertical_diffusion(a, kappa, dt=DT)
    assert got.dims == ("time",) + a.dims
    # (the metrics are whatever the lookup returns at the flux' and at the field's dims, here with "time")
    f_dims, dims = ("time", "ZO", "YC", "XC"), ("time",) + a.dims
    mf, mc = (g2.get_metric(_DimsOnly(d[1:]), ("Z",)) for d in (f_dims, dims))
    assert "time" in mf.dims and "time" in mc.dims
    _same_bits(got.values, statement(np.broadcast_to(a.values, (2,) + a.shape).copy(), kappa.values[None], TD._aligned(mf, f_dims),
                                     TD._aligned(mc, dims), DT))


# the refusals of the docstring
@pytest.mark.parametrize("dt", [-1.0, -1e-300, float("nan"), float("inf"), float("-inf")])
def test_a_bad_dt_raises_on_the_host(host_abi, monkeypatch, dt):
    _no_fused(monkeypatch)
    grid, ds, a, kappa = _case()
    with pytest.raises(ValueError, match="dt must be finite and not negative"):
        grid.implicit_vertical_diffusion(a, kappa, dt=dt)


def test_a_missing_dt_raises(host_abi):
    grid, ds, a, kappa = _case()
    with pytest.raises(TypeError, match="dt, the time step, is required"):
        grid.implicit_vertical_diffusion(a, kappa)


@pytest.mark.parametrize("dtype", [np.int64, np.int32, np.bool_, np.float16])
def test_integer_bool_and_half_fields_raise(host_abi, monkeypatch, dtype):
    _no_fused(monkeypatch)
    grid, ds, a, kappa = _case()
    ai = DataArray((a.values * 100).astype(dtype), a.dims, name="T")
    with pytest.raises(TypeError, match="has no exact solve"):
        grid.implicit_vertical_diffusion(ai, None, dt=DT, metric_weighted=False)


def test_mixed_dtypes_raise(host_abi, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, a, kappa = _case(dtype=np.float32, mdtype=np.float64)
    with pytest.raises(TypeError, match="mixed dtypes.*metric"):
        grid.implicit_vertical_diffusion(a, kappa, dt=DT)                                   # float32 over float64 metrics
    with pytest.raises(TypeError, match="mixed dtypes.*kappa"):
        grid.implicit_vertical_diffusion(a, kappa._replace(data=kappa.values.astype(np.float64)), dt=DT, metric_weighted=False)
    with pytest.raises(TypeError, match="labelled arrays"):
        grid.implicit_vertical_diffusion(a, 2.0, dt=DT, metric_weighted=False)              # a plain number


def test_chunked_inputs_raise(host_abi, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, dims = _grid((4,), 3, 6, 8, np.float64)
    a = TD._field((4,), 3, 6, 8, np.float64, dims)
    kappa = _kappa("lead", (4,), 3, 6, 8, np.float64, dims, "outer")
    ca = DataArray(BlockArray.from_array(a.values, ((2, 2), (3,), (6,), (8,))), a.dims, name="T")
    ck = DataArray(BlockArray.from_array(kappa.values, ((2, 2), (4,), (6,), (8,))), kappa.dims, name="kappa")
    for x, k in ((ca, kappa), (a, ck)):
        with pytest.raises(NotImplementedError, match="chunked inputs are not served"):
            grid.implicit_vertical_diffusion(x, k, dt=DT)


def test_positions_that_do_not_fit_raise(host_abi, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, a, kappa = _case()
    for to in ("right", "inner", "center", "nowhere"):
        with pytest.raises(ValueError, match="flux position must be 'left' or 'outer'"):
            grid.implicit_vertical_diffusion(a, None, dt=DT, to=to)
    axes = dict(TD.AXES, Z={"center": "ZC", "left": "ZL"})
    g2, _, _ = _grid((2,), 4, 5, 6, np.float64, axes=axes, metric=None)
    with pytest.raises(ValueError, match="flux position must be 'left' or 'outer'"):
        g2.implicit_vertical_diffusion(a, None, dt=DT, to="outer", metric_weighted=False)   # a position the axis lacks
    with pytest.raises(ValueError, match="must sit at Z:center"):
        grid.implicit_vertical_diffusion(DataArray(a.values, ("time", "ZL", "YC", "XC"), name="T"), None, dt=DT)
    with pytest.raises(ValueError, match="must sit at the flux position"):
        grid.implicit_vertical_diffusion(a, DataArray(kappa.values[:4], ("ZC", "YC", "XC")), dt=DT)
    with pytest.raises(ValueError, match="must sit at the flux position"):
        grid.implicit_vertical_diffusion(a, DataArray(kappa.values[:4], ("ZL", "YC", "XC")), dt=DT, to="outer")
    with pytest.raises(ValueError, match="has 4 entries along 'ZO', the flux has 5"):
        grid.implicit_vertical_diffusion(a, DataArray(kappa.values[:4], ("ZO", "YC", "XC")), dt=DT)


def test_a_missing_metric_raises_the_lookups_error_and_is_served_unweighted(host_abi, monkeypatch):
    calls = _counted(monkeypatch)
    grid, ds, a, kappa = _case(metric=None)
    with pytest.raises((KeyError, ValueError)):
        grid.implicit_vertical_diffusion(a, kappa, dt=DT)
    assert not calls
    _same_bits(grid.implicit_vertical_diffusion(a, kappa, dt=DT_PLAIN, metric_weighted=False).values,
               statement(a.values, kappa.values[None], None, None, DT_PLAIN))
    assert len(calls) == 1


def test_faces_connected_along_z_raise(host_abi, monkeypatch):
    from test_topology import COORDS

    _no_fused(monkeypatch)
    ds = Dataset({"drF": (("zc",), R.synthetic_metric((4,), 63)), "drC": (("zl",), R.synthetic_metric((4,), 64))},
                 coords={"x": np.arange(4), "xl": np.arange(4) - 0.5, "y": np.arange(4), "yl": np.arange(4) - 0.5,
                         "face": np.arange(2), "zc": np.arange(4) + 0.5, "zl": np.arange(4) * 1.0})
    grid = Grid(ds, coords=dict(COORDS, Z={"center": "zc", "left": "zl"}), face_connections=TD.Z_TO_Z,
                metrics={("Z",): ["drF", "drC"]}, padding={"X": "periodic", "Y": "extend", "Z": "fill"}, autoparse_metadata=False)
    a = DataArray(R.synthetic_field((2, 4, 4, 4), 82), ("face", "zc", "y", "x"), name="T")
    with pytest.raises(NotImplementedError, match="face connections or a fold along 'Z'"):
        grid.implicit_vertical_diffusion(a, None, dt=DT)


def test_a_fold_along_z_raises(host_abi, monkeypatch):
    import warnings

    _no_fused(monkeypatch)
    nz, ny, nx = 4, 3, 6
    ds = Dataset({"drF": (("zc",), R.synthetic_metric((nz,), 63)), "drC": (("zl",), R.synthetic_metric((nz,), 64))},
                 coords={"xh": np.arange(nx), "xl": np.arange(nx), "yh": np.arange(ny), "yl": np.arange(ny),
                         "zc": np.arange(nz) + 0.5, "zl": np.arange(nz) * 1.0})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        grid = Grid(ds, coords={"X": {"center": "xh", "left": "xl"}, "Y": {"center": "yh", "left": "yl"},
                                "Z": {"center": "zc", "left": "zl"}}, metrics={("Z",): ["drF", "drC"]},
                    padding={"X": "periodic", "Y": "extend", "Z": {"fold": "corner"}}, autoparse_metadata=False)
        a = DataArray(R.synthetic_field((2, nz, ny, nx), 92), ("t", "zc", "yh", "xh"), name="T")
        with pytest.raises(NotImplementedError, match="face connections or a fold along 'Z'"):
            grid.implicit_vertical_diffusion(a, None, dt=DT)
