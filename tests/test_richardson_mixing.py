"""The Pacanowski-Philander mixing coefficients at the faces of Z, `Grid.richardson_mixing`, on CPU.

The one-pass path runs through the `host_abi` fixture (the product's `xgcm_amd.device` over libxgcm_host.so); the chain it
replaces

    s2 = grid.vertical_shear_squared(u, v, ...);  n2 = step(b, Z, to);  ri = n2 / (s2 + shear_floor)
    rp = (ri + abs(ri)) * 0.5;  den = 1.0 + alpha * rp;  nu = nu0 / (den * den) + nu_b;  kappa = nu / den + kappa_b

runs through the same Grid over the oracle double, installed AFTER the one-pass calls of a test have run, with s2 written out
as its own chain (the double has no one-pass entry).  `Mix.want` states the chain a third time: the oracle's one-axis
functions up to n2 and s2, then plain numpy in the fields' dtype.  Values are compared bit for bit (NaN = NaN, -0.0 is not
+0.0), with dims, coords and names.  The case tables are those of tests/test_richardson_number.py, each case with one of
`SCALARS`; the builders and the direct-ABI cases are shared with the GPU suite.

`Mix.not_hollow` asserts on the REFERENCE alone, in every case without an injected NaN and without a NaN fill:
  * with a positive `shear_floor` both results are finite everywhere;
  * under `fill` on Z with two levels or more and at least 64 interior result cells, a quarter of the interior faces or more
    have Ri > RI_CLEAR = 2^-16 (stricter than Ri > 0: there the closure visibly departs from its maximum) and a quarter or
    more Ri < 0;
  * nu != kappa - kappa_b on every face with Ri > 0 when alpha > 0 (alpha = 0 makes den exactly 1 and the two equal, so the
    statement is impossible there)."""

import itertools

import numpy as np
import pytest
import torch

import guarded_memory as GM
import test_richardson_number as TR
from oracle import refimpl as R
from test_fused_layouts import ALIGNED, _contig, _strided
from xgcm_amd import DataArray, _hip

FLOOR = 2.0 ** -10
RI_CLEAR = 2.0 ** -16
DEFAULTS = dict(nu0=5e-3, alpha=5.0, nu_b=1e-4, kappa_b=1e-5, shear_floor=0.0)
# the scalar sets the tables rotate through: the defaults over a floor, other values of all five, integers, alpha = 0, and
# the defaults with no floor (0 / 0 stays NaN)
SCALARS = [dict(shear_floor=FLOOR), dict(nu0=1.25e-2, alpha=10.0, nu_b=3e-5, kappa_b=2e-6, shear_floor=2.0 ** -8),
           dict(nu0=1, alpha=2, nu_b=0, kappa_b=0, shear_floor=FLOOR), dict(alpha=0, shear_floor=FLOOR), dict()]
_same_labelled, _same_bits = TR._same_labelled, TR._same_bits


def closure(n2, s2, nu0, alpha, nu_b, kappa_b, shear_floor):
    """(nu, kappa, ri) of the closure over numpy arrays, every operation in their dtype, each scalar cast to it once"""
    t = n2.dtype.type
    with np.errstate(all="ignore"):
        ri = n2 / (s2 + t(shear_floor))
        rp = (ri + np.abs(ri)) * t(0.5)
        den = t(1.0) + t(alpha) * rp
        nu = t(nu0) / (den * den) + t(nu_b)
        kappa = nu / den + t(kappa_b)
    assert nu.dtype == kappa.dtype == n2.dtype
    return nu, kappa, ri


def _chain(grid, b, u, v, nu0=5e-3, alpha=5.0, nu_b=1e-4, kappa_b=1e-5, shear_floor=0.0, x_axis="X", y_axis="Y", z_axis="Z",
           to=None, padding=None, fill_value=None, metric_weighted=True, s2_written_out=True):
    """the specification.  `s2_written_out`: the squared shear as its own chain (under the oracle double, which has no
    one-pass entry) instead of `grid.vertical_shear_squared`"""
    kw = dict(padding=padding, fill_value=fill_value)
    step = grid.derivative if metric_weighted else grid.diff
    if to is None:
        to = "outer" if "outer" in grid.axes[z_axis].coords else "left"
    if s2_written_out:
        s2 = TR._chain(grid, None, u, v, x_axis, y_axis, z_axis, to=to, metric_weighted=metric_weighted, **kw)
    else:
        s2 = grid.vertical_shear_squared(u, v, x_axis, y_axis, z_axis, to=to, metric_weighted=metric_weighted, **kw)
    n2 = step(b, z_axis, to=to, **kw)
    ri = n2 / (s2 + shear_floor)
    rp = (ri + abs(ri)) * 0.5
    den = 1.0 + alpha * rp
    nu = nu0 / (den * den) + nu_b
    kappa = nu / den + kappa_b
    return nu, kappa


class Mix:
    """one call of the operator: a case of tests/test_richardson_number.py and the closure's scalars"""

    def __init__(self, case, scalars):
        self.c, self.given = case, dict(scalars)
        self.s = dict(DEFAULTS, **scalars)

    def __repr__(self):
        return f"{self.c} {self.given}"

    def one_pass(self):
        return self.c.grid.richardson_mixing(*self.c.f, **self.given, **self.c.kw)

    def chain(self, **kw):
        return _chain(self.c.grid, *self.c.f, **self.given, **self.c.kw, **kw)

    def want(self):
        """(nu, kappa, ri, n2, s2) of the numpy statement"""
        c = self.c
        fill = c.kw["fill_value"] or {"X": 0.0, "Y": 0.0, "Z": 0.0}
        mets = TR._metrics_of(c.ds, c.metric if c.kw["metric_weighted"] else None, c.to, c.dims)
        b, u, v = (a.values for a in c.f)
        s2 = TR._want(None, u, v, c.pads, c.to, fill, *mets[:2])
        n2 = R.stencil1d("diff", b, b.ndim - 3, 1, 1 if c.to == "outer" else 0, c.pads[2], fill["Z"], m_out=mets[2])
        return closure(n2, s2, **self.s) + (n2, s2)

    def not_hollow(self, nu, kappa, ri, n2, s2):
        """the module docstring's statements about the reference; returns 1 when the sign statement was made"""
        c, t = self.c, np.asarray(nu).dtype.type
        fill = c.kw["fill_value"] or {}
        if c.nan or any(np.isnan(x) for x in fill.values()):
            return 0
        if self.s["shear_floor"] > 0:
            assert np.isfinite(nu).all() and np.isfinite(kappa).all(), self
        if self.s["alpha"] > 0:
            with np.errstate(invalid="ignore"):
                stable = ri > 0
                assert (nu[stable] != kappa[stable] - t(self.s["kappa_b"])).all(), self
        inner = ri[..., 1:c.nz, :, :]
        if c.pads[2] == "fill" and c.nz >= 2 and inner.size >= 64:
            assert (inner > RI_CLEAR).mean() >= 0.25 and (inner < 0).mean() >= 0.25, (self, (inner > RI_CLEAR).mean(), (inner < 0).mean())
            return 1
        return 0

    def properties(self, nu, kappa):
        """the closure's properties on a RESULT: the maximum, exactly, wherever the reference's N2 is negative and finite
        over a finite positive S2 + floor (the column is statically unstable); elsewhere finite within [nu_b, nu0 + nu_b]"""
        _, _, ri, n2, s2 = self.want()
        t = n2.dtype.type
        nu, kappa = np.asarray(nu), np.asarray(kappa)
        with np.errstate(invalid="ignore"):
            under = s2 + t(self.s["shear_floor"])
            unstable = (n2 < 0) & np.isfinite(n2) & np.isfinite(under) & (under > 0)
            top = t(self.s["nu0"]) + t(self.s["nu_b"])
            assert (nu[unstable] == top).all() and (kappa[unstable] == top + t(self.s["kappa_b"])).all(), self
            rest = np.isfinite(nu) & ~unstable
            assert (nu[rest] >= t(self.s["nu_b"])).all() and (nu[rest] <= top).all(), self
        return int(unstable.sum())


def mixed(cases, start=0):
    """the cases of a table of tests/test_richardson_number.py, the scalar sets rotating"""
    return [Mix(c, SCALARS[(start + n) % len(SCALARS)]) for n, c in enumerate(cases)]


def _counted(monkeypatch, bar_chain=False):
    """the calls of the one-pass device entry; `bar_chain`: and those of the chain's own device functions"""
    import xgcm_amd.device as D

    calls = {"fused": 0, "chain": 0}

    def counted(fn, key):
        def wrapped(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(D, "richardson_mixing", counted(D.richardson_mixing, "fused"))
    if bar_chain:
        for name in ("binary", "stencil1d", "richardson_number"):
            monkeypatch.setattr(D, name, counted(getattr(D, name), "chain"))
    return calls


def compare_with_numpy(cases, monkeypatch=None):
    """both results of every case against the numpy statement, bit for bit, and the closure's properties on them; on whatever
    library `_MEM` serves.  With `monkeypatch`: exactly one call of the one-pass entry per case and none of the chain's.
    Returns (cases whose sign statement was made, unstable cells met)"""
    calls = _counted(monkeypatch, bar_chain=True) if monkeypatch is not None else None
    solid = unstable = 0
    for m in cases:
        (nu, kappa), want = m.one_pass(), m.want()
        try:
            _same_bits(nu.values, want[0])
            _same_bits(kappa.values, want[1])
            assert nu.dims == kappa.dims == m.c.dims + (TR.ZDIM[m.c.to], "YC", "XC")
            unstable += m.properties(nu.values, kappa.values)
        except AssertionError as err:
            raise AssertionError(f"case {m}") from err
        solid += m.not_hollow(*want)
    if calls is not None:
        assert calls == {"fused": len(cases), "chain": 0}
    return solid, unstable


def compare_with_chain(monkeypatch, cases):
    """every one-pass call first (counted), then the chain over the oracle double: values, dims, coords and names"""
    from oracle import fake_device

    calls = _counted(monkeypatch, bar_chain=True)
    got = [m.one_pass() for m in cases]
    assert calls == {"fused": len(cases), "chain": 0}
    fake_device.install(monkeypatch)
    for m, (nu, kappa) in zip(cases, got):
        with np.errstate(all="ignore"):
            want_nu, want_kappa = m.chain()
        try:
            _same_labelled(nu, want_nu)
            _same_labelled(kappa, want_kappa)
            _same_bits(nu.values, want_nu.values)
            _same_bits(kappa.values, want_kappa.values)
        except AssertionError as err:
            raise AssertionError(f"case {m}") from err


# ---- 1. against the numpy statement and against the chain ------------------------------------------------------------------
@pytest.mark.parametrize("px,py,pz", TR.PADS3)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_equals_the_chain(host_abi, monkeypatch, px, py, pz, dtype):
    compare_with_chain(monkeypatch, mixed(TR.matrix_cases((px, py, pz), dtype), TR.PADS3.index((px, py, pz))))


@pytest.mark.parametrize("px,py,pz", TR.PADS3)
def test_equals_the_numpy_statement(host_abi, monkeypatch, px, py, pz):
    cases = [m for dtype in (np.float64, np.float32) for m in mixed(TR.matrix_cases((px, py, pz), dtype), TR.PADS3.index((px, py, pz)))]
    solid, unstable = compare_with_numpy(cases, monkeypatch)
    assert unstable > 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_metric_forms_and_leading_dims(host_abi, monkeypatch, dtype):
    cases = mixed(TR.metric_cases(dtype))
    solid, unstable = compare_with_numpy(cases)
    assert solid > 0 and unstable > 0
    compare_with_chain(monkeypatch, cases)


def test_coords_and_names_follow_the_chain(host_abi, monkeypatch):
    cases = []
    for names in (("b", "u", "v"), ("q", "q", "q"), ("drCo", "drCo", "drCo"), (None, "v", None), ("hCo", "hWo", "hSo")):
        for metric, to in (("1d", "outer"), ("full", "outer"), ("full", "left"), (None, "left")):
            c = TR.Case((2,), 3, 5, 6, np.float64, ("periodic", "extend", "fill"), to, metric)
            f = [a._replace(name=n) for a, n in zip(c.f, names)]
            f[1] = f[1].assign_coords({"lonW": (("YC", "XG"), np.ones((5, 6))), "t2": (("time",), np.arange(2) + 7.0)})
            f[0] = f[0].assign_coords({"depth": (("ZC",), np.arange(3) * 10.0), "t2": (("time",), np.arange(2) + 9.0),
                                       "lonC": (("YC", "XC"), np.ones((5, 6)))})
            c.f = tuple(f)
            cases.append(c)
    compare_with_chain(monkeypatch, mixed(cases))


def test_xarray_in_xarray_out(host_abi, monkeypatch):
    import xarray_standin
    from oracle import fake_device

    xarray_standin.install(monkeypatch)
    import xarray as xr

    m = Mix(TR.Case((), 3, 4, 6, np.float64, ("periodic", "fill", "extend"), "left"), SCALARS[1])
    xs = [xr.DataArray(a.values, dims=a.dims, name=a.name) for a in m.c.f]
    got = m.c.grid.richardson_mixing(*xs, **m.given, **m.c.kw)
    assert len(got) == 2 and all(type(g).__module__.split(".")[0] == "xarray" for g in got)
    fake_device.install(monkeypatch)
    for g, w in zip(got, m.chain()):
        assert tuple(g.dims) == tuple(w.dims) and g.name == w.name
        _same_bits(np.asarray(g.values), np.asarray(w.values))


def test_to_defaults_to_outer_when_the_axis_has_it(host_abi, monkeypatch):
    calls = _counted(monkeypatch)
    m = Mix(TR.Case((), 3, 4, 6, np.float64, ("periodic", "fill", "extend"), "outer"), SCALARS[0])
    nu, kappa = m.c.grid.richardson_mixing(*m.c.f, **m.given, fill_value=TR.FILL)
    assert nu.dims == kappa.dims == ("ZO", "YC", "XC") and calls["fused"] == 1
    want = m.want()
    _same_bits(nu.values, want[0])
    _same_bits(kappa.values, want[1])


# ---- 2. the smallest shapes at which it can go wrong ----------------------------------------------------------------------
@pytest.mark.parametrize("nx", TR.NXS)
def test_small_shapes(host_abi, monkeypatch, nx):
    cases = mixed(TR.shape_cases(nx), TR.NXS.index(nx))
    assert len(cases) == len(TR.NZS) * len(TR.NYS)
    compare_with_numpy(cases)
    compare_with_chain(monkeypatch, cases)


def test_the_tables_meet_every_scalar_set_with_every_dtype_and_face_position():
    cases = [m for nx in TR.NXS for m in mixed(TR.shape_cases(nx), TR.NXS.index(nx))]
    seen = {(SCALARS.index(m.given), m.c.f[0].values.dtype.itemsize, m.c.to) for m in cases}
    assert seen == set(itertools.product(range(len(SCALARS)), (4, 8), TR.TOS))


def mid_size_cases(dtype, nx):
    return mixed(TR.mid_size_cases(dtype, nx), nx % 2)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("nx", [515, 516])
def test_mid_size(host_abi, monkeypatch, dtype, nx):
    solid, unstable = compare_with_numpy(mid_size_cases(dtype, nx), monkeypatch)
    assert unstable > 1000


# ---- 3. cases that are not hollow -----------------------------------------------------------------------------------------
def test_the_tables_are_not_hollow():
    """the reference alone, over every table the CPU and the GPU suite run: no case breaks a statement of `not_hollow`, and
    the sign statement is made often"""
    tables = [mixed(TR.shape_cases(nx), TR.NXS.index(nx)) for nx in TR.NXS]
    tables += [mixed(TR.matrix_cases(p, dt), TR.PADS3.index(p)) for p in TR.PADS3 for dt in (np.float64, np.float32)]
    tables += [mixed(TR.metric_cases(dt)) for dt in (np.float64, np.float32)] + [fuzz_cases()]
    tables += [mid_size_cases(dt, nx) for dt in (np.float64, np.float32) for nx in (515, 516)]
    solid = sum(m.not_hollow(*m.want()) for t in tables for m in t)
    assert solid >= 40, solid


def zero_over_zero_cases(dtype):
    """`extend` on Z to "outer" without a floor: both differences vanish at faces 0 and nz, so Ri is 0 / 0 there (X and Y
    periodic or `extend`: a `fill` pad puts the fill value itself beside the last derivative, which is a shear)"""
    return [Mix(TR.Case(lead, nz, 5, nx, dtype, (px, py, "extend"), "outer", metric), dict(shear_floor=0.0, **extra))
            for (lead, nz, nx, metric), (px, py), extra in zip(
                [((), 4, 6, "1d"), ((2,), 3, 132, "full"), ((), 1, 8, None), ((2,), 5, 9, "lead")],
                [("periodic", "periodic"), ("extend", "periodic"), ("extend", "extend"), ("periodic", "extend")],
                [dict(), dict(alpha=10.0), dict(nu0=1e-2), dict()])]


def check_zero_over_zero(dtype):
    for m in zero_over_zero_cases(dtype):
        (nu, kappa), (want_nu, want_kappa, ri, n2, s2) = m.one_pass(), m.want()
        nz = m.c.nz
        nan = np.zeros(want_nu.shape, bool)
        nan[..., [0, nz], :, :] = True
        assert np.array_equal(np.isnan(want_nu), nan) and np.array_equal(np.isnan(want_kappa), nan), m   # the reference
        assert (s2[..., [0, nz], :, :] == 0).all() and (n2[..., [0, nz], :, :] == 0).all()
        assert np.array_equal(np.isnan(nu.values), nan) and np.array_equal(np.isnan(kappa.values), nan), m
        _same_bits(nu.values, want_nu)
        _same_bits(kappa.values, want_kappa)
        floored = Mix(m.c, dict(m.given, shear_floor=FLOOR))          # a floor makes those faces the closure's value at Ri = 0
        fnu, fkappa = floored.one_pass()
        t = want_nu.dtype.type
        top = t(floored.s["nu0"]) + t(floored.s["nu_b"])
        assert (fnu.values[..., [0, nz], :, :] == top).all() and (fkappa.values[..., [0, nz], :, :] == top + t(floored.s["kappa_b"])).all()
        assert np.isfinite(fnu.values).all() and np.isfinite(fkappa.values).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_without_a_floor_zero_over_zero_is_nan_exactly_where_the_reference_has_it(host_abi, dtype):
    check_zero_over_zero(dtype)


def check_nan_locality(to, pads):
    """one NaN at a time in b, u or v: NaN in both results exactly where the reference has it, and never everywhere"""
    for c, which, at in TR.nan_cases(to, pads):
        m = Mix(c, SCALARS[which])
        (nu, kappa), want = m.one_pass(), m.want()
        for got, w in zip((nu, kappa), want[:2]):
            assert np.array_equal(np.isnan(got.values), np.isnan(w)), (m, which, at)
            assert np.isnan(got.values).any() and not np.isnan(got.values).all()
        assert np.array_equal(np.isnan(nu.values), np.isnan(kappa.values))


@pytest.mark.parametrize("to", TR.TOS)
@pytest.mark.parametrize("pads", [("periodic", "periodic", "periodic"), ("extend", "fill", "fill"), ("fill", "extend", "fill")],
                         ids=lambda p: "-".join(p))
def test_a_nan_poisons_exactly_what_the_chain_has_as_nan(host_abi, to, pads):
    check_nan_locality(to, pads)


def test_infinities_do_what_the_chain_does(host_abi):
    """Ri = +inf (N2 > 0 over no shear, no floor) gives the background values, Ri = -inf gives NaN, as in the reference"""
    c = TR.Case((), 3, 4, 6, np.float64, ("extend", "extend", "fill"), "left", metric=None, fill={"X": 0.0, "Y": 0.0, "Z": 0.25})
    b, u, v = c.f
    c.f = (b, u._replace(data=np.full(u.shape, 0.25)), v._replace(data=np.full(v.shape, 0.25)))
    m = Mix(c, dict())
    (nu, kappa), (want_nu, want_kappa, ri, n2, s2) = m.one_pass(), m.want()
    assert (s2 == 0).all() and np.isinf(ri).all() and (ri > 0).any() and (ri < 0).any()
    _same_bits(nu.values, want_nu)
    _same_bits(kappa.values, want_kappa)
    assert (nu.values[ri > 0] == 1e-4).all() and (kappa.values[ri > 0] == 1e-5).all()
    assert np.isnan(nu.values[ri < 0]).all() and np.isnan(kappa.values[ri < 0]).all()


# ---- 4. seeded fuzz -------------------------------------------------------------------------------------------------------
def fuzz_cases():
    return mixed(TR.fuzz_cases(seed=20241020, n=120))


def test_seeded_fuzz(host_abi, monkeypatch):
    cases = fuzz_cases()
    solid, unstable = compare_with_numpy(cases)
    assert len(cases) == 120 and solid >= 5 and unstable > 0
    compare_with_chain(monkeypatch, cases)


# ---- 5. scalars -----------------------------------------------------------------------------------------------------------
def _case(pads=("periodic", "extend", "fill"), lead=(), nz=3, ny=5, nx=6, dtype=np.float64, to="outer", metric="1d", **kw):
    return TR.Case(lead, nz, ny, nx, dtype, pads, to, metric, **kw)


def test_float32_fields_with_python_floats_stay_float32(host_abi, monkeypatch):
    calls = _counted(monkeypatch, bar_chain=True)
    m = Mix(_case(dtype=np.float32, lead=(2,)), SCALARS[1])
    nu, kappa = m.one_pass()
    assert nu.values.dtype == kappa.values.dtype == np.float32 and calls == {"fused": 1, "chain": 0}
    want = m.want()
    _same_bits(nu.values, want[0])
    _same_bits(kappa.values, want[1])


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_numpy_scalars_that_do_not_promote_are_served(host_abi, monkeypatch, dtype):
    calls = _counted(monkeypatch, bar_chain=True)
    scalars = dict(nu0=dtype(1.25e-2), alpha=np.float32(10.0), nu_b=np.float16(0.0001), kappa_b=dtype(2e-6), shear_floor=np.float32(FLOOR))
    m = Mix(_case(dtype=dtype), scalars)
    nu, kappa = m.one_pass()
    assert calls == {"fused": 1, "chain": 0} and nu.values.dtype == np.dtype(dtype)
    want = m.want()
    _same_bits(nu.values, want[0])
    _same_bits(kappa.values, want[1])


def _bar_the_entry(monkeypatch, s2_too=False):
    import xgcm_amd.device as D

    monkeypatch.setattr(D, "richardson_mixing", lambda *a, **k: pytest.fail("one-pass entry called"))
    if s2_too:
        monkeypatch.setattr(D, "richardson_number", lambda *a, **k: pytest.fail("one-pass entry called"))


@pytest.mark.parametrize("which", ["nu_b", "kappa_b", "shear_floor"])
def test_a_wider_numpy_scalar_runs_the_chain(host_abi, monkeypatch, which):
    """a numpy float64 scalar next to float32 fields promotes in the chain: the results are float64 from that step on"""
    _bar_the_entry(monkeypatch)
    c = _case(dtype=np.float32)
    kw = dict(SCALARS[1], **{which: np.float64(SCALARS[1][which])}, fill_value=TR.FILL)
    got, want = c.grid.richardson_mixing(*c.f, **kw), _chain(c.grid, *c.f, **kw, s2_written_out=False)
    for g, w in zip(got, want):
        _same_labelled(g, w)
        _same_bits(g.values, w.values)
    assert got[1].values.dtype == np.float64 and got[0].values.dtype == (np.float32 if which == "kappa_b" else np.float64)


def test_an_array_valued_scalar_runs_the_chain(host_abi, monkeypatch):
    _bar_the_entry(monkeypatch)
    c = _case(lead=(2,))
    prof = DataArray(np.linspace(1e-5, 1e-4, 4), ("ZO",), name="nu_b")
    plane = np.full((5, 6), 2e-6)
    for kw in (dict(nu_b=prof), dict(kappa_b=plane), dict(nu_b=prof, kappa_b=np.float64(1e-6)), dict(shear_floor=np.full((1,), FLOOR))):
        kw = dict(kw, fill_value=TR.FILL)
        got, want = c.grid.richardson_mixing(*c.f, **kw), _chain(c.grid, *c.f, **kw, s2_written_out=False)
        for g, w in zip(got, want):
            _same_labelled(g, w)
            _same_bits(g.values, w.values)
    nu, kappa = c.grid.richardson_mixing(*c.f, nu_b=prof, shear_floor=FLOOR, fill_value=TR.FILL)
    want = Mix(c, dict(shear_floor=FLOOR, nu_b=prof.values[:, None, None])).want()
    _same_bits(nu.values, want[0])


def test_a_scalar_that_is_no_number_raises_what_the_chain_raises(host_abi, monkeypatch):
    _bar_the_entry(monkeypatch)
    c = _case()
    for kw in (dict(alpha="5"), dict(nu0=None), dict(shear_floor=1j)):
        TR._same_error(lambda: c.grid.richardson_mixing(*c.f, **kw), lambda: _chain(c.grid, *c.f, **kw, s2_written_out=False),
                       own=AttributeError)


# ---- 6. every fallback of richardson_number's docstring takes the chain ---------------------------------------------------
def _fallback_equals_chain(grid, f, **kw):
    kw = dict(SCALARS[1], **kw)
    for got, want in zip(grid.richardson_mixing(*f, **kw), _chain(grid, *f, **kw)):
        _same_labelled(got, want)


@pytest.mark.parametrize("dtype", [np.int64, np.int32, np.float16])
def test_integer_and_half_fields_run_the_chain(backend, monkeypatch, dtype):
    _bar_the_entry(monkeypatch, s2_too=True)
    c = _case()
    f = tuple(DataArray((a.values * 100).astype(dtype), a.dims, name=a.name) for a in c.f)
    for kw in (dict(), dict(metric_weighted=False, fill_value=TR.FILL, to="left")):
        with np.errstate(all="ignore"):
            _fallback_equals_chain(c.grid, f, **kw)


def test_mixed_dtypes_run_the_chain(backend, monkeypatch):
    _bar_the_entry(monkeypatch, s2_too=True)
    grid, ds, dims = TR._grid((), 3, 5, 6, np.float32, {"X": "fill", "Y": "periodic", "Z": "extend"}, mdtype=np.float64)
    b, u, v = TR._fields((), 3, 5, 6, np.float32, dims)
    with np.errstate(all="ignore"):
        _fallback_equals_chain(grid, (b, u, v), fill_value=TR.FILL)
        _fallback_equals_chain(grid, (b, u, v._replace(data=v.values.astype(np.float64))), fill_value=TR.FILL, metric_weighted=False)


def test_a_float64_b_next_to_float32_velocities_runs_the_chain(host_abi, monkeypatch):
    _bar_the_entry(monkeypatch)
    c = _case(dtype=np.float32, metric=None)
    b = c.f[0]._replace(data=c.f[0].values.astype(np.float64))
    kw = dict(SCALARS[0], fill_value=TR.FILL, metric_weighted=False)
    for got, want in zip(c.grid.richardson_mixing(b, *c.f[1:], **kw), _chain(c.grid, b, *c.f[1:], **kw, s2_written_out=False)):
        _same_labelled(got, want)
        assert got.values.dtype == np.float64


def test_fewer_than_three_dims_or_z_elsewhere_run_the_chain(backend, monkeypatch):
    _bar_the_entry(monkeypatch, s2_too=True)
    c = _case(lead=(2,))
    b, u, v = c.f
    with np.errstate(all="ignore"):
        _fallback_equals_chain(c.grid, (b.transpose("ZC", "time", "YC", "XC"), u.transpose("ZC", "time", "YC", "XG"),
                                        v.transpose("ZC", "time", "YG", "XC")), fill_value=TR.FILL)
        _fallback_equals_chain(c.grid, (b, u.transpose("time", "YC", "ZC", "XG"), v), fill_value=TR.FILL, metric_weighted=False)
        col = lambda a, name: DataArray(np.ascontiguousarray(a.values[0, :, 0, :]), (a.dims[1], a.dims[3]), name=name)  # noqa: E731
        _fallback_equals_chain(c.grid, (col(u, "b"), col(u, "u"), col(u, "v")), y_axis="X", fill_value=TR.FILL)


def test_velocities_elsewhere_or_of_different_shapes_run_the_chain(backend, monkeypatch):
    _bar_the_entry(monkeypatch, s2_too=True)
    c = _case(lead=(2,))
    b, u, v = c.f
    with np.errstate(all="ignore"):
        _fallback_equals_chain(c.grid, (b, DataArray(u.values, b.dims, name="u"), v), fill_value=TR.FILL)
        _fallback_equals_chain(c.grid, (b, u, DataArray(v.values, b.dims, name="v")), fill_value=TR.FILL, metric_weighted=False)
        v0 = DataArray(np.ascontiguousarray(v.values[0]), v.dims[1:], name="v")   # v without the leading dim: it broadcasts
        _fallback_equals_chain(c.grid, (b, u, v0), fill_value=TR.FILL)


def test_b_elsewhere_runs_the_chain(host_abi, monkeypatch):
    """b at u's points: the squared shear is still one pass (as in the chain), the closure is the chain's"""
    _bar_the_entry(monkeypatch)
    c = _case(lead=(2,))
    b, u, v = c.f
    bu = DataArray(b.values, u.dims, name="b")
    kw = dict(SCALARS[1], metric_weighted=False)
    with np.errstate(all="ignore"):
        for got, want in zip(c.grid.richardson_mixing(bu, u, v, **kw), _chain(c.grid, bu, u, v, **kw, s2_written_out=False)):
            _same_labelled(got, want)


@pytest.mark.parametrize("to", ["right", "inner", "center", "nowhere"])
def test_other_targets_do_what_the_chain_does(backend, monkeypatch, to):
    _bar_the_entry(monkeypatch, s2_too=True)
    c = _case()
    TR._same_error(lambda: c.grid.richardson_mixing(*c.f, to=to), lambda: _chain(c.grid, *c.f, to=to), own=AttributeError)


def test_chunked_velocities_run_the_chain(backend, monkeypatch):
    from xgcm_amd.chunked import BlockArray

    _bar_the_entry(monkeypatch, s2_too=True)
    c = _case(lead=(4,), ny=6, nx=8)
    for which in (1, 2):
        f = list(c.f)
        f[which] = DataArray(BlockArray.from_array(f[which].values, ((2, 2), (3,), (6,), (8,))), f[which].dims, name=f[which].name)
        kw = dict(SCALARS[0], fill_value=TR.FILL)
        got, want = c.grid.richardson_mixing(*f, **kw), _chain(c.grid, *f, **kw)
        plain = Mix(c, SCALARS[0]).want()
        for g, w, p in zip(got, want, plain):
            assert g.dims == w.dims and g.name == w.name
            assert np.array_equal(np.asarray(g.values), np.asarray(w.values), equal_nan=True)
            assert np.array_equal(np.asarray(g.values), p, equal_nan=True)


def test_a_chunked_b_runs_the_chain(host_abi, monkeypatch):
    from xgcm_amd.chunked import BlockArray

    _bar_the_entry(monkeypatch)
    c = _case(lead=(4,), ny=6, nx=8)
    b = DataArray(BlockArray.from_array(c.f[0].values, ((2, 2), (3,), (6,), (8,))), c.f[0].dims, name="b")
    kw = dict(SCALARS[0], fill_value=TR.FILL)
    got, want = c.grid.richardson_mixing(b, *c.f[1:], **kw), _chain(c.grid, b, *c.f[1:], **kw, s2_written_out=False)
    for g, w, p in zip(got, want, Mix(c, SCALARS[0]).want()):
        assert g.dims == w.dims and g.name == w.name
        assert np.array_equal(np.asarray(g.values), np.asarray(w.values), equal_nan=True)
        assert np.array_equal(np.asarray(g.values), p, equal_nan=True)


def test_a_metric_with_an_extra_dim_runs_the_chain(backend, monkeypatch):
    from xgcm_amd import Dataset, Grid

    _bar_the_entry(monkeypatch, s2_too=True)
    c = _case()
    coords = {k: (k, np.asarray(c.ds.coords[k].values)) for k in ("XC", "XG", "YC", "YG", "ZC", "ZL", "ZO")}
    coords["time"] = ("time", np.arange(2) * 2.0)
    ds2 = Dataset({"drCo": (("ZO", "time"), R.synthetic_metric((4, 2), 66))}, coords)
    g2 = Grid(ds2, coords=TR.AXES, metrics={("Z",): ["drCo"]}, padding=dict(zip("XYZ", c.pads)), autoparse_metadata=False)
    got = g2.richardson_mixing(*c.f, fill_value=TR.FILL)
    assert "time" in got[0].dims and "time" in got[1].dims
    for g, w in zip(got, _chain(g2, *c.f, fill_value=TR.FILL)):
        _same_labelled(g, w)


def test_a_chunked_metric_runs_the_chain(backend, monkeypatch):
    from xgcm_amd import Dataset, Grid
    from xgcm_amd.chunked import BlockArray

    _bar_the_entry(monkeypatch, s2_too=True)
    c = _case(nz=4, metric="full", to="left")
    coords = {k: (k, np.asarray(c.ds.coords[k].values)) for k in ("XC", "XG", "YC", "YG", "ZC", "ZL", "ZO")}
    names = ("hWl", "hSl", "hCl")
    ds2 = Dataset({k: (c.ds[k].dims, BlockArray.from_array(np.asarray(c.ds[k].values), ((2, 2), (5,), (6,)))) for k in names}, coords)
    g2 = Grid(ds2, coords=TR.AXES, metrics={("Z",): list(names)}, padding=dict(zip("XYZ", c.pads)), autoparse_metadata=False)
    kw = dict(SCALARS[0], to="left", fill_value=TR.FILL)
    for got, want, plain in zip(g2.richardson_mixing(*c.f, **kw), _chain(g2, *c.f, **kw), Mix(c, SCALARS[0]).want()):
        assert got.dims == want.dims and got.name == want.name
        assert np.array_equal(np.asarray(got.values), np.asarray(want.values), equal_nan=True)
        assert np.array_equal(np.asarray(got.values), plain, equal_nan=True)


def test_a_missing_metric_raises_the_chains_error(backend, monkeypatch):
    _bar_the_entry(monkeypatch, s2_too=True)
    c = _case(metric=None)
    TR._same_error(lambda: c.grid.richardson_mixing(*c.f), lambda: _chain(c.grid, *c.f))


def test_a_missing_metric_is_still_served_unweighted(host_abi, monkeypatch):
    c = _case(metric=None)
    c.kw["metric_weighted"] = False
    compare_with_chain(monkeypatch, [Mix(c, SCALARS[0])])


@pytest.mark.parametrize("axis", ["X", "Y", "Z"])
def test_an_axis_without_a_boundary_raises_the_chains_error(backend, monkeypatch, axis):
    _bar_the_entry(monkeypatch, s2_too=True)
    pad = {"X": "periodic", "Y": "extend", "Z": "fill"}
    del pad[axis]
    grid, ds, dims = TR._grid((), 3, 5, 6, np.float64, pad)
    f = TR._fields((), 3, 5, 6, np.float64, dims)
    TR._same_error(lambda: grid.richardson_mixing(*f), lambda: _chain(grid, *f))


def test_a_boundary_given_with_the_call_is_served(host_abi, monkeypatch):
    calls = _counted(monkeypatch, bar_chain=True)
    grid, ds, dims = TR._grid((), 3, 5, 6, np.float64, {})
    c = _case(pads=("fill", "periodic", "extend"))
    kw = dict(SCALARS[0], padding=dict(zip("XYZ", c.pads)), fill_value=TR.FILL, to="outer")
    nu, kappa = grid.richardson_mixing(*c.f, **kw)
    want = Mix(c, SCALARS[0]).want()
    _same_bits(nu.values, want[0])
    _same_bits(kappa.values, want[1])
    assert calls == {"fused": 1, "chain": 0}


def test_fields_without_a_level_do_what_the_chain_does(backend, monkeypatch):
    _bar_the_entry(monkeypatch, s2_too=True)
    c = _case()
    f = tuple(DataArray(np.zeros((0, 5, 6)), a.dims, name=a.name) for a in c.f)
    kw = dict(fill_value=TR.FILL, metric_weighted=False, to="left")
    try:
        want = _chain(c.grid, *f, **kw)
    except Exception:
        TR._same_error(lambda: c.grid.richardson_mixing(*f, **kw), lambda: _chain(c.grid, *f, **kw), own=AttributeError)
    else:
        for g, w in zip(c.grid.richardson_mixing(*f, **kw), want):
            _same_labelled(g, w)


@pytest.mark.parametrize("conn", ["x2x", "y2y", "z2z"])
def test_connected_faces_run_the_chain(backend, monkeypatch, conn):
    from test_topology import COORDS, X_TO_X
    from xgcm_amd import Dataset, Grid

    _bar_the_entry(monkeypatch, s2_too=True)
    ds = Dataset({"drC": (("zo",), R.synthetic_metric((5,), 63))},
                 coords={"x": np.arange(4), "xl": np.arange(4) - 0.5, "y": np.arange(4), "yl": np.arange(4) - 0.5,
                         "face": np.arange(2), "zc": np.arange(4) + 0.5, "zo": np.arange(5) * 1.0})
    grid = Grid(ds, coords=dict(COORDS, Z={"center": "zc", "outer": "zo"}), metrics={("Z",): ["drC"]},
                face_connections={"x2x": X_TO_X, "y2y": TR.Y_TO_Y, "z2z": TR.Z_TO_Z}[conn],
                padding={"X": "fill", "Y": "extend", "Z": "fill"}, autoparse_metadata=False)
    f = lambda seed, dims: DataArray(R.synthetic_field((2, 4, 4, 4), seed), dims, name="f")  # noqa: E731
    b, u, v = f(81, ("face", "zc", "y", "x")), f(82, ("face", "zc", "y", "xl")), f(83, ("face", "zc", "yl", "x"))
    for mw in (True, False):
        _fallback_equals_chain(grid, (b, u, v), fill_value=TR.FILL, metric_weighted=mw)


def test_fold_grid_runs_the_chain(backend, monkeypatch):
    import warnings

    from test_topology import Nx, Ny
    from xgcm_amd import Dataset, Grid

    _bar_the_entry(monkeypatch, s2_too=True)
    ds = Dataset({"drC": (("zo",), R.synthetic_metric((3,), 63))},
                 coords={"xh": np.arange(Nx), "xl": np.arange(Nx), "yh": np.arange(Ny), "yl": np.arange(Ny),
                         "zc": np.arange(2) + 0.5, "zo": np.arange(3) * 1.0})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        grid = Grid(ds, coords={"X": {"center": "xh", "left": "xl"}, "Y": {"center": "yh", "left": "yl"},
                                "Z": {"center": "zc", "outer": "zo"}}, metrics={("Z",): ["drC"]},
                    padding={"X": "periodic", "Y": {"fold": "corner"}, "Z": "fill"}, autoparse_metadata=False)
        f = lambda seed, dims: DataArray(R.synthetic_field((2, Ny, Nx), seed), dims)  # noqa: E731
        b, u, v = f(91, ("zc", "yh", "xh")), f(92, ("zc", "yh", "xl")), f(93, ("zc", "yl", "xh"))
        for mw in (True, False):
            _fallback_equals_chain(grid, (b, u, v), metric_weighted=mw)


# ---- 7. end to end: nu and kappa into the implicit solves -----------------------------------------------------------------
def end_to_end(to, dtype, chain_kw):
    """(solves fed by the one-pass nu and kappa, solves fed by the chain's): u, v and b one implicit step further"""
    from xgcm_amd import Dataset, Grid

    nz, ny, nx = 5, 6, 8
    c = TR.Case((2,), nz, ny, nx, dtype, ("periodic", "extend", "extend"), to, "1d")
    data = {k: (c.ds[k].dims, np.asarray(c.ds[k].values)) for k in ("drCl", "drCo")}
    data["drF"] = (("ZC",), R.synthetic_metric((nz,), 65).astype(dtype))
    coords = {k: (k, np.asarray(c.ds.coords[k].values)) for k in c.ds.coords}
    grid = Grid(Dataset(data, coords), coords=TR.AXES, metrics={("Z",): list(data)}, padding=dict(zip("XYZ", c.pads)),
                autoparse_metadata=False)
    b, u, v = c.f
    kw = dict(nu0=5e3, alpha=5.0, nu_b=1e2, kappa_b=1e1, shear_floor=FLOOR, to=to)   # (large against dz^2 / dt: the solves mix)
    out = []
    for nu, kappa in (grid.richardson_mixing(b, u, v, **kw), _chain(grid, b, u, v, **kw, **chain_kw)):
        assert nu.dims == kappa.dims == ("time", TR.ZDIM[to], "YC", "XC")
        xu, xv = grid.implicit_vertical_viscosity(u, v, nu, dt=3600.0, to=to)
        xb = grid.implicit_vertical_diffusion(b, kappa, dt=3600.0, to=to)
        assert not np.array_equal(xu.values, u.values) and not np.array_equal(xb.values, b.values)
        out.append((xu, xv, xb))
    return out


@pytest.mark.parametrize("to", TR.TOS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_nu_and_kappa_feed_the_implicit_solves(host_abi, monkeypatch, to, dtype):
    calls = _counted(monkeypatch)
    one, other = end_to_end(to, dtype, dict(s2_written_out=False))
    assert calls["fused"] == 1
    for got, want in zip(one, other):
        _same_labelled(got, want)
        _same_bits(got.values, want.values)
        assert np.isfinite(got.values).all()


# ---- 8. the entry of the C ABI called directly, with views ----------------------------------------------------------------
ABI_SCALARS = (1.25e-2, 10.0, 3e-5, 2e-6, 2.0 ** -8)


def _abi_call(D, dtype, shape, fields, planes, k, offs=(ALIGNED, ALIGNED), scalars=ABI_SCALARS):
    """one call of xg_richardson_mixing: `fields` (b, u, v) views, `planes` {mu, mv, mb} views; each result is written
    `offs[n]` elements into an allocation of its own full of SENTINEL, which must still surround it afterwards"""
    (px, py, pz), to = TR.ABI_PADS[k]
    fshape = shape[:-3] + [TR._nf(shape[-3], to)] + shape[-2:]
    args = [TR.CODE[dtype]] + [f.data_ptr() for f in fields]
    for name in ("mu", "mv", "mb"):
        m = planes.get(name)
        if m is None:
            args += [None, None]
        else:
            assert all(n in (1, s) for n, s in zip(m.shape, fshape))
            args += [m.data_ptr(), _hip.i64([0 if n == 1 else m.stride(d) for d, n in enumerate(m.shape)])]
    n = int(np.prod(fshape))
    bufs = [torch.full((off + n + ALIGNED,), TR.SENTINEL, dtype=TR.TORCH[dtype], device=D._MEM.device) for off in offs]
    outs = [buf[off:off + n] for buf, off in zip(bufs, offs)]
    args += list(scalars) + [o.data_ptr() for o in outs]
    args += [_hip.i64(shape), len(shape), int(to == "outer"), _hip.BC[px], TR.FILL["X"], _hip.BC[py], TR.FILL["Y"], _hip.BC[pz],
             TR.FILL["Z"]]
    D._check(D._MEM.lib().xg_richardson_mixing(*args, D._stream()))
    res = []
    for buf, off in zip(bufs, offs):
        whole = buf.cpu().numpy()
        assert (whole[:off] == TR.SENTINEL).all() and (whole[off + n:] == TR.SENTINEL).all()
        res.append(whole[off:off + n].reshape(fshape))
    return res


def _abi_want(fv, pads, to, pv, dtype):
    s2 = TR._want(None, fv[1], fv[2], pads, to, TR.FILL, pv.get("mu"), pv.get("mv"))
    n2 = R.stencil1d("diff", fv[0], fv[0].ndim - 3, 1, 1 if to == "outer" else 0, pads[2], TR.FILL["Z"], m_out=pv.get("mb"))
    return closure(n2, s2, *ABI_SCALARS)[:2]


def abi_layout_cases(dtype):
    """Runs the direct-ABI table on whatever library `xgcm_amd.device._MEM` serves.  Every input view lives in a NaN-filled
    allocation, so a read outside it shows in the results; the contiguous, aligned control of each set of planes is compared
    with the numpy statement, every other layout with that control."""
    import xgcm_amd.device as D

    shape = [2, 5, 7, TR.ABI_NX[dtype]]
    lead, nz, ny, nx = shape
    fv = [R.synthetic_field(tuple(shape), 101 + n).astype(dtype) for n in range(3)]
    fv[2].reshape(-1)[5::17] = np.nan
    put = lambda a, st=None, off=ALIGNED: _strided(D, a, st or _contig(a.shape), off)  # noqa: E731
    same = lambda got, want: [_same_bits(g, w) for g, w in zip(got, want)]  # noqa: E731
    for k, ((px, py, pz), to) in enumerate(TR.ABI_PADS):
        nf = TR._nf(nz, to)
        forms = {"z": (1, nf, 1, 1), "p": (1, 1, ny, nx), "v3": (1, nf, ny, nx), "vl": (lead, nf, ny, nx)}
        vals = {form: R.synthetic_metric(sh, 111 + i).astype(dtype) for i, (form, sh) in enumerate(forms.items())}
        fields = [put(a) for a in fv]
        assert all(f.is_contiguous() and f.data_ptr() % 16 == 0 for f in fields)
        for present in ({"mu": "z"}, {"mv": "p"}, {"mb": "v3"}, {"mu": "v3", "mv": "vl", "mb": "z"}, {"mu": "vl", "mv": "z", "mb": "p"}, {}):
            pv = {n: vals[form] for n, form in present.items()}
            aligned = {n: put(a) for n, a in pv.items()}
            control = _abi_call(D, dtype, shape, fields, aligned, k)
            want = _abi_want(fv, (px, py, pz), to, pv, dtype)
            assert control[0].dtype == want[0].dtype == np.dtype(dtype)
            same(control, want)
            assert not np.isnan(want[0]).all() and (want[0] != want[1]).any()
            views = []
            # a misaligned base: each field in turn, then all three (the narrow form); each result misaligned, then both
            for moved in ((0,), (1,), (2,), (0, 1, 2)):
                off = [put(a, off=1) if n in moved else fields[n] for n, a in enumerate(fv)]
                assert all(off[n].data_ptr() % 16 == fv[n].dtype.itemsize for n in moved)
                views.append((off, aligned, (ALIGNED, ALIGNED)))
            views += [(fields, aligned, offs) for offs in ((1, ALIGNED), (ALIGNED, 1), (1, 1))]
            # the planes one element in; with an odd row pitch; with an odd level pitch (volumes)
            views.append((fields, {n: put(a, off=1) for n, a in pv.items()}, (ALIGNED, ALIGNED)))
            pitched = {}
            for n, a in pv.items():
                s = list(a.shape)
                pitched[n] = put(a, _contig(s[:-1] + [s[-1] + 1]) if s[-1] > 1 else _contig(s))
                assert s[-1] == 1 or (pitched[n].stride(-2) == nx + 1 and pitched[n].stride(-1) == 1)
            views.append((fields, pitched, (ALIGNED, ALIGNED)))
            for n, form in present.items():
                a = pv[n]
                if form in ("v3", "vl"):
                    st = [(nf * (ny * nx + 1)) * (a.shape[0] > 1), ny * nx + 1, nx, 1]
                    lev = put(a, [s or 1 for s in st])
                    assert lev.stride(1) == ny * nx + 1
                    views.append((fields, dict(aligned, **{n: lev}), (ALIGNED, ALIGNED)))
                if form == "z":   # the Z-only metric three elements apart
                    views.append((fields, dict(aligned, **{n: put(a, [3 * nf, 3, 1, 1], 1)}), (ALIGNED, ALIGNED)))
                if form == "p":   # the plane stored (X, Y): a transposed view
                    t = put(np.ascontiguousarray(a.transpose(0, 1, 3, 2))).permute(0, 1, 3, 2)
                    assert t.stride(-1) == ny and t.stride(-2) == 1
                    views.append((fields, dict(aligned, **{n: t}), (ALIGNED, ALIGNED)))
            for f_, planes, offs in views:
                same(_abi_call(D, dtype, shape, f_, planes, k, offs), control)
        # a stride-0 metric along X and Y: one value per face, expanded over the whole volume, equals the Z-only metric
        flat = put(vals["z"]).expand(1, nf, ny, nx)
        assert flat.stride(-1) == 0 and flat.stride(-2) == 0
        full = put(np.ascontiguousarray(np.broadcast_to(vals["z"], (1, nf, ny, nx))))
        same(_abi_call(D, dtype, shape, fields, {"mu": flat, "mv": flat, "mb": flat}, k),
             _abi_call(D, dtype, shape, fields, {"mu": full, "mv": full, "mb": full}, k))
    assert nx % TR.NVS[dtype] == 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_abi_layouts(host_abi, dtype):
    abi_layout_cases(dtype)


def abi_bad_calls():
    """bad calls return an error code, write nothing and leave the process alone; runs on whatever library `_MEM` serves"""
    import xgcm_amd.device as D

    lib = D._MEM.lib()
    shape = [2, 3, 4]
    t = torch.ones(shape, dtype=torch.float64, device=D._MEM.device)
    outs = [torch.full([3, 3, 4], TR.SENTINEL, dtype=torch.float64, device=D._MEM.device) for _ in range(2)]   # room for Z:outer
    P = lambda x: None if x is None else x.data_ptr()  # noqa: E731

    def call(code=TR.CODE[np.float64], b=t, u=t, v=t, o=outs, shape=shape, ndim=3, outer=0, bcx=_hip.BC["periodic"],
             bcy=_hip.BC["extend"], bcz=_hip.BC["fill"], mu=None, mus=None):
        return lib.xg_richardson_mixing(code, P(b), P(u), P(v), mu, mus, None, None, None, None, *ABI_SCALARS, P(o[0]), P(o[1]),
                                        None if shape is None else _hip.i64(shape), ndim, outer, bcx, 0.0, bcy, 0.0, bcz, 0.0,
                                        D._stream())

    untouched = lambda: all(bool((o == TR.SENTINEL).all()) for o in outs)  # noqa: E731
    for code in (-1, _hip.DTYPE["float16"], _hip.DTYPE["int64"], _hip.DTYPE["int32"], 12, 99):
        assert call(code=code) == -1                              # any other element type: XG_ERR_INVALID
    assert call(b=None) == -1 and call(u=None) == -1 and call(v=None) == -1 and call(shape=None) == -1   # NULL arguments (b too)
    assert call(o=[None, outs[1]]) == -1 and call(o=[outs[0], None]) == -1                                # a NULL result
    assert call(bcx=7) == -1 and call(bcy=-1) == -1 and call(bcz=9) == -1     # unknown boundary codes
    assert call(outer=2) == -1 and call(outer=-1) == -1           # unknown face position
    assert call(shape=[0, 3, 4]) == -1                            # nz = 0: no level to pad from
    assert call(mu=t.data_ptr(), mus=None) == -1                  # a metric without strides
    assert call(ndim=2) < 0 and call(ndim=2) != -1                # XG_ERR_UNSUPPORTED
    assert untouched()
    assert call(shape=[2, 0, 4]) == 0 and call(shape=[2, 3, 0]) == 0 and untouched()   # an empty plane: nothing to do
    assert call() == 0 and call(bcz=_hip.BC["periodic"], outer=1) == 0 and call(bcz=_hip.BC["extend"], outer=1) == 0
    assert not untouched()


def test_abi_refuses_bad_calls(host_abi):
    abi_bad_calls()


# ---- 9. the tunable call table, between guard bands -----------------------------------------------------------------------
def tunable_calls(D, dtype):
    """(calls, references) of the K7p tunable sweep: name -> thunk that calls `D` on inputs uploaded once, name -> thunk that
    gives numpy's pair of results of the same call.  The battery's own shapes, both face positions, a profile and three
    volumes as the metrics, the scalar sets in turn"""
    f = lambda shape, seed: R.synthetic_field(shape, seed).astype(dtype)  # noqa: E731
    m = lambda shape, seed: R.synthetic_metric(shape, seed).astype(dtype)  # noqa: E731
    calls, references = {}, {}
    for n, shape in enumerate(((5, 300, 264), (3, 65, 131))):
        nz, ny, nx = shape
        b, u, v = (f(shape, 150 + 3 * n + k) for k in range(3))
        u[1, 7, 9] = v[0, 0, 0] = b[nz - 1, ny - 1, nx - 1] = np.nan
        dev = tuple(D.asdevice(x) for x in (b, u, v))
        for k, (to, pads) in enumerate((("left", ("periodic", "extend", "fill")), ("outer", ("extend", "fill", "periodic")),
                                        ("left", ("fill", "periodic", "extend")), ("outer", ("periodic", "periodic", "fill")))):
            nf = nz + (to == "outer")
            mets = [m((nf, 1, 1), 170)] * 3 if k % 2 else [m((nf, ny, nx), 171 + j) for j in range(3)]
            if k == 2:
                mets = [None, None, None]
            dm = tuple(None if x is None else D.asdevice(x) for x in mets)
            s = dict(DEFAULTS, **SCALARS[k])
            sc = tuple(float(s[name]) for name in ("nu0", "alpha", "nu_b", "kappa_b", "shear_floor"))
            key = f"{nx}{to}{pads[2]}"
            fill = [TR.FILL[a] for a in "XYZ"]
            calls[key] = lambda dev=dev, dm=dm, sc=sc, to=to, pads=pads: D.richardson_mixing(*dev, *dm, *sc, to == "outer", *pads, *fill)

            def reference(h=(b, u, v), mets=mets, sc=sc, to=to, pads=pads):
                s2 = TR._want(None, h[1], h[2], pads, to, TR.FILL, *mets[:2])
                n2 = R.stencil1d("diff", h[0], 0, 1, 1 if to == "outer" else 0, pads[2], TR.FILL["Z"], m_out=mets[2])
                return list(closure(n2, s2, *sc)[:2])

            references[key] = reference
    return calls, references


def _bits_equal(got, want):
    try:
        _same_bits(got, want)
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_the_tunable_call_table_equals_its_numpy_references(host_abi, dtype):
    """the thunks the GPU suite sweeps over every tunable value, once through the host build (which reads no tunable): the
    arguments, their order, the shapes and the references are checked before any GPU time is spent on them"""
    import xgcm_amd.device as D

    calls, references = tunable_calls(D, dtype)
    assert len(calls) == 8 and set(calls) == set(references)
    for name, thunk in calls.items():
        got, want = [D.tohost(x) for x in thunk()], references[name]()
        assert len(got) == len(want) == 2, name
        for g, w in zip(got, want):
            assert g.dtype == np.dtype(dtype) and np.isnan(w).any() and np.isnan(w).mean() < 0.01, name
            assert _bits_equal(g, w), name
        assert (want[0] != want[1]).any()


def guarded_table(D, monkeypatch, dtype, offset, same_bits):
    """the table built and run between guard bands: a store outside either result, a cell left unwritten and a
    result-changing read outside a field or a metric all fail; returns the number of results checked"""
    checked = 0
    with GM.guarded(D, monkeypatch, offset) as g:
        calls, references = tunable_calls(D, dtype)
        assert g.placed >= 2 * 3 + 2 * 4          # the fields of both shapes, the metrics of the calls that have them
        for k, fn in calls.items():
            before = g.handed_out
            got = [D.tohost(x) for x in fn()]
            g.check(f"{k} at offset {offset}")
            assert g.handed_out - before >= 2     # both results between guards
            for x, want in zip(got, references[k]()):
                assert same_bits(x, want), f"{k} at offset {offset}: not numpy's result"
                checked += 1
    return checked


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_between_guard_bands_through_the_host_abi(host_abi, monkeypatch, dtype):
    import xgcm_amd.device as D

    for offset in (0, np.dtype(dtype).itemsize):
        assert guarded_table(D, monkeypatch, dtype, offset, _bits_equal) == 16
