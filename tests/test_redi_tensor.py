"""The tapered Redi / Gent-McWilliams tensor column at the faces of Z, `Grid.redi_tensor`, on CPU.

The one-pass path runs through the `host_abi` fixture (the product's `xgcm_amd.device` over libxgcm_host.so); the chain it
replaces

    sx, sy = grid.isopycnal_slope(b, ...)                                     (here: its own chain, tests/test_isopycnal_slope.py)
    s2 = sx * sx + sy * sy
    kt = kappa                      if slope_max is None else
         kappa * (m2 / den)         with m2 = slope_max * slope_max, ex = s2 - m2, den = m2 + (ex + abs(ex)) * 0.5
    kwx, kwy, kwz = kt * sx, kt * sy, kt * s2

runs through the same Grid over the oracle double, installed AFTER the one-pass calls of a test have run.  `_tensor` states the
epilogue a third time, over plain numpy arrays with `R.binary`, on top of `TI._want`.  Every comparison is bit for bit (NaN
where the other has NaN, -0.0 is not +0.0), with dims, coords and names where labels are compared.  The one-pass device entry
is counted and the chain's device functions (`isopycnal_slope`'s entry among them) are barred wherever a case must not pass by
falling back.  The case builders, grids and fields are those of tests/test_isopycnal_slope.py, by import; every table runs
tapered (slope_max = 0.75, m2 = 0.5625 exactly) and untapered (slope_max = None).

Asserted on the REFERENCE alone: `TI.Case.not_hollow` (sx and sy finite on every interior face of the cases it names), and,
over those cases of a test taken together, that at least a fifth of the finite interior faces have s2 <= m2 and at least a
fifth s2 > m2 (`Tally.balanced`): both branches of the taper are met in every test.  Properties, first on the statement and
then on the operator: where s2 <= m2 the tapered results carry the bits of the untapered ones; where s2 > m2 and finite,
kwz <= kappa * m2 * (1 + 4 eps) -- den = m2 + (s2 - m2) is two roundings from s2, the quotient adds one, each of the two
products one."""

import numpy as np
import pytest
import torch

import guarded_memory as GM
import test_isopycnal_slope as TI
import test_richardson_number as TR
from oracle import refimpl as R
from test_fused_layouts import ALIGNED, _contig, _strided
from xgcm_amd import DataArray, _hip
from xgcm_amd.chunked import BlockArray

FILL, ZDIM, PADS3 = TI.FILL, TI.ZDIM, TI.PADS3
SMAX, M2 = 0.75, 0.5625
KAPPAS = (1000.0, 2.5, 3)        # (exact in float32; the int is a weak scalar too)
_same_labelled, _same_bits, _same_error = TR._same_labelled, TR._same_bits, TR._same_error


def _tensor(sx, sy, kappa, slope_max):
    """the numpy statement of the epilogue, one `R.binary` per operation of the chain"""
    B = R.binary
    with np.errstate(all="ignore"):
        s2 = B("add", B("mul", sx, sx), B("mul", sy, sy))
        if slope_max is None:
            kt = kappa
        else:
            m2 = float(slope_max) * float(slope_max)
            ex = B("sub", s2, m2)
            den = B("add", m2, B("mul", B("add", ex, np.abs(ex)), 0.5))
            kt = B("mul", kappa, B("div", m2, den))
        out = B("mul", kt, sx), B("mul", kt, sy), B("mul", kt, s2)
    assert all(o.dtype == sx.dtype for o in out)
    return out


def _chain(grid, b, kappa=1000.0, slope_max=1e-2, x_axis="X", y_axis="Y", z_axis="Z", to=None, padding=None, fill_value=None,
           metric_weighted=True):
    """the specification, the slopes as `isopycnal_slope`'s own chain"""
    sx, sy = TI._chain(grid, b, x_axis, y_axis, z_axis, to=to, padding=padding, fill_value=fill_value, metric_weighted=metric_weighted)
    s2 = sx * sx + sy * sy
    if slope_max is None:
        kt = kappa
    else:
        m2 = float(slope_max) * float(slope_max)
        ex = s2 - m2
        den = m2 + (ex + abs(ex)) * 0.5
        kt = kappa * (m2 / den)
    return kt * sx, kt * sy, kt * s2


class Case:
    """one call of the operator: a case of tests/test_isopycnal_slope.py, kappa and slope_max"""

    def __init__(self, base, slope_max, kappa=1000.0):
        self.base, self.slope_max, self.kappa = base, slope_max, kappa
        self.dims, self.to, self.nz, self.pads = base.dims, base.to, base.nz, base.pads

    def __repr__(self):
        return f"{self.base} kappa {self.kappa!r} slope_max {self.slope_max!r}"

    def one_pass(self):
        return self.base.grid.redi_tensor(self.base.b, self.kappa, self.slope_max, **self.base.kw)

    def chain(self):
        return _chain(self.base.grid, self.base.b, self.kappa, self.slope_max, **self.base.kw)

    def slopes(self):
        return self.base.want()

    def want(self, slopes=None):
        return _tensor(*(slopes or self.slopes()), self.kappa, self.slope_max)


def both(bases):
    """every case of a table of tests/test_isopycnal_slope.py tapered and untapered, kappa rotating"""
    return [Case(c, sm, KAPPAS[(n + k) % 3]) for n, c in enumerate(bases) for k, sm in enumerate((SMAX, None))]


class Tally:
    """the finite interior faces of the not-hollow cases of a test: how many lie below the limit and how many above it"""

    def __init__(self):
        self.solid = self.below = self.above = 0

    def add(self, c, sx, sy):
        if not c.base.not_hollow(sx, sy):
            return
        self.solid += 1
        with np.errstate(all="ignore"):
            s2 = (sx * sx + sy * sy)[..., 1:c.nz, :, :]
        s2 = s2[np.isfinite(s2)]
        self.below += int((s2 <= M2).sum())
        self.above += int((s2 > M2).sum())

    def balanced(self):
        n = self.below + self.above
        assert n > 0 and 5 * self.below >= n and 5 * self.above >= n, (self.below, self.above)
        return self.solid


def check_properties(c, slopes, got):
    """the two consequences of the docstring on the three results `got` of a tapered case, numpy arrays"""
    if c.slope_max is None:
        return
    sx, sy = slopes
    with np.errstate(all="ignore"):
        s2 = sx * sx + sy * sy
        free = _tensor(sx, sy, c.kappa, None)
    m2 = np.asarray(float(c.slope_max) ** 2, sx.dtype)
    low = s2 <= m2
    for g, f in zip(got, free):
        _same_bits(g[low], f[low])      # exactly the untapered bits
    high = (s2 > m2) & np.isfinite(s2)
    bound = float(c.kappa) * float(m2) * (1 + 4 * float(np.finfo(sx.dtype).eps))
    assert (got[2][high].astype(np.float64) <= bound).all(), c


def _counted(monkeypatch, bar_chain=True):
    """the calls of the one-pass device entry; `bar_chain`: and those of the chain's own device functions"""
    import xgcm_amd.device as D

    calls = {"fused": 0, "chain": 0}

    def counted(fn, key):
        def wrapped(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(D, "redi_tensor", counted(D.redi_tensor, "fused"))
    if bar_chain:
        for name in ("binary", "stencil1d", "isopycnal_slope"):
            monkeypatch.setattr(D, name, counted(getattr(D, name), "chain"))
    return calls


def compare_with_numpy(cases, monkeypatch=None):
    """the three results of every case against the numpy statement, bit for bit; the statement is first held to `not_hollow`
    and to the two properties, then the operator to the properties; on whatever library `_MEM` serves.  With `monkeypatch`:
    exactly one call of the one-pass entry per case and none of the chain's.  Returns the number of not-hollow cases, after
    `Tally.balanced` has made its statement over them"""
    calls = _counted(monkeypatch) if monkeypatch is not None else None
    tally = Tally()
    for c in cases:
        slopes = c.slopes()
        want = c.want(slopes)
        tally.add(c, *slopes)
        check_properties(c, slopes, want)
        got = c.one_pass()
        try:
            assert len(got) == 3
            for g, w in zip(got, want):
                _same_bits(g.values, w)
                assert g.dims == c.dims + (ZDIM[c.to], "YC", "XC")
            check_properties(c, slopes, [g.values for g in got])
        except AssertionError as err:
            raise AssertionError(f"case {c}") from err
    if calls is not None:
        assert calls == {"fused": len(cases), "chain": 0}
    return tally.balanced()


def compare_with_chain(monkeypatch, cases):
    """every one-pass call first (counted, the chain barred), then the chain over the oracle double: values, dims, coords, names"""
    from oracle import fake_device

    calls = _counted(monkeypatch)
    got = [c.one_pass() for c in cases]
    assert calls == {"fused": len(cases), "chain": 0}
    fake_device.install(monkeypatch)
    for c, triple in zip(cases, got):
        with np.errstate(all="ignore"):
            want = c.chain()
        try:
            assert len(triple) == len(want) == 3
            for g, w in zip(triple, want):
                _same_labelled(g, w)
                _same_bits(g.values, w.values)
        except AssertionError as err:
            raise AssertionError(f"case {c}") from err


# ---- 1. small shapes -------------------------------------------------------------------------------------------------------
def shape_cases():
    """the small shapes of tests/test_isopycnal_slope.py over NZS x NYS x NXS as ONE table: with one column a single case of
    four interior faces is not hollow, and no field seed puts those on both sides of the limit, so the statement about the
    limit is made over the whole table"""
    return [c for nx in TI.NXS for c in both(TI.shape_cases(nx))]


def test_small_shapes(host_abi, monkeypatch):
    cases = shape_cases()
    assert len(cases) == 2 * len(TI.NZS) * len(TI.NYS) * len(TI.NXS)
    compare_with_numpy(cases)
    compare_with_chain(monkeypatch, cases)


# ---- 2. every boundary triple, metric forms, mid size ----------------------------------------------------------------------
def matrix_cases(pads, dtype):
    return both(TI.matrix_cases(pads, dtype))


@pytest.mark.parametrize("px,py,pz", PADS3)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_every_boundary_triple(host_abi, monkeypatch, px, py, pz, dtype):
    cases = matrix_cases((px, py, pz), dtype)
    assert compare_with_numpy(cases) >= 2
    compare_with_chain(monkeypatch, cases)


def metric_cases(dtype):
    return both(TI.metric_cases(dtype))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_metric_forms_and_leading_dims(host_abi, monkeypatch, dtype):
    cases = metric_cases(dtype)
    assert compare_with_numpy(cases) > 10
    compare_with_chain(monkeypatch, cases)


def mid_size_cases(dtype, nx):
    return both(TI.mid_size_cases(dtype, nx))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("nx", [515, 516])
def test_mid_size(host_abi, monkeypatch, dtype, nx):
    assert compare_with_numpy(mid_size_cases(dtype, nx), monkeypatch) == 4


# ---- 3. fills, NaNs, zero over zero -----------------------------------------------------------------------------------------
def fill_cases(dtype):
    return both(TI.fill_cases(dtype))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_fills_keep_their_bits(host_abi, monkeypatch, dtype):
    cases = fill_cases(dtype)
    assert compare_with_numpy(cases, monkeypatch) == 16
    for c in cases:
        if c.base.zero and c.slope_max is not None:   # 0 / 0 or x / 0 on every interior face: NaN under the taper (0 * inf)
            assert all(np.isnan(w[..., 1:c.nz, :, :]).all() for w in c.want()), c


def check_nan_locality(to, pads, slope_max):
    """one NaN at a time in b: NaN in the results exactly where the statement has it; in the middle of the volume kwx and kwy
    are NaN wherever sx OR sy is (the taper reads both), kwz likewise: columns i-1 .. i+1 of row j and rows j-1 .. j+1 of
    column i at faces k and k + 1"""
    for at in TI.NAN_AT:
        c = Case(TI.Case((), 5, 6, 8, np.float64, pads, to, "planes"), slope_max)
        c.base.b.values[at] = np.nan
        got, want = c.one_pass(), c.want()
        for g, w in zip(got, want):
            assert np.array_equal(np.isnan(g.values), np.isnan(w)), (c, at)
            assert np.isnan(g.values).any() and not np.isnan(g.values).all()
        if at == TI.NAN_AT[-1]:
            k, j, i = at
            mx_, my_ = np.zeros(got[0].shape, bool), np.zeros(got[0].shape, bool)
            mx_[k:k + 2, j, i - 1:i + 2] = True
            my_[k:k + 2, j - 1:j + 2, i] = True
            masks = (mx_, my_, mx_ | my_) if slope_max is None else (mx_ | my_,) * 3
            clean = Case(TI.Case((), 5, 6, 8, np.float64, pads, to, "planes"), slope_max).want()   # (0 * inf at the outermost faces)
            for g, m, w0 in zip(got, masks, clean):
                assert np.array_equal(np.isnan(g.values), m | np.isnan(w0)), (c, at)


@pytest.mark.parametrize("slope_max", [SMAX, None])
@pytest.mark.parametrize("to", TI.TOS)
@pytest.mark.parametrize("pads", [("periodic", "periodic", "periodic"), ("extend", "fill", "fill"), ("fill", "extend", "extend")],
                         ids=lambda p: "-".join(p))
def test_a_nan_poisons_exactly_what_the_statement_has_as_nan(host_abi, to, pads, slope_max):
    check_nan_locality(to, pads, slope_max)


def check_infinite_slopes(dtype):
    """`extend` on Z to "outer": bz is exactly 0 at faces 0 and nz, the slopes x / 0 or 0 / 0 there.  Tapered, an infinite
    slope gives taper 0 and 0 * inf: NaN in all three results; untapered the infinities stand.  Every interior face is finite"""
    seen = set()
    for base in TI.zero_over_zero_cases(dtype):
        for c in (Case(base, SMAX), Case(base, None)):
            got, want = c.one_pass(), c.want()
            nz = c.nz
            for g, w in zip(got, want):
                outer = w[..., [0, nz], :, :]
                assert not np.isfinite(outer).any() and np.isfinite(w[..., 1:nz, :, :]).all(), c     # the reference
                if c.slope_max is not None:
                    assert np.isnan(outer).all(), c
                else:
                    seen |= {"inf"} if np.isinf(outer).any() else set()
                _same_bits(g.values, w)
    assert "inf" in seen


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_an_infinite_slope_is_nan_under_the_taper(host_abi, dtype):
    check_infinite_slopes(dtype)


def check_identity_and_bound():
    """the two properties on fields made for them: slopes scaled so that every interior face lies below the limit (tapered ==
    untapered, bit for bit, everywhere finite), and slopes so steep that every interior face lies far above it"""
    for dtype in (np.float64, np.float32):
        eps = float(np.finfo(dtype).eps)
        for scale, below in ((1e-3, True), (1e3, False)):
            base = TI.Case((2,), 5, 9, 136, dtype, ("periodic", "extend", "fill"), "left", None)
            v = base.b.values
            # a steady stratification along Z (bz = 4 on every interior face) under one horizontal pattern, which is scaled
            base.b = base.b._replace(data=(v[:, :1] * dtype(scale) + np.arange(5, dtype=dtype)[:, None, None] * dtype(4)).astype(dtype))
            t, u = Case(base, SMAX, 1000.0), Case(base, None, 1000.0)
            sx, sy = t.slopes()
            s2 = (sx * sx + sy * sy)[:, 1:]
            assert np.isfinite(s2).all() and ((s2 <= M2).all() if below else (s2 > M2).mean() > 0.9), (dtype, scale)
            got_t, got_u = [g.values for g in t.one_pass()], [g.values for g in u.one_pass()]
            for g, w in zip(got_t, t.want()):
                _same_bits(g, w)
            check_properties(t, (sx, sy), got_t)
            if below:
                for a, b_ in zip(got_t, got_u):
                    _same_bits(a[:, 1:], b_[:, 1:])
            else:
                high = (s2 > M2)
                assert (got_t[2][:, 1:][high] <= 1000.0 * M2 * (1 + 4 * eps)).all()
                assert (got_t[2][:, 1:][high] >= 1000.0 * M2 * (1 - 4 * eps)).all()   # near kappa m2, not merely under it


def test_the_identity_below_the_limit_and_the_bound_above_it(host_abi):
    check_identity_and_bound()


# ---- 4. labels, residency, defaults ----------------------------------------------------------------------------------------
def label_cases():
    return both(TI.label_cases())


def test_coords_and_names_follow_the_chain(host_abi, monkeypatch):
    compare_with_chain(monkeypatch, label_cases())


def test_xarray_in_xarray_out(host_abi, monkeypatch):
    import xarray_standin
    from oracle import fake_device

    xarray_standin.install(monkeypatch)
    import xarray as xr

    c = Case(TI.Case((), 3, 4, 6, np.float64, ("periodic", "fill", "extend"), "left"), SMAX)
    got = c.base.grid.redi_tensor(xr.DataArray(c.base.b.values, dims=c.base.b.dims, name=c.base.b.name), c.kappa, SMAX, **c.base.kw)
    assert len(got) == 3 and all(type(g).__module__.split(".")[0] == "xarray" for g in got)
    fake_device.install(monkeypatch)
    with np.errstate(all="ignore"):
        want = c.chain()
    for g, w in zip(got, want):
        assert tuple(g.dims) == tuple(w.dims) and g.name == w.name
        _same_bits(np.asarray(g.values), np.asarray(w.values))


def test_the_defaults_are_kappa_1000_and_slope_max_1e_2(host_abi, monkeypatch):
    calls = _counted(monkeypatch)
    base = TI.Case((), 3, 4, 6, np.float64, ("periodic", "fill", "extend"), "outer")
    got = base.grid.redi_tensor(base.b, fill_value=FILL)
    assert calls == {"fused": 1, "chain": 0} and got[0].dims == ("ZO", "YC", "XC") and isinstance(got[0].data, np.ndarray)
    for g, w in zip(got, _tensor(*base.want(), 1000.0, 1e-2)):
        _same_bits(g.values, w)
    got = base.grid.redi_tensor(base.b, np.float32(4.0), np.float64(0.5), fill_value=FILL)    # numpy scalars that do not promote
    assert calls == {"fused": 2, "chain": 0}
    for g, w in zip(got, _tensor(*base.want(), 4.0, 0.5)):
        _same_bits(g.values, w)


# ---- 5. seeded fuzz ---------------------------------------------------------------------------------------------------------
def fuzz_cases():
    """the 120 cases of tests/test_isopycnal_slope.py, tapered and untapered in turns"""
    return [Case(c, (SMAX, None)[n % 2], KAPPAS[n % 3]) for n, c in enumerate(TI.fuzz_cases())]


def test_seeded_fuzz(host_abi, monkeypatch):
    cases = fuzz_cases()
    assert len(cases) == 120 and compare_with_numpy(cases) >= 10
    compare_with_chain(monkeypatch, cases)


def test_the_tables_meet_both_sides_of_the_limit():
    """the reference alone, over every table the CPU and the GPU suite run, table by table as the tests take them: the
    not-hollow cases of each have at least a fifth of their finite interior faces on either side of m2"""
    tables = [shape_cases()] + [matrix_cases(p, dt) for p in PADS3 for dt in (np.float64, np.float32)]
    tables += [t(dt) for t in (metric_cases, fill_cases) for dt in (np.float64, np.float32)] + [fuzz_cases()]
    tables += [mid_size_cases(dt, nx) for dt in (np.float64, np.float32) for nx in (515, 516)]
    for table in tables:
        tally = Tally()
        for c in table:
            tally.add(c, *c.slopes())
        assert tally.balanced() >= 2, table[0]


# ---- 6. every fallback of the docstring takes the chain ---------------------------------------------------------------------
def _no_fused(monkeypatch):
    import xgcm_amd.device as D

    monkeypatch.setattr(D, "redi_tensor", lambda *a, **k: pytest.fail("one-pass entry called"))


def _fallback_equals_chain(grid, b, *scalars, **kw):
    with np.errstate(all="ignore"):
        got, want = grid.redi_tensor(b, *scalars, **kw), _chain(grid, b, *scalars, **kw)
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        _same_labelled(g, w)


def _case(pads=("periodic", "extend", "fill"), lead=(), nz=3, ny=5, nx=6, dtype=np.float64, to="outer", metric="planes", **kw):
    return TI.Case(lead, nz, ny, nx, dtype, pads, to, metric, **kw)


def test_an_array_kappa_runs_the_chain(host_abi, monkeypatch):
    _no_fused(monkeypatch)
    c = _case(lead=(2,))
    profile = DataArray(np.linspace(500.0, 1500.0, 4), ("ZO",), name="kappa")
    for sm in (SMAX, None):
        _fallback_equals_chain(c.grid, c.b, profile, sm, fill_value=FILL)
    _fallback_equals_chain(c.grid, c.b, np.full((2, 4, 5, 6), 7.0), SMAX, fill_value=FILL)


def test_a_wider_numpy_scalar_runs_the_chain(host_abi, monkeypatch):
    _no_fused(monkeypatch)
    c = _case(dtype=np.float32)
    _fallback_equals_chain(c.grid, c.b, np.float64(1000.0), SMAX, fill_value=FILL)      # promotes the float32 fields
    _fallback_equals_chain(c.grid, c.b, 1000.0, np.float64(SMAX), fill_value=FILL)      # (float() of it: the same values)
    with np.errstate(all="ignore"):
        wide = c.grid.redi_tensor(c.b, np.float64(1000.0), SMAX, fill_value=FILL)
    assert all(np.asarray(w.values).dtype == np.float64 for w in wide)


@pytest.mark.parametrize("dtype", [np.int64, np.int32, np.float16])
def test_integer_and_half_fields_run_the_chain(backend, monkeypatch, dtype):
    _no_fused(monkeypatch)
    c = _case()
    b = DataArray((c.b.values * 100).astype(dtype), c.b.dims, name="b")
    _fallback_equals_chain(c.grid, b)
    _fallback_equals_chain(c.grid, b, 2.5, None, metric_weighted=False, fill_value=FILL, to="left")


def test_a_chunked_b_runs_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    c = _case(lead=(4,), ny=6, nx=8)
    b = DataArray(BlockArray.from_array(c.b.values, ((2, 2), (3,), (6,), (8,))), c.b.dims, name="b")
    with np.errstate(all="ignore"):
        got, want = c.grid.redi_tensor(b, 1000.0, SMAX, fill_value=FILL), _chain(c.grid, b, 1000.0, SMAX, fill_value=FILL)
    for g, w, p in zip(got, want, _tensor(*c.want(), 1000.0, SMAX)):
        assert g.dims == w.dims and g.name == w.name
        assert np.array_equal(np.asarray(g.values), np.asarray(w.values), equal_nan=True)
        assert np.array_equal(np.asarray(g.values), p, equal_nan=True)


def test_b_elsewhere_or_z_elsewhere_runs_the_chain(backend, monkeypatch):
    _no_fused(monkeypatch)
    c = _case(lead=(2,))
    for dims in (("time", "ZC", "YC", "XG"), ("time", "ZC", "YG", "XC")):
        _fallback_equals_chain(c.grid, DataArray(c.b.values, dims, name="b"), 1000.0, SMAX, fill_value=FILL, metric_weighted=False)
    _fallback_equals_chain(c.grid, c.b.transpose("ZC", "time", "YC", "XC"), 1000.0, SMAX, fill_value=FILL)
    _fallback_equals_chain(c.grid, c.b.transpose("time", "YC", "ZC", "XC"), 2.5, None, fill_value=FILL, metric_weighted=False)


@pytest.mark.parametrize("conn", ["x2x", "y2y", "z2z"])
def test_connected_faces_run_the_chain(backend, monkeypatch, conn):
    from test_topology import COORDS, X_TO_X
    from xgcm_amd import Dataset, Grid

    _no_fused(monkeypatch)
    ds = Dataset({"drC": (("zo",), R.synthetic_metric((5,), 63)), "dxC": (("y", "xl"), R.synthetic_metric((4, 4), 61)),
                  "dyC": (("yl", "x"), R.synthetic_metric((4, 4), 62))},
                 coords={"x": np.arange(4), "xl": np.arange(4) - 0.5, "y": np.arange(4), "yl": np.arange(4) - 0.5,
                         "face": np.arange(2), "zc": np.arange(4) + 0.5, "zo": np.arange(5) * 1.0})
    grid = Grid(ds, coords=dict(COORDS, Z={"center": "zc", "outer": "zo"}), metrics={("X",): ["dxC"], ("Y",): ["dyC"], ("Z",): ["drC"]},
                face_connections={"x2x": X_TO_X, "y2y": TR.Y_TO_Y, "z2z": TR.Z_TO_Z}[conn],
                padding={"X": "fill", "Y": "extend", "Z": "fill"}, autoparse_metadata=False)
    b = DataArray(R.synthetic_field((2, 4, 4, 4), 81), ("face", "zc", "y", "x"), name="f")
    for mw in (True, False):
        _fallback_equals_chain(grid, b, 1000.0, SMAX, fill_value=FILL, metric_weighted=mw)


def test_a_missing_boundary_along_z_raises_the_chains_error(backend, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, dims = TI._grid((), 3, 5, 6, np.float64, {"X": "periodic", "Y": "extend"})
    b = TI._field((), 3, 5, 6, np.float64, dims)
    _same_error(lambda: grid.redi_tensor(b, 1000.0, SMAX), lambda: _chain(grid, b, 1000.0, SMAX))


def test_scalars_are_not_validated(host_abi, monkeypatch):
    """a slope_max that float() refuses raises what the chain raises; a negative kappa and slope_max = 0 are served"""
    _no_fused(monkeypatch)
    c = _case()
    _same_error(lambda: c.grid.redi_tensor(c.b, 1000.0, "steep", fill_value=FILL), lambda: _chain(c.grid, c.b, 1000.0, "steep", fill_value=FILL),
                own=AttributeError)


def test_isopycnal_slope_is_what_it_was(host_abi, monkeypatch):
    """the slopes' own operator, which shares its plan with this one: still one call of its own entry, none of the tensor's"""
    _no_fused(monkeypatch)
    TI.compare_with_numpy(TI.metric_cases(np.float64), monkeypatch)


# ---- 7. the entry of the C ABI called directly, with views ------------------------------------------------------------------
ABI_TENSOR = [(1000.0, M2, 1), (2.5, 0.0, 0)]   # (kappa, slope_max2, taper) by the parity of the table's row


def _abi_call(D, dtype, shape, b, planes, k, offs=(ALIGNED, ALIGNED, ALIGNED)):
    """one call of xg_redi_tensor: `b` a view, `planes` {mx, my, mz} views; each result is written `offs[n]` elements into an
    allocation of its own full of SENTINEL, which must still surround it afterwards"""
    (px, py, pz), to = TR.ABI_PADS[k]
    kappa, m2, taper = ABI_TENSOR[k % 2]
    fshape = shape[:-3] + [TR._nf(shape[-3], to)] + shape[-2:]
    args = [TR.CODE[dtype], b.data_ptr()]
    for name, against in (("mx", shape), ("my", shape), ("mz", fshape)):
        m = planes.get(name)
        if m is None:
            args += [None, None]
        else:
            assert all(n in (1, s) for n, s in zip(m.shape, against))
            args += [m.data_ptr(), _hip.i64([0 if n == 1 else m.stride(d) for d, n in enumerate(m.shape)])]
    args += [kappa, m2, taper]
    n = int(np.prod(fshape))
    bufs = [torch.full((off + n + ALIGNED,), TR.SENTINEL, dtype=TR.TORCH[dtype], device=D._MEM.device) for off in offs]
    args += [buf[off:off + n].data_ptr() for buf, off in zip(bufs, offs)]
    args += [_hip.i64(shape), len(shape), int(to == "outer"), _hip.BC[px], FILL["X"], _hip.BC[py], FILL["Y"], _hip.BC[pz], FILL["Z"]]
    D._check(D._MEM.lib().xg_redi_tensor(*args, D._stream()))
    res = []
    for buf, off in zip(bufs, offs):
        whole = buf.cpu().numpy()
        assert (whole[:off] == TR.SENTINEL).all() and (whole[off + n:] == TR.SENTINEL).all()
        res.append(whole[off:off + n].reshape(fshape))
    return res


def abi_layout_cases(dtype):
    """Runs the direct-ABI table on whatever library `xgcm_amd.device._MEM` serves.  Every input view lives in a NaN-filled
    allocation, so a read outside it shows in the results; the contiguous, aligned control of each set of planes is compared
    with the numpy statement, every other layout with that control.  Result offsets: 0, 16 bytes and one element."""
    import xgcm_amd.device as D

    shape = [2, 5, 7, TR.ABI_NX[dtype]]
    lead, nz, ny, nx = shape
    bv = R.synthetic_field(tuple(shape), 101).astype(dtype)
    bv.reshape(-1)[5::97] = np.nan
    put = lambda a, st=None, off=ALIGNED: _strided(D, a, st or _contig(a.shape), off)  # noqa: E731
    same = lambda got, want: [_same_bits(g, w) for g, w in zip(got, want)]  # noqa: E731
    sixteen = 16 // np.dtype(dtype).itemsize
    A = ALIGNED
    for k, ((px, py, pz), to) in enumerate(TR.ABI_PADS):
        kappa, m2, taper = ABI_TENSOR[k % 2]
        nf = TR._nf(nz, to)
        levels = {"mx": nz, "my": nz, "mz": nf}
        form = lambda f, n: {"z": (1, n, 1, 1), "p": (1, 1, ny, nx), "v3": (1, n, ny, nx), "vl": (lead, n, ny, nx)}[f]  # noqa: E731
        val = lambda name, f: R.synthetic_metric(form(f, levels[name]), 111 + "zpv3vl".index(f) + ord(name[1])).astype(dtype)  # noqa: E731
        b = put(bv)
        assert b.is_contiguous() and b.data_ptr() % 16 == 0
        for present in ({"mx": "p"}, {"my": "p"}, {"mz": "z"}, {"mx": "p", "my": "p", "mz": "z"}, {"mx": "v3", "my": "vl", "mz": "v3"},
                        {"mx": "vl", "my": "z", "mz": "p"}, {"mx": "z", "my": "v3", "mz": "vl"}, {}):
            pv = {n: val(n, f) for n, f in present.items()}
            aligned = {n: put(a) for n, a in pv.items()}
            control = _abi_call(D, dtype, shape, b, aligned, k)
            want = _tensor(*TI._want(bv, (px, py, pz), to, FILL, pv.get("mx"), pv.get("my"), pv.get("mz")), kappa, np.sqrt(m2) if taper else None)
            assert control[0].dtype == want[0].dtype == np.dtype(dtype)
            same(control, want)
            assert not np.isnan(want[0]).all() and np.isfinite(want[2]).any() and (want[0] != want[1]).any()
            views = [(put(bv, off=1), aligned, (A, A, A))]     # b one element in: the narrow form
            assert views[0][0].data_ptr() % 16 == np.dtype(dtype).itemsize
            views += [(b, aligned, offs) for offs in ((0, 0, 0), (sixteen, sixteen, sixteen), (1, A, A), (A, 1, A), (A, A, 1), (1, 1, 1),
                                                      (0, sixteen, 1))]
            # the planes one element in; with an odd row pitch; with an odd level pitch (volumes)
            views.append((b, {n: put(a, off=1) for n, a in pv.items()}, (A, A, A)))
            pitched = {}
            for n, a in pv.items():
                s = list(a.shape)
                pitched[n] = put(a, _contig(s[:-1] + [s[-1] + 1]) if s[-1] > 1 else _contig(s))
                assert s[-1] == 1 or (pitched[n].stride(-2) == nx + 1 and pitched[n].stride(-1) == 1)
            views.append((b, pitched, (A, A, A)))
            for n, f in present.items():
                a, nl = pv[n], levels[n]
                if f in ("v3", "vl"):
                    st = [(nl * (ny * nx + 1)) * (a.shape[0] > 1), ny * nx + 1, nx, 1]
                    lev = put(a, [s or 1 for s in st])
                    assert lev.stride(1) == ny * nx + 1
                    views.append((b, dict(aligned, **{n: lev}), (A, A, A)))
                if f == "z":   # the Z-only metric three elements apart
                    views.append((b, dict(aligned, **{n: put(a, [3 * nl, 3, 1, 1], 1)}), (A, A, A)))
                if f == "p":   # the plane stored (X, Y): a transposed view
                    t = put(np.ascontiguousarray(a.transpose(0, 1, 3, 2))).permute(0, 1, 3, 2)
                    assert t.stride(-1) == ny and t.stride(-2) == 1
                    views.append((b, dict(aligned, **{n: t}), (A, A, A)))
            for b_, planes, offs in views:
                same(_abi_call(D, dtype, shape, b_, planes, k, offs), control)
        # stride-0 metrics along X and Y: one value per level, expanded over the whole volume, equal the Z-only metrics
        flat = {n: put(val(n, "z")).expand(1, levels[n], ny, nx) for n in levels}
        assert all(m.stride(-1) == 0 and m.stride(-2) == 0 for m in flat.values())
        full = {n: put(np.ascontiguousarray(np.broadcast_to(val(n, "z"), (1, levels[n], ny, nx)))) for n in levels}
        same(_abi_call(D, dtype, shape, b, flat, k), _abi_call(D, dtype, shape, b, full, k))
    assert nx % TR.NVS[dtype] == 0 and len(TR.ABI_PADS) >= 2


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_abi_layouts(host_abi, dtype):
    abi_layout_cases(dtype)


def abi_bad_calls():
    """bad calls return an error code, write nothing and leave the process alone; runs on whatever library `_MEM` serves"""
    import xgcm_amd.device as D

    lib = D._MEM.lib()
    shape = [2, 3, 4]
    t = torch.ones(shape, dtype=torch.float64, device=D._MEM.device)
    outs = [torch.full([3, 3, 4], TR.SENTINEL, dtype=torch.float64, device=D._MEM.device) for _ in range(3)]   # room for Z:outer
    long = torch.full([2 * 36], TR.SENTINEL, dtype=torch.float64, device=D._MEM.device)
    P = lambda x: None if x is None else x.data_ptr()  # noqa: E731

    def call(code=TR.CODE[np.float64], b=t, o=outs, shape=shape, ndim=3, outer=0, bcx=_hip.BC["periodic"], bcy=_hip.BC["extend"],
             bcz=_hip.BC["fill"], mets=(None, None, None), strides=(None, None, None), taper=1):
        margs = [x for pair in zip(mets, strides) for x in pair]
        return lib.xg_redi_tensor(code, P(b), *margs, 1000.0, M2, taper, P(o[0]), P(o[1]), P(o[2]),
                                  None if shape is None else _hip.i64(shape), ndim, outer, bcx, 0.0, bcy, 0.0, bcz, 0.0, D._stream())

    untouched = lambda: all(bool((o == TR.SENTINEL).all()) for o in outs + [long])  # noqa: E731
    for code in (-1, _hip.DTYPE["float16"], _hip.DTYPE["int64"], _hip.DTYPE["int32"], 12, 99):
        assert call(code=code) == -1                              # any other element type: XG_ERR_INVALID
    assert call(b=None) == -1 and call(shape=None) == -1          # NULL arguments
    for k in range(3):                                            # a NULL result, each of the three
        assert call(o=[None if j == k else outs[j] for j in range(3)]) == -1
    assert call(taper=2) == -1 and call(taper=-1) == -1           # the taper flag
    assert call(bcx=7) == -1 and call(bcy=-1) == -1 and call(bcz=9) == -1           # unknown boundary codes
    assert call(outer=2) == -1 and call(outer=-1) == -1           # unknown face position
    assert call(shape=[0, 3, 4]) == -1                            # nz = 0: no level to pad from
    for k in range(3):                                            # a metric without strides, each of the three
        assert call(mets=tuple(t.data_ptr() if j == k else None for j in range(3))) == -1
    # results that overlap: the same array twice, each pair; one result beginning inside another (24 elements each here)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        o = list(outs)
        o[j] = o[i]
        assert call(o=o) == -1
    assert call(o=[long[0:24], long[23:47], outs[2]]) == -1 and call(o=[long[30:54], outs[1], long[8:32]]) == -1
    assert call(ndim=2) < 0 and call(ndim=2) != -1                # XG_ERR_UNSUPPORTED
    assert untouched()
    assert call(shape=[2, 0, 4]) == 0 and call(shape=[2, 3, 0]) == 0 and untouched()   # an empty plane: nothing to do
    assert call(o=[long[0:24], long[24:48], outs[2]]) == 0        # results end to end do not overlap
    assert call() == 0 and call(bcz=_hip.BC["periodic"], outer=1, taper=0) == 0 and call(bcz=_hip.BC["extend"], outer=1) == 0
    assert not any(bool((o == TR.SENTINEL).all()) for o in outs)


def test_abi_refuses_bad_calls(host_abi):
    abi_bad_calls()


def test_empty_results_return_without_a_launch(host_abi, monkeypatch):
    import xgcm_amd.device as D

    monkeypatch.setattr(D, "_check", lambda rc: pytest.fail("the library was called for an empty result"))
    for shape in ((2, 3, 0, 4), (0, 3, 5, 4), (3, 5, 0)):
        outs = D.redi_tensor(np.zeros(shape), None, None, None, 1000.0, M2, True, "periodic", "fill", "extend")
        assert len(outs) == 3
        assert all(tuple(o.shape) == shape[:-3] + (shape[-3] + 1,) + shape[-2:] and o.numel() == 0 for o in outs)


# ---- 8. the tunable call table, between guard bands -------------------------------------------------------------------------
def tunable_calls(D, dtype):
    """(calls, references) of the K7r tunable sweep: name -> thunk that calls `D` on inputs uploaded once, name -> thunk that
    gives numpy's three results of the same call.  The battery's own shapes, both face positions; planes with a profile,
    three volumes, and no metric; tapered and untapered in turns"""
    f = lambda shape, seed: R.synthetic_field(shape, seed).astype(dtype)  # noqa: E731
    m = lambda shape, seed: R.synthetic_metric(shape, seed).astype(dtype)  # noqa: E731
    calls, references = {}, {}
    for n, shape in enumerate(((5, 300, 264), (3, 65, 131))):
        nz, ny, nx = shape
        b = f(shape, 150 + n)
        b[1, 7, 9] = b[0, 0, 0] = b[nz - 1, ny - 1, nx - 1] = np.nan
        dev = D.asdevice(b)
        for k, (to, pads) in enumerate((("left", ("periodic", "extend", "fill")), ("outer", ("extend", "fill", "periodic")),
                                        ("left", ("fill", "periodic", "extend")), ("outer", ("periodic", "periodic", "fill")))):
            nf = nz + (to == "outer")
            if k % 2:
                mets = [m((1, ny, nx), 170), m((1, ny, nx), 171), m((nf, 1, 1), 172)]
            else:
                mets = [m((nz, ny, nx), 173), m((nz, ny, nx), 174), m((nf, ny, nx), 175)]
            if k == 2:
                mets = [None, None, None]
            dm = tuple(None if x is None else D.asdevice(x) for x in mets)
            key = f"{nx}{to}{pads[2]}"
            fill = [FILL[a] for a in "XYZ"]
            kappa, sm = KAPPAS[(n + k) % 3], (SMAX, None)[(n + k // 2) % 2]
            m2 = None if sm is None else sm * sm
            calls[key] = lambda dev=dev, dm=dm, to=to, pads=pads, kappa=kappa, m2=m2: D.redi_tensor(
                dev, *dm, float(kappa), m2, to == "outer", *pads, *fill)
            references[key] = lambda h=b, mets=mets, to=to, pads=pads, kappa=kappa, sm=sm: list(
                _tensor(*TI._want(h, pads, to, FILL, *mets), kappa, sm))
    return calls, references


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_the_tunable_call_table_equals_its_numpy_references(host_abi, dtype):
    """the thunks the GPU suite sweeps over every tunable value, once through the host build (which reads no tunable): the
    arguments, their order, the shapes and the references are checked before any GPU time is spent on them"""
    import xgcm_amd.device as D

    calls, references = tunable_calls(D, dtype)
    assert len(calls) == 8 and set(calls) == set(references)
    for name, thunk in calls.items():
        got, want = [D.tohost(x) for x in thunk()], references[name]()
        assert len(got) == len(want) == 3, name
        for g, w in zip(got, want):
            assert g.dtype == np.dtype(dtype) and np.isnan(w).any() and np.isnan(w).mean() < 0.4, name   # (0 * inf: a whole face under `extend`)
            assert TI._bits_equal(g, w), name
        assert (want[0] != want[1]).any() and (want[2] != want[0]).any()


def guarded_table(D, monkeypatch, dtype, offset, same_bits):
    """the table built and run between guard bands: a store outside any of the three results, a cell left unwritten and a
    result-changing read outside the field or a metric all fail; returns the number of results checked"""
    checked = 0
    with GM.guarded(D, monkeypatch, offset) as g:
        calls, references = tunable_calls(D, dtype)
        assert g.placed >= 2 + 2 * 3 * 3          # the field of both shapes, the metrics of the calls that have them
        for k, fn in calls.items():
            before = g.handed_out
            got = [D.tohost(x) for x in fn()]
            g.check(f"{k} at offset {offset}")
            assert g.handed_out - before >= 3     # all three results between guards
            for x, want in zip(got, references[k]()):
                assert same_bits(x, want), f"{k} at offset {offset}: not numpy's result"
                checked += 1
    return checked


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_between_guard_bands_through_the_host_abi(host_abi, monkeypatch, dtype):
    import xgcm_amd.device as D

    for offset in (0, 16, np.dtype(dtype).itemsize):
        assert guarded_table(D, monkeypatch, dtype, offset, TI._bits_equal) == 24
