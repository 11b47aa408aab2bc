"""The Gent-McWilliams eddy-induced (bolus) velocity, `Grid.bolus_velocity`, on CPU.

The one-pass path runs through the `host_abi` fixture (the product's `xgcm_amd.device` over libxgcm_host.so); the chain it
replaces

    step = grid.derivative | grid.diff
    px = interp(kwx, X);  py = interp(kwy, Y)
    closed: px, py = copies with face 0 (and, at Z:outer, face nz) set to +0.0
    ub = -step(px, Z);  vb = -step(py, Z)
    tx = px [* dyG];  ty = py [* dxG]
    wb = divergence(tx, ty)

runs through the same Grid over the oracle double, installed AFTER the one-pass calls of a test have run.  `_want` states the
chain a third time, over plain numpy arrays with the oracle's `stencil1d` and `binary`.  Every comparison is bit for bit (NaN
where the other has NaN, -0.0 is not +0.0), with dims, coords and names where labels are compared.  The one-pass device entry
is counted and the chain's device functions are barred wherever a case must not pass by falling back.

Asserted on the REFERENCE alone, before the kernel is compared (`Table`): every result cell of an ORDINARY case -- seeded kwx
and kwy of order 1, positive metrics, no planted NaN, no all-zero field, no NaN fill -- is finite, and at least half of the
cells of EACH of the three results of every table are non-zero.  No case is left out of a comparison."""

import itertools

import numpy as np
import pytest
import torch

import guarded_memory as GM
import test_isopycnal_slope as TI
import test_richardson_number as TR
from oracle import refimpl as R
from test_fused_layouts import ALIGNED, _contig, _strided
from xgcm_amd import DataArray, Dataset, Grid, _hip
from xgcm_amd.chunked import BlockArray

BCS, TOS, PADS3, FILL, FILLS, AXES, ZDIM = TR.BCS, TR.TOS, TR.PADS3, TR.FILL, TR.FILLS, TR.AXES, TR.ZDIM
NZS, NYS, NXS = TR.NZS, TR.NYS, TR.NXS
_same_labelled, _same_bits, _same_error, _bits_equal = TR._same_labelled, TR._same_bits, TR._same_error, TI._bits_equal
ZERO_FILL = {"X": 0.0, "Y": 0.0, "Z": 0.0}
METRICS = [None, "planes", "full", "lead"]
NAMES = ("mzu", "mzv", "dyg", "dxg", "ra")


def _stage_dims(to):
    """the dims of the five metrics' stages behind the leading dims: ub's, vb's, px's, py's, wb's"""
    zf = ZDIM[to]
    return ("ZC", "YC", "XG"), ("ZC", "YG", "XC"), (zf, "YC", "XG"), (zf, "YG", "XC"), (zf, "YC", "XC")


def _grid(lead, nz, ny, nx, dtype, padding, metric="planes"):
    """the C-grid of tests/test_redi_vertical_flux_divergence.py with the metrics this operator reads.  "planes": dyG(YC, XG)
    as the Y metric, dxG(YG, XC) as the X metric, rA(YC, XC) for (X, Y) and the profile drF(ZC); "full": 3-D arrays at each
    stage's points, for both face positions; "lead": the same with the first leading dim in front; None: no metric at all"""
    dims = ("time", "member")[:len(lead)]
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0),
              "YC": ("YC", np.arange(ny) + 0.5), "YG": ("YG", np.arange(ny) * 1.0),
              "ZC": ("ZC", np.arange(nz) + 0.5), "ZL": ("ZL", np.arange(nz) * 1.0), "ZO": ("ZO", np.arange(nz + 1) * 1.0)}
    for d, n in zip(dims, lead):
        coords[d] = (d, np.arange(n) * 2.0)
    m = lambda shape, seed: R.synthetic_metric(shape, seed).astype(dtype)  # noqa: E731
    data, metrics = {}, {}
    if metric == "planes":
        data = {"dyG": (("YC", "XG"), m((ny, nx), 61)), "dxG": (("YG", "XC"), m((ny, nx), 62)), "rA": (("YC", "XC"), m((ny, nx), 63)),
                "drF": (("ZC",), m((nz,), 65))}
        metrics = {("Y",): ["dyG"], ("X",): ["dxG"], ("X", "Y"): ["rA"], ("Z",): ["drF"]}
    elif metric is not None:
        pl, pd = ((lead[0],), dims[:1]) if metric == "lead" and lead else ((), ())
        f = {"ZL": nz, "ZO": nz + 1}
        data = {"hzu": (pd + ("ZC", "YC", "XG"), m(pl + (nz, ny, nx), 66)), "hzv": (pd + ("ZC", "YG", "XC"), m(pl + (nz, ny, nx), 67))}
        for k, (zd, n) in enumerate(f.items()):
            data["hy" + zd] = (pd + (zd, "YC", "XG"), m(pl + (n, ny, nx), 68 + k))
            data["hx" + zd] = (pd + (zd, "YG", "XC"), m(pl + (n, ny, nx), 70 + k))
            data["ha" + zd] = (pd + (zd, "YC", "XC"), m(pl + (n, ny, nx), 72 + k))
        metrics = {("Z",): ["hzu", "hzv"], ("Y",): ["hyZL", "hyZO"], ("X",): ["hxZL", "hxZO"], ("X", "Y"): ["haZL", "haZO"]}
    ds = Dataset(data, coords)
    return Grid(ds, coords=AXES, metrics=metrics, padding=padding, autoparse_metadata=False), ds, dims


def _closed_copy(f, to):
    """the closing step of the chain, written out: a copy of the labelled streamfunction with face 0 and (Z:outer) face nz
    at +0.0"""
    data = np.array(np.asarray(f.data), copy=True)
    at = [slice(None)] * data.ndim
    for face in (0, -1) if to == "outer" else (0,):
        at[f.dims.index(ZDIM[to])] = face
        data[tuple(at)] = 0.0
    return f._replace(data=data)


def _chain(grid, kwx, kwy, x_axis="X", y_axis="Y", z_axis="Z", closed=True, padding=None, fill_value=None, metric_weighted=True):
    """the specification; the face position is read from kwx's own Z dim"""
    kw = dict(padding=padding, fill_value=fill_value)
    step = grid.derivative if metric_weighted else grid.diff
    px = grid.interp(kwx, x_axis, **kw)
    py = grid.interp(kwy, y_axis, **kw)
    to = next((p for p in ("outer", "left") if ZDIM[p] in getattr(px, "dims", ())), None)
    if closed and to is not None:
        px = _closed_copy(px, to) if ZDIM[to] in px.dims else px
        py = _closed_copy(py, to) if ZDIM[to] in py.dims else py
    ub = -step(px, z_axis, **kw)
    vb = -step(py, z_axis, **kw)
    tx, ty = px, py
    if metric_weighted:
        tx = px * grid.get_metric(px, (y_axis,))
        ty = py * grid.get_metric(py, (x_axis,))
    wb = grid.divergence(tx, ty, x_axis, y_axis, metric_weighted=metric_weighted, **kw)
    return ub, vb, wb


def _psi(kwx, kwy, pads, to, closed, fill=FILL):
    """the streamfunction at u's and at v's columns, the statement's own: the oracle's one-axis function, then the closing"""
    y, x = kwx.ndim - 2, kwx.ndim - 1
    with np.errstate(all="ignore"):
        px = R.stencil1d("interp", kwx, x, 1, 0, pads[0], fill["X"])
        py = R.stencil1d("interp", kwy, y, 1, 0, pads[1], fill["Y"])
    if closed:
        for p in (px, py):
            p[..., 0, :, :] = 0.0
            if to == "outer":
                p[..., -1, :, :] = 0.0
    return px, py


def _want(kwx, kwy, pads, to, closed, fill=FILL, mzu=None, mzv=None, dyg=None, dxg=None, ra=None):
    """the numpy statement of the chain: (ub, vb, wb)"""
    z, y, x = kwx.ndim - 3, kwx.ndim - 2, kwx.ndim - 1
    px, py = _psi(kwx, kwy, pads, to, closed, fill)
    minus = np.full((1,) * kwx.ndim, -1.0, kwx.dtype)
    hi = 0 if to == "outer" else 1
    with np.errstate(all="ignore"):
        ub = R.binary("mul", minus, R.stencil1d("diff", px, z, 0, hi, pads[2], fill["Z"], m_out=mzu))
        vb = R.binary("mul", minus, R.stencil1d("diff", py, z, 0, hi, pads[2], fill["Z"], m_out=mzv))
        tx = px if dyg is None else R.binary("mul", px, dyg)
        ty = py if dxg is None else R.binary("mul", py, dxg)
        wb = R.binary("add", R.stencil1d("diff", tx, x, 0, 1, pads[0], fill["X"]), R.stencil1d("diff", ty, y, 0, 1, pads[1], fill["Y"]))
        if ra is not None:
            wb = R.binary("div", wb, ra)
    nz = kwx.shape[z] - (to == "outer")
    lshape = kwx.shape[:z] + (nz,) + kwx.shape[y:]
    assert ub.shape == vb.shape == lshape and wb.shape == kwx.shape and {ub.dtype, vb.dtype, wb.dtype} == {kwx.dtype}
    return ub, vb, wb


def _metrics_of(ds, metric, to, dims):
    """(mzu, mzv, dyg, dxg, ra) of `_grid` as numpy arrays that broadcast against their stage behind the leading dims `dims`"""
    if metric is None:
        return (None,) * 5
    zf = ZDIM[to]
    names = ("drF", "drF", "dyG", "dxG", "rA") if metric == "planes" else ("hzu", "hzv", "hy" + zf, "hx" + zf, "ha" + zf)
    return tuple(TR._aligned(ds[n], dims + sd) for n, sd in zip(names, _stage_dims(to)))


class Case:
    """one call of the operator: the grid, its dataset and metric form, seeded kwx and kwy at the faces, the keywords"""

    def __init__(self, lead, nz, ny, nx, dtype, pads, to, metric="planes", closed=True, weighted=True, fill=FILL, nan=False, seed=0,
                 zero=False):
        self.pads, self.to, self.metric, self.nan, self.zero, self.closed = tuple(pads), to, metric, nan, zero, closed
        self.grid, self.ds, self.dims = _grid(lead, nz, ny, nx, dtype, dict(zip("XYZ", pads)), metric=metric)
        fshape, fdims = tuple(lead) + (TR._nf(nz, to), ny, nx), self.dims + (ZDIM[to], "YC", "XC")
        vals = [np.zeros(fshape, dtype) if zero else R.synthetic_field(fshape, 901 + 2 * seed + j).astype(dtype) for j in range(2)]
        if nan:
            for j, v in enumerate(vals):
                v.reshape(-1)[3 + j::11] = np.nan
        self.kwx, self.kwy = DataArray(vals[0], fdims, name="kwx"), DataArray(vals[1], fdims, name="kwy")
        self.kw = dict(closed=closed, fill_value=fill, metric_weighted=bool(weighted and metric is not None))
        self.nz, self.lead, self.dtype = nz, tuple(lead), dtype

    def __repr__(self):
        return (f"{self.kwx.shape} {np.dtype(self.dtype)} {self.pads} {self.to} metric {self.metric} nan {self.nan} zero {self.zero} "
                f"{self.kw}")

    def dims_of(self):
        u, v, _, _, w = _stage_dims(self.to)
        return self.dims + u, self.dims + v, self.dims + w

    def one_pass(self):
        return self.grid.bolus_velocity(self.kwx, self.kwy, **self.kw)

    def chain(self):
        return _chain(self.grid, self.kwx, self.kwy, **self.kw)

    def metrics(self):
        return _metrics_of(self.ds, self.metric if self.kw["metric_weighted"] else None, self.to, self.dims)

    def want(self):
        fill = self.kw["fill_value"] or ZERO_FILL
        return _want(self.kwx.values, self.kwy.values, self.pads, self.to, self.closed, fill, *self.metrics())

    def ordinary(self):
        fill = self.kw["fill_value"] or {}
        return not (self.nan or self.zero or any(np.isnan(x) for x in fill.values()))


class Table:
    """what the statement alone must satisfy over the cases of one test"""

    def __init__(self):
        self.ordinary, self.cells, self.nonzero = 0, [0, 0, 0], [0, 0, 0]

    def add(self, c, want):
        if c.ordinary():
            assert all(np.isfinite(w).all() for w in want), c
            self.ordinary += 1
        for k, w in enumerate(want):
            self.cells[k] += w.size
            self.nonzero[k] += int((w != 0).sum())     # (a NaN is not zero)

    def solid(self):
        assert all(c > 0 and 2 * n >= c for n, c in zip(self.nonzero, self.cells)), (self.nonzero, self.cells)
        return self.ordinary


def _counted(monkeypatch, bar_chain=True):
    """the calls of the one-pass device entry; `bar_chain`: and those of the chain's own device functions"""
    import xgcm_amd.device as D

    calls = {"fused": 0, "chain": 0}

    def counted(fn, key):
        def wrapped(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(D, "bolus_velocity", counted(D.bolus_velocity, "fused"))
    if bar_chain:
        for name in ("binary", "stencil1d", "divergence"):
            monkeypatch.setattr(D, name, counted(getattr(D, name), "chain"))
    return calls


def compare_with_numpy(cases, monkeypatch=None):
    """the three results of every case against the numpy statement, bit for bit, the statement first held to `Table`; on
    whatever library `_MEM` serves.  With `monkeypatch`: exactly one call of the one-pass entry per case and none of the
    chain's.  Returns the number of ordinary cases"""
    calls = _counted(monkeypatch) if monkeypatch is not None else None
    table, wants = Table(), []
    for c in cases:
        wants.append(c.want())
        table.add(c, wants[-1])
    solid = table.solid()
    for c, want in zip(cases, wants):
        got = c.one_pass()
        try:
            assert len(got) == 3
            for g, w, dims in zip(got, want, c.dims_of()):
                _same_bits(g.values, w)
                assert g.dims == dims
        except AssertionError as err:
            raise AssertionError(f"case {c}") from err
    if calls is not None:
        assert calls == {"fused": len(cases), "chain": 0}
    return solid


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
            for g, w in zip(triple, want):
                _same_labelled(g, w)
                _same_bits(g.values, w.values)
        except AssertionError as err:
            raise AssertionError(f"case {c}") from err


# ---- 1. small shapes -------------------------------------------------------------------------------------------------------
def shape_cases(nx):
    """every nz and ny with this nx, both face positions and both closings for each -- one level, one row (both neighbours
    are pads), one column, nx across a tile's last lane, odd nx (the narrow form) -- the boundary triple, the dtype, the
    metric form and the fills rotating"""
    out = []
    for n, (nz, ny, to, closed) in enumerate(itertools.product(NZS, NYS, TOS, (True, False))):
        k = n + 5 * NXS.index(nx)
        out.append(Case((), nz, ny, nx, (np.float64, np.float32)[(k // 4) % 2], PADS3[(7 * k) % 27], to, METRICS[(k // 4) % 3 + (k % 5 == 0)],
                        closed, fill=FILLS[0 if k % 3 else (k // 3) % 3], seed=k))
    return out


def shape_table_is_complete():
    """the table as a whole meets every boundary triple, metric form, Z boundary x position x closing x dtype, and every
    nz, ny, position and closing at one column"""
    cases = [c for nx in NXS for c in shape_cases(nx)]
    assert {c.pads for c in cases} == set(PADS3) and {c.metric for c in cases} == set(METRICS)
    assert {(c.pads[2], c.to, c.closed, np.dtype(c.dtype).itemsize) for c in cases} == set(itertools.product(BCS, TOS, (True, False), (4, 8)))
    assert {(c.nz, c.kwx.shape[-2], c.to, c.closed) for c in cases if c.kwx.shape[-1] == 1} == set(itertools.product(NZS, NYS, TOS, (True, False)))


@pytest.mark.parametrize("nx", NXS)
def test_small_shapes(host_abi, monkeypatch, nx):
    cases = shape_cases(nx)
    assert len(cases) == 4 * len(NZS) * len(NYS)
    if nx == NXS[0]:
        shape_table_is_complete()
    compare_with_numpy(cases)
    compare_with_chain(monkeypatch, cases)


def test_one_level_closed_at_outer_is_all_minus_zero(host_abi, monkeypatch):
    """nz = 1, Z:outer, closed: both faces of psi are +0.0, so ub and vb are -(+0.0 [/ drF]) = -0.0 everywhere"""
    calls = _counted(monkeypatch)
    for metric in ("planes", None):
        c = Case((2,), 1, 3, 8, np.float64, ("periodic", "extend", "fill"), "outer", metric, True)
        ub, vb, wb = c.want()
        assert (ub == 0).all() and np.signbit(ub).all() and (vb == 0).all() and np.signbit(vb).all()
        compare_with_numpy([c, Case((2,), 1, 3, 8, np.float64, ("periodic", "extend", "fill"), "outer", metric, False)])
    assert calls == {"fused": 4, "chain": 0}


# ---- 2. every boundary triple, metric forms, leading dims, mid size ---------------------------------------------------------
LEAD_CASES = [((), 4, 5, 8, "planes"), ((2,), 3, 5, 6, "full"), ((2, 3), 3, 4, 5, "lead"), ((2, 3), 2, 3, 12, "planes")]


def matrix_cases(pads, dtype):
    """leading dims (), (2,), (2, 3) x both face positions x both closings, weighted or not and the fills rotating"""
    out = []
    for n, ((lead, nz, ny, nx, metric), to, closed) in enumerate(itertools.product(LEAD_CASES, TOS, (True, False))):
        out.append(Case(lead, nz, ny, nx, dtype, pads, to, metric, closed, weighted=n % 5 != 2, fill=FILLS[0 if n % 4 else (n // 4) % 3],
                        nan=n % 8 == 7, seed=n))
    return out


@pytest.mark.parametrize("px,py,pz", PADS3)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_every_boundary_triple(host_abi, monkeypatch, px, py, pz, dtype):
    cases = matrix_cases((px, py, pz), dtype)
    assert {(c.to, c.closed) for c in cases} == set(itertools.product(TOS, (True, False)))
    assert {c.lead for c in cases} == {(), (2,), (2, 3)}
    assert compare_with_numpy(cases) >= 8
    compare_with_chain(monkeypatch, cases)


def metric_cases(dtype):
    """every metric form under every depth of leading dims, both face positions, both closings, and the unweighted call"""
    out = []
    for n, (metric, lead, to) in enumerate(itertools.product(METRICS, [(), (2,), (2, 3)], TOS)):
        out.append(Case(lead, 3, 4, 6, dtype, PADS3[(5 * n + 1) % 27], to, metric, bool(n % 2), weighted=n % 7 != 3, seed=n))
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_metric_forms_and_leading_dims(host_abi, monkeypatch, dtype):
    cases = metric_cases(dtype)
    assert {c.metric for c in cases} == set(METRICS) and {len(c.dims) for c in cases} == {0, 1, 2}
    assert any(not c.kw["metric_weighted"] and c.metric is not None for c in cases)
    assert compare_with_numpy(cases) > 10
    compare_with_chain(monkeypatch, cases)


def check_each_metric_absent_on_its_own(dtype):
    """the device wrapper with every subset of one, four and five of the metrics and none: a profile, planes, volumes"""
    import xgcm_amd.device as D

    lead, nz, ny, nx = 2, 5, 5, 12     # (nz = 5: closed at Z:outer, four of wb's six faces are open)
    m = lambda shape, seed: R.synthetic_metric(shape, seed).astype(dtype)  # noqa: E731
    subsets = [(k,) for k in NAMES] + [tuple(x for x in NAMES if x != k) for k in NAMES] + [NAMES, ()]
    for n, (present, to, closed) in enumerate(itertools.product(subsets, TOS, (True, False))):
        nf = TR._nf(nz, to)
        forms = {"mzu": m((1, nz, 1, 1), 311), "mzv": m((lead, nz, ny, nx), 312), "dyg": m((1, 1, ny, nx), 313),
                 "dxg": m((1, nf, ny, nx), 314), "ra": m((lead, 1, ny, nx), 315)}
        pads = PADS3[(5 * n + 2) % 27]
        fshape = (lead, nf, ny, nx)
        kwx, kwy = R.synthetic_field(fshape, 320 + n).astype(dtype), R.synthetic_field(fshape, 420 + n).astype(dtype)
        mets = [forms[k] if k in present else None for k in NAMES]
        got = D.bolus_velocity(kwx, kwy, *mets, to == "outer", closed, *pads, *[FILL[x] for x in "XYZ"])
        want = _want(kwx, kwy, pads, to, closed, FILL, *mets)
        for g, w in zip(got, want):
            assert np.isfinite(w).all()
            _same_bits(D.tohost(g), w)
        assert (want[2] != 0).mean() > 0.5


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_each_metric_absent_on_its_own(host_abi, dtype):
    check_each_metric_absent_on_its_own(dtype)


def mid_size_cases(dtype, nx):
    """several tiles, ragged tiles and segments together; nx = 515 takes the narrow form, 516 the vector form"""
    return [Case((2,), 5, 40, nx, dtype, ("periodic", "extend", "fill"), "outer", "full", True),
            Case((2,), 5, 40, nx, dtype, ("fill", "periodic", "extend"), "left", "planes", False),
            Case((), 4, 40, nx, dtype, ("extend", "fill", "periodic"), "left", "planes", True),
            Case((), 4, 40, nx, dtype, ("periodic", "periodic", "periodic"), "outer", None, False)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("nx", [515, 516])
def test_mid_size(host_abi, monkeypatch, dtype, nx):
    assert compare_with_numpy(mid_size_cases(dtype, nx), monkeypatch) == 4


# ---- 3. fills, zeros, closed faces, NaNs --------------------------------------------------------------------------------------
FILL_SETS = [{"X": -0.0, "Y": -0.0, "Z": -0.0}, {"X": float("nan"), "Y": float("nan"), "Z": float("nan")}, FILL,
             {"X": -2.5, "Y": 0.0, "Z": 3.0}]


def fill_cases(dtype):
    """four fill sets -- -0.0, NaN, distinct per axis twice -- with `fill` on one axis after the other and on all three, both
    face positions, both closings"""
    out = []
    for n, (fill, pads, (to, metric), closed) in enumerate(itertools.product(
            FILL_SETS, (("fill", "fill", "fill"), ("fill", "periodic", "extend"), ("extend", "fill", "periodic"), ("periodic", "extend", "fill")),
            (("outer", "planes"), ("left", None)), (True, False))):
        out.append(Case((2,), 3, 4, 6, dtype, pads, to, metric, closed, fill=fill, seed=n))
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_fills_keep_their_bits(host_abi, monkeypatch, dtype):
    cases = fill_cases(dtype)
    assert compare_with_numpy(cases, monkeypatch) == 48
    # a non-zero fill pad on X shows in the last column of a CLOSED face of wb, as the docstring says
    c = Case((), 3, 4, 6, dtype, ("fill", "periodic", "extend"), "outer", "planes", True)
    wb = c.want()[2]
    assert (wb[0, :, -1] != 0).all() and (wb[0, :, :-1] == 0).all() and (wb[-1, :, -1] != 0).all()
    _same_bits(c.one_pass()[2].values, wb)


def zero_cases(dtype):
    return [Case((2,), 3, 4, 6, dtype, pads, to, metric, closed, fill=fill, zero=True)
            for (pads, fill), to, metric, closed in itertools.product(
                ((("periodic", "extend", "periodic"), FILL), (("fill", "fill", "fill"), FILL_SETS[0]), (("fill", "fill", "fill"), ZERO_FILL)),
                TOS, ("planes", None), (True, False))]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_all_zero_fields_give_zeros_of_the_statements_signs(host_abi, dtype):
    """the table's own condition (half the cells non-zero) is not for these: every cell is a zero, and its SIGN is compared.
    ub and vb are -(0 - 0) = -0.0 under periodic / extend; wb is +0.0"""
    signs = set()
    for c in zero_cases(dtype):
        want = c.want()
        if c.pads[0] != "fill" or c.kw["fill_value"] is not FILL:
            assert all((w == 0).all() for w in want), c
        signs |= {bool(s) for w in want for s in np.unique(np.signbit(w))}
        for g, w in zip(c.one_pass(), want):
            _same_bits(g.values, w)
    assert signs == {True, False}


def check_closed_is_closed(dtype):
    """NaN, then 1e300 (float32: 1e30), planted in the closed faces of kwx and kwy changes no bit of any result; open, the
    NaN appears exactly where the statement has it"""
    big = 1e300 if dtype == np.float64 else 1e30
    for n, (to, pads, metric) in enumerate(itertools.product(TOS, [("periodic", "extend", "extend"), ("fill", "periodic", "periodic"),
                                                                    ("extend", "fill", "fill")], ("planes", "full"))):
        faces = (0, -1) if to == "outer" else (0,)
        res = {}
        for closed, plant in itertools.product((True, False), (np.nan, big, None)):
            c = Case((2,), 4, 5, 10, dtype, pads, to, metric, closed, seed=n)
            if plant is not None:
                for k in (c.kwx, c.kwy):
                    for face in faces:
                        k.values[:, face] = plant
            want = c.want()
            for g, w in zip(c.one_pass(), want):
                _same_bits(g.values, w)
            res[closed, plant] = want
        for k in range(3):
            assert np.isfinite(res[True, np.nan][k]).all()
            _same_bits(res[True, np.nan][k], res[True, None][k])
            _same_bits(res[True, big][k], res[True, None][k])
        nan = [np.isnan(x) for x in res[False, np.nan]]
        assert nan[0][:, 0].all() and nan[1][:, 0].all() and nan[2][:, 0].all() and not nan[2][:, 1:-1].any()
        assert not nan[0][:, 1:-1].any() and nan[0][:, -1].all() == (to == "outer" or pads[2] == "periodic")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_closed_really_is_closed(host_abi, dtype):
    check_closed_is_closed(dtype)


def check_nan_locality(to, pads, closed):
    """one NaN at a time in an interior face of kwx, then of kwy: NaN in the results exactly where the statement has it -- in
    the middle of the volume ub at levels k-1 and k, columns i and i+1; wb at face k, columns i-1 .. i+1 (through tx[i] and
    tx[i+1]); vb and wb likewise along Y"""
    for which, at in itertools.product((0, 1), [(2, 3, 4), (1, 0, 0), (2, 5, 7), (3, 0, 7)]):
        c = Case((), 5, 6, 8, np.float64, pads, to, "planes", closed)
        (c.kwx, c.kwy)[which].values[at] = np.nan
        got, want = [g.values for g in c.one_pass()], c.want()
        for g, w in zip(got, want):
            assert np.array_equal(np.isnan(g), np.isnan(w)), (c, at)
        assert np.isnan(got[which]).any() and not np.isnan(got[1 - which]).any()
        if at == (2, 3, 4):
            k, j, i = at
            mu, mw = np.zeros(got[0].shape, bool), np.zeros(got[2].shape, bool)
            if which == 0:
                mu[k - 1:k + 1, j, i:i + 2] = True
                mw[k, j, i - 1:i + 2] = True
            else:
                mu[k - 1:k + 1, j:j + 2, i] = True
                mw[k, j - 1:j + 2, i] = True
            assert np.array_equal(np.isnan(got[which]), mu) and np.array_equal(np.isnan(got[2]), mw)


@pytest.mark.parametrize("closed", [True, False])
@pytest.mark.parametrize("to", TOS)
@pytest.mark.parametrize("pads", [("periodic", "periodic", "periodic"), ("extend", "fill", "fill"), ("fill", "extend", "extend")],
                         ids=lambda p: "-".join(p))
def test_a_nan_poisons_exactly_what_the_statement_has_as_nan(host_abi, to, pads, closed):
    check_nan_locality(to, pads, closed)


def nan_cases(dtype):
    return [Case((2,), 4, 5, 9, dtype, PADS3[(4 * n) % 27], TOS[n % 2], METRICS[n % 4], bool(n % 3), nan=True, seed=n) for n in range(12)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_planted_nans_land_where_the_statement_has_them(host_abi, dtype):
    for c in nan_cases(dtype):
        want = c.want()
        assert all(np.isnan(w).any() and not np.isnan(w).all() for w in want), c
        for g, w in zip(c.one_pass(), want):
            _same_bits(g.values, w)


# ---- 4. on redi_tensor's own results; continuity ---------------------------------------------------------------------------
def check_on_redi_tensors_own_results(dtype):
    """`redi_tensor(b)` under `extend` at Z:outer has NaN outermost faces; with the default `closed=True` all three results
    of the bolus velocity are finite"""
    import test_redi_tensor as TD

    base = TI.Case((2,), 5, 9, 12, dtype, ("periodic", "extend", "extend"), "outer", "planes")
    b = DataArray(R.synthetic_field(base.b.shape, 77).astype(dtype), base.b.dims, name="b")
    kwx, kwy, _ = base.grid.redi_tensor(b, 1000.0, TD.SMAX, fill_value=FILL)
    assert np.isnan(kwx.values[:, [0, -1]]).all() and np.isfinite(kwx.values[:, 1:-1]).all()
    c = Case((2,), 5, 9, 12, dtype, base.pads, "outer", "planes", True)
    got = c.grid.bolus_velocity(kwx, kwy, fill_value=FILL)         # the defaults
    want = _want(kwx.values, kwy.values, c.pads, "outer", True, FILL, *c.metrics())
    for g, w, dims in zip(got, want, c.dims_of()):
        assert np.isfinite(w).all() and (w != 0).mean() > 0.5
        _same_bits(g.values, w)
        assert g.dims == dims


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_on_redi_tensors_own_results(host_abi, monkeypatch, dtype):
    calls = _counted(monkeypatch, bar_chain=False)
    check_on_redi_tensors_own_results(dtype)
    assert calls["fused"] == 1


CONTINUITY_ROUNDINGS = 6


def check_continuity(dtype):
    """At Z:outer with the profile drF, periodic X and Y, cell by cell

        | div(ub dyG, vb dxG) drF + (wb[k+1] - wb[k]) rA |  <=  CONTINUITY_ROUNDINGS * (eps / 2) * S

    S = the sum of |psi * metric| over the sixteen products the cell touches (px dyG at columns i, i+1 and py dxG at rows j,
    j+1, at faces k and k+1, each once in the horizontal and once in the vertical part).  In exact arithmetic the two parts
    cancel product by product.  The operator's roundings, eps / 2 each, relative to a product: in ub, the difference of the
    two faces and the quotient by drF: 2 (the negation is exact); in wb, the product psi * metric, the difference along its
    axis, the sum of the two differences and the quotient by rA: 4.  The six act on different copies of one product, so the
    first-order bound is 6 * (eps / 2) * S, and that is what is asserted (the second order is O(eps^2)).  The combination
    itself is evaluated in a wider format (float64 for float32 results, long double for float64), so it adds no rounding of the results' size"""
    eps = float(np.finfo(dtype).eps)
    wide = np.float64 if dtype == np.float32 else np.longdouble
    worst = 0.0
    for closed, lead in itertools.product((True, False), ((), (2,))):
        c = Case(lead, 5, 9, 12, dtype, ("periodic", "periodic", "fill"), "outer", "planes", closed, seed=3)
        ub, vb, wb = (np.asarray(g.values).astype(wide) for g in c.one_pass())
        mzu, mzv, dyg, dxg, ra = (np.asarray(m).astype(wide) for m in c.metrics())
        px, py = (p.astype(wide) for p in _psi(c.kwx.values, c.kwy.values, c.pads, "outer", closed))
        east = lambda f: np.roll(f, -1, axis=-1)     # noqa: E731
        north = lambda f: np.roll(f, -1, axis=-2)    # noqa: E731
        fu, fv = ub * dyg, vb * dxg
        total = ((east(fu) - fu) + (north(fv) - fv)) * mzu + (wb[..., 1:, :, :] - wb[..., :-1, :, :]) * ra
        ax, ay = np.abs(px * dyg), np.abs(py * dxg)
        per_face = ax + east(ax) + ay + north(ay)
        S = 2 * (per_face[..., 1:, :, :] + per_face[..., :-1, :, :])
        assert (S > 0).all() and (np.abs(total) <= CONTINUITY_ROUNDINGS * (eps / 2) * S).all(), float((np.abs(total) / S).max() / eps)
        assert (total != 0).any()
        worst = max(worst, float((np.abs(total) / S).max() / eps))
    return worst


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_the_bolus_velocity_is_non_divergent_cell_by_cell(host_abi, dtype):
    print(f"continuity: worst |residual| / S = {check_continuity(dtype):.3f} eps")


# ---- 5. labels, residency, xarray ------------------------------------------------------------------------------------------
def label_cases():
    cases = []
    for n, name in enumerate(("kwx", "dyG", "drF", None, "hzu", "haZO")):
        for metric, to in (("planes", "outer"), ("full", "outer"), ("full", "left"), (None, "left")):
            c = Case((2,), 3, 5, 6, np.float64, ("periodic", "extend", "fill"), to, metric, bool(n % 2), seed=n)
            zf = ZDIM[to]
            c.kwx = c.kwx._replace(name=name).assign_coords({"depth": ((zf,), np.arange(c.kwx.shape[1]) * 10.0), "t2": (("time",), np.arange(2) + 9.0),
                                                             "lonC": (("YC", "XC"), np.ones((5, 6)))})
            c.kwy = c.kwy._replace(name=(name, "kwx", "kwy")[n % 3]).assign_coords({"latC": (("YC", "XC"), np.ones((5, 6)) * 2),
                                                                                    "t3": (("time",), np.arange(2) - 1.0)})
            cases.append(c)
    return cases


def test_coords_and_names_follow_the_chain(host_abi, monkeypatch):
    compare_with_chain(monkeypatch, label_cases())


def test_xarray_in_xarray_out(host_abi, monkeypatch):
    import xarray_standin
    from oracle import fake_device

    xarray_standin.install(monkeypatch)
    import xarray as xr

    c = Case((), 3, 4, 6, np.float64, ("periodic", "fill", "extend"), "left", "planes", True)
    X = lambda d: xr.DataArray(d.values, dims=d.dims, name=d.name)  # noqa: E731
    got = c.grid.bolus_velocity(X(c.kwx), X(c.kwy), **c.kw)
    assert all(type(g).__module__.split(".")[0] == "xarray" for g in got)
    fake_device.install(monkeypatch)
    with np.errstate(all="ignore"):
        want = c.chain()
    for g, w in zip(got, want):
        assert tuple(g.dims) == tuple(w.dims) and g.name == w.name
        _same_bits(np.asarray(g.values), np.asarray(w.values))


def test_under_fused_the_one_pass_runs_as_it_does_outside(host_abi, monkeypatch):
    calls = _counted(monkeypatch)
    for closed in (True, False):
        c = Case((2,), 3, 5, 6, np.float64, ("periodic", "extend", "fill"), "outer", "planes", closed)
        with c.grid.fused():
            got = c.one_pass()
        for g, w in zip(got, c.want()):
            assert isinstance(g.data, np.ndarray)
            _same_bits(g.values, w)
    assert calls == {"fused": 2, "chain": 0}


# ---- 6. seeded fuzz ---------------------------------------------------------------------------------------------------------
def fuzz_cases(seed=20261021, n=120):
    """cases over the small shapes, the boundary triples, both face positions and closings, the fills, the dtype, the metric
    forms and the leading dims; a fifth of them with NaNs"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        lead = [(), (2,), (2, 3)][int(rng.integers(3))]
        nz, ny = int(rng.choice(NZS)), int(rng.choice(NYS))
        nx = int(rng.choice([1, 2, 3, 8, 13, 16, 129, 130, 132])) if not lead else int(rng.choice([1, 2, 5, 8, 12]))
        out.append(Case(lead, nz, ny, nx, (np.float64, np.float32)[int(rng.integers(2))], PADS3[int(rng.integers(27))], TOS[int(rng.integers(2))],
                        METRICS[int(rng.integers(4))], bool(rng.integers(2)), weighted=bool(rng.integers(4)),
                        fill=(FILLS + FILL_SETS)[int(rng.integers(7))] if rng.integers(3) == 0 else FILL, nan=rng.integers(5) == 0, seed=k))
    return out


def test_seeded_fuzz(host_abi, monkeypatch):
    cases = fuzz_cases()
    assert len(cases) == 120 and compare_with_numpy(cases) >= 40
    compare_with_chain(monkeypatch, cases)


# ---- 7. every fallback of the docstring takes the chain ---------------------------------------------------------------------
def _chain_counted(monkeypatch):
    """no call of the one-pass entry; the chains that ran: each makes two calls of `Grid.interp` and one of `Grid.divergence`"""
    import xgcm_amd.device as D

    monkeypatch.setattr(D, "bolus_velocity", lambda *a, **k: pytest.fail("one-pass entry called"))
    calls = {"interp": 0, "divergence": 0}
    interp, divergence = Grid.interp, Grid.divergence

    def counted_interp(self, *a, **k):
        calls["interp"] += 1
        return interp(self, *a, **k)

    def counted_divergence(self, *a, **k):
        calls["divergence"] += 1
        return divergence(self, *a, **k)

    monkeypatch.setattr(Grid, "interp", counted_interp)
    monkeypatch.setattr(Grid, "divergence", counted_divergence)
    return calls


def _fallback_equals_chain(calls, grid, kwx, kwy, **kw):
    """one chain inside the operator, bit-equal with its labels to the chain written out here"""
    before = dict(calls)
    with np.errstate(all="ignore"):
        got = grid.bolus_velocity(kwx, kwy, **kw)
        assert calls["interp"] - before["interp"] == 2 and calls["divergence"] - before["divergence"] == 1
        want = _chain(grid, kwx, kwy, **kw)
    assert len(got) == 3
    for g_, w_ in zip(got, want):
        _same_labelled(g_, w_)
        g, w = np.asarray(g_.values), np.asarray(w_.values)
        if g.dtype.itemsize == 2 or g.dtype.kind != "f":
            assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=g.dtype.kind == "f")
        else:
            _same_bits(g, w)
    return got


def _case(pads=("periodic", "extend", "fill"), lead=(), nz=3, ny=5, nx=6, dtype=np.float64, to="outer", metric="planes", closed=True, **kw):
    return Case(lead, nz, ny, nx, dtype, pads, to, metric, closed, **kw)


@pytest.mark.parametrize("dtype", [np.int64, np.int32, np.float16])
def test_integer_and_half_fields_run_the_chain(backend, monkeypatch, dtype):
    calls = _chain_counted(monkeypatch)
    cast = lambda d: DataArray((d.values * 100).astype(dtype), d.dims, name=d.name)  # noqa: E731
    for to, closed in itertools.product(TOS, (True, False)):
        c = _case(to=to)
        _fallback_equals_chain(calls, c.grid, cast(c.kwx), cast(c.kwy), closed=closed, metric_weighted=False, fill_value=FILL)
    c = _case()
    _fallback_equals_chain(calls, c.grid, cast(c.kwx), c.kwy, metric_weighted=False, fill_value=FILL)


def test_mixed_dtypes_run_the_chain(backend, monkeypatch):
    calls = _chain_counted(monkeypatch)
    c = _case()
    got = _fallback_equals_chain(calls, c.grid, DataArray(c.kwx.values.astype(np.float32), c.kwx.dims, name="kwx"), c.kwy, fill_value=FILL)
    assert {np.asarray(g.values).dtype for g in got} == {np.dtype(np.float64)}      # (the chain's promotion, with float64 metrics)


def test_inputs_of_different_shapes_or_positions_do_what_the_chain_does(backend, monkeypatch):
    calls = _chain_counted(monkeypatch)
    c = _case(lead=(2,))
    small = DataArray(np.ascontiguousarray(c.kwy.values[0]), c.kwy.dims[1:], name="kwy")           # a missing leading dim
    shifted = DataArray(c.kwx.values, ("time", "ZO", "YC", "XG"), name="kwx")                        # kwx at u's points
    left = _case(lead=(2,), to="left")
    centre = DataArray(left.kwx.values, ("time", "ZC", "YC", "XC"), name="kwx")                      # no face dim at all
    for grid, kwx, kwy in ((c.grid, c.kwx, small), (c.grid, shifted, c.kwy), (left.grid, left.kwx, c.kwy), (left.grid, centre, centre)):
        for closed in (True, False):
            kw = dict(closed=closed, fill_value=FILL)
            try:
                with np.errstate(all="ignore"):
                    _chain(grid, kwx, kwy, **kw)
            except Exception:
                _same_error(lambda: grid.bolus_velocity(kwx, kwy, **kw), lambda: _chain(grid, kwx, kwy, **kw), own=AttributeError)
            else:
                _fallback_equals_chain(calls, grid, kwx, kwy, **kw)


def _chunked(d, chunks):
    return DataArray(BlockArray.from_array(d.values, chunks), d.dims, name=d.name)


def test_chunked_inputs_run_the_chain_and_psi_is_computed_first(backend, monkeypatch):
    calls = _chain_counted(monkeypatch)
    for closed in (True, False):
        c = _case(lead=(4,), ny=6, nx=8, closed=closed)
        want = c.want()
        ch = ((2, 2), (4,), (6,), (8,))
        for kwx, kwy in ((_chunked(c.kwx, ch), c.kwy), (c.kwx, _chunked(c.kwy, ch)), (_chunked(c.kwx, ch), _chunked(c.kwy, ch))):
            before = calls["interp"]
            with np.errstate(all="ignore"):
                got = c.grid.bolus_velocity(kwx, kwy, closed=closed, fill_value=FILL)
                assert calls["interp"] - before == 2
                chain = _chain(c.grid, kwx, kwy, closed=closed, fill_value=FILL)
            for g, w, ww in zip(got, chain, want):
                assert g.dims == w.dims and g.name == w.name
                _same_bits(np.asarray(g.values), np.asarray(w.values))
                _same_bits(np.asarray(g.values), ww)


def test_z_elsewhere_runs_the_chain(backend, monkeypatch):
    calls = _chain_counted(monkeypatch)
    c = _case(lead=(2,))
    T = lambda d, *dims: d.transpose(*dims)  # noqa: E731
    for closed in (True, False):
        _fallback_equals_chain(calls, c.grid, T(c.kwx, "ZO", "time", "YC", "XC"), T(c.kwy, "ZO", "time", "YC", "XC"), fill_value=FILL,
                               closed=closed, metric_weighted=False)


def test_a_missing_metric_does_what_the_chain_does(backend, monkeypatch):
    """a grid without an (X, Y) metric and without one of its factors: `get_metric` raises where the chain looks it up"""
    _chain_counted(monkeypatch)
    c = _case()
    ds = Dataset({k: (c.ds[k].dims, np.asarray(c.ds[k].values)) for k in ("dyG", "drF")}, dict(c.ds.coords))
    grid = Grid(ds, coords=AXES, metrics={("Y",): ["dyG"], ("Z",): ["drF"]}, padding=dict(zip("XYZ", c.pads)), autoparse_metadata=False)
    _same_error(lambda: grid.bolus_velocity(c.kwx, c.kwy), lambda: _chain(grid, c.kwx, c.kwy))


@pytest.mark.parametrize("axis", ["X", "Y", "Z"])
def test_an_axis_without_a_boundary_raises_the_chains_error(backend, monkeypatch, axis):
    _chain_counted(monkeypatch)
    pad = {"X": "periodic", "Y": "extend", "Z": "fill"}
    del pad[axis]
    for to in TOS if axis == "Z" else ("outer",):
        c = _case(to=to)
        grid, ds, dims = _grid((), 3, 5, 6, np.float64, pad)
        if axis == "Z" and to == "outer":      # (Z:outer needs no Z pad: the chain runs, and so it runs here)
            calls = _chain_counted(monkeypatch)
            _fallback_equals_chain(calls, grid, c.kwx, c.kwy)
        else:
            _same_error(lambda: grid.bolus_velocity(c.kwx, c.kwy), lambda: _chain(grid, c.kwx, c.kwy))


@pytest.mark.parametrize("conn", ["x2x", "y2y", "z2z"])
def test_connected_faces_run_the_chain(backend, monkeypatch, conn):
    from test_topology import COORDS, X_TO_X

    calls = _chain_counted(monkeypatch)
    ds = Dataset({"drF": (("zc",), R.synthetic_metric((4,), 65)), "dyG": (("y", "xl"), R.synthetic_metric((4, 4), 61)),
                  "dxG": (("yl", "x"), R.synthetic_metric((4, 4), 62)), "rA": (("y", "x"), R.synthetic_metric((4, 4), 63))},
                 coords={"x": np.arange(4), "xl": np.arange(4) - 0.5, "y": np.arange(4), "yl": np.arange(4) - 0.5,
                         "face": np.arange(2), "zc": np.arange(4) + 0.5, "zo": np.arange(5) * 1.0})
    grid = Grid(ds, coords=dict(COORDS, Z={"center": "zc", "outer": "zo"}),
                metrics={("Y",): ["dyG"], ("X",): ["dxG"], ("X", "Y"): ["rA"], ("Z",): ["drF"]},
                face_connections={"x2x": X_TO_X, "y2y": TR.Y_TO_Y, "z2z": TR.Z_TO_Z}[conn],
                padding={"X": "fill", "Y": "extend", "Z": "fill"}, autoparse_metadata=False)
    kwx = DataArray(R.synthetic_field((2, 5, 4, 4), 82), ("face", "zo", "y", "x"), name="kwx")
    kwy = DataArray(R.synthetic_field((2, 5, 4, 4), 83), ("face", "zo", "y", "x"), name="kwy")
    for mw, closed in itertools.product((True, False), (True, False)):
        kw = dict(fill_value=FILL, metric_weighted=mw, closed=closed)
        before = calls["interp"]
        try:
            with np.errstate(all="ignore"):
                step = grid.derivative if mw else grid.diff
                px, py = grid.interp(kwx, "X", fill_value=FILL), grid.interp(kwy, "Y", fill_value=FILL)
                if closed:
                    px, py = (p._replace(data=np.array(np.asarray(p.data), copy=True)) for p in (px, py))
                    for p in (px, py):
                        p.data[:, [0, -1]] = 0.0
                want = [-step(px, "Z", fill_value=FILL), -step(py, "Z", fill_value=FILL)]
                tx, ty = (px * grid.get_metric(px, ("Y",)), py * grid.get_metric(py, ("X",))) if mw else (px, py)
                want.append(grid.divergence(tx, ty, metric_weighted=mw, fill_value=FILL))
        except Exception as err:
            with pytest.raises(type(err)) as got_err:
                grid.bolus_velocity(kwx, kwy, **kw)
            assert str(got_err.value) == str(err)
            continue
        before = calls["interp"]
        with np.errstate(all="ignore"):
            got = grid.bolus_velocity(kwx, kwy, **kw)
        assert calls["interp"] - before == 2
        for g, w in zip(got, want):
            _same_labelled(g, w)


# ---- 8. the entry of the C ABI called directly, with views ------------------------------------------------------------------
def _abi_call(D, dtype, shape, kws, planes, k, off=ALIGNED):
    """one call of xg_bolus_velocity: `kws` (kwx, kwy) and `planes` {mzu, mzv, dyg, dxg, ra} views; each result is written
    `off` elements into an allocation of its own full of SENTINEL, which must still surround it afterwards.  The row of
    TR.ABI_PADS gives the boundary triple and the face position, its parity `closed`"""
    (px, py, pz), to = TR.ABI_PADS[k % len(TR.ABI_PADS)]
    closed = (k // len(TR.ABI_PADS)) % 2
    fshape = list(shape[:-3]) + [TR._nf(shape[-3], to)] + list(shape[-2:])
    args = [TR.CODE[dtype], kws[0].data_ptr(), kws[1].data_ptr()]
    for name in NAMES:
        m = planes.get(name)
        if m is None:
            args += [None, None]
        else:
            assert all(n in (1, s) for n, s in zip(m.shape, shape if name.startswith("mz") else fshape))
            args += [m.data_ptr(), _hip.i64([0 if n == 1 else m.stride(d) for d, n in enumerate(m.shape)])]
    bufs = []
    for s in (shape, shape, fshape):
        n = int(np.prod(s))
        bufs.append((torch.full((off + n + ALIGNED,), TR.SENTINEL, dtype=TR.TORCH[dtype], device=D._MEM.device), n, s))
        args.append(bufs[-1][0][off:off + n].data_ptr())
    args += [_hip.i64(shape), len(shape), int(to == "outer"), closed, _hip.BC[px], FILL["X"], _hip.BC[py], FILL["Y"], _hip.BC[pz], FILL["Z"]]
    D._check(getattr(D._MEM.lib(), "xg_bolus_velocity")(*args, D._stream()))
    outs = []
    for buf, n, s in bufs:
        whole = buf.cpu().numpy()
        assert (whole[:off] == TR.SENTINEL).all() and (whole[off + n:] == TR.SENTINEL).all()
        outs.append(whole[off:off + n].reshape(s))
    return outs


def abi_layout_cases(dtype):
    """Runs the direct-ABI table on whatever library `xgcm_amd.device._MEM` serves.  Every input view lives in a NaN-filled
    allocation, so a read outside it shows in a result; the contiguous, aligned control of each set of planes is compared
    with the numpy statement, every other layout with that control: kwx, kwy and the results aligned, 16 bytes in and one
    element in (the narrow form), the metrics one element in, with odd row and level pitches, three elements apart,
    transposed and with stride 0.  Under `closed` the closed faces of kwx and kwy hold NaN"""
    import xgcm_amd.device as D

    shape = [2, 4, 7, TR.ABI_NX[dtype]]
    lead, nz, ny, nx = shape
    put = lambda x, st=None, off=ALIGNED: _strided(D, x, st or _contig(x.shape), off)  # noqa: E731
    sixteen = 16 // np.dtype(dtype).itemsize
    A = ALIGNED
    for k in range(2 * len(TR.ABI_PADS)):
        (px, py, pz), to = TR.ABI_PADS[k % len(TR.ABI_PADS)]
        closed = bool((k // len(TR.ABI_PADS)) % 2)
        nf = TR._nf(nz, to)
        fshape = (lead, nf, ny, nx)
        kv = [R.synthetic_field(fshape, 103 + j).astype(dtype) for j in range(2)]
        kv[0].reshape(-1)[5::97] = np.nan
        if closed:
            for x in kv:
                x[:, 0] = np.nan
                if to == "outer":
                    x[:, -1] = np.nan
        nzof = lambda name: nz if name.startswith("mz") else nf  # noqa: E731
        form = lambda name, f: {"z": (1, nzof(name), 1, 1), "p": (1, 1, ny, nx), "v3": (1, nzof(name), ny, nx),  # noqa: E731
                                "vl": (lead, nzof(name), ny, nx)}[f]
        val = lambda name, f: R.synthetic_metric(form(name, f), 111 + "zpv3vl".index(f) + 7 * NAMES.index(name)).astype(dtype)  # noqa: E731
        kws = [put(x) for x in kv]
        assert kws[0].is_contiguous() and kws[0].data_ptr() % 16 == 0
        for present in ({"mzu": "z"}, {"dyg": "p"}, {"ra": "p"}, {"mzu": "z", "mzv": "z", "dyg": "p", "dxg": "p", "ra": "p"},
                        {"mzu": "v3", "mzv": "vl", "dyg": "v3", "dxg": "vl", "ra": "v3"}, {"mzu": "p", "mzv": "p", "dyg": "z", "dxg": "z", "ra": "vl"}, {}):
            pv = {n: val(n, f) for n, f in present.items()}
            aligned = {n: put(x) for n, x in pv.items()}
            control = _abi_call(D, dtype, shape, kws, aligned, k)
            want = _want(kv[0], kv[1], (px, py, pz), to, closed, FILL, *[pv.get(n) for n in NAMES])
            for g, w in zip(control, want):
                assert g.dtype == w.dtype == np.dtype(dtype)
                _same_bits(g, w)
            assert np.isnan(want[0]).any() and np.isnan(want[0]).mean() < 0.2 and all((w[np.isfinite(w)] != 0).mean() > 0.5 for w in want)
            views = [([put(kv[0], off=1), kws[1]], aligned, A), ([kws[0], put(kv[1], off=1)], aligned, A),
                     ([put(x, off=sixteen) for x in kv], aligned, sixteen)]
            assert views[0][0][0].data_ptr() % 16 == np.dtype(dtype).itemsize
            views += [(kws, aligned, off) for off in (0, sixteen, 1)]
            views.append((kws, {n: put(x, off=1) for n, x in pv.items()}, A))
            pitched = {}
            for n, x in pv.items():
                s = list(x.shape)
                pitched[n] = put(x, _contig(s[:-1] + [s[-1] + 1]) if s[-1] > 1 else _contig(s))
            views.append((kws, pitched, A))
            for n, f in present.items():
                x = pv[n]
                if f in ("v3", "vl"):
                    st = [(x.shape[1] * (ny * nx + 1)) * (x.shape[0] > 1), ny * nx + 1, nx, 1]
                    views.append((kws, dict(aligned, **{n: put(x, [s or 1 for s in st])}), A))
                if f == "z":   # the Z-only metric three elements apart
                    views.append((kws, dict(aligned, **{n: put(x, [3 * x.shape[1], 3, 1, 1], 1)}), A))
                if f == "p":   # the plane stored (X, Y): a transposed view
                    t = put(np.ascontiguousarray(x.transpose(0, 1, 3, 2))).permute(0, 1, 3, 2)
                    assert t.stride(-1) == ny and t.stride(-2) == 1
                    views.append((kws, dict(aligned, **{n: t}), A))
            for kws_, planes, off in views:
                for g, w in zip(_abi_call(D, dtype, shape, kws_, planes, k, off), control):
                    _same_bits(g, w)
        # stride-0 metrics along X and Y: one value per level, expanded over the whole volume, equal the Z-only metrics
        flat = {n: put(val(n, "z")).expand(1, nzof(n), ny, nx) for n in NAMES}
        assert all(m.stride(-1) == 0 and m.stride(-2) == 0 for m in flat.values())
        full = {n: put(np.ascontiguousarray(np.broadcast_to(val(n, "z"), (1, nzof(n), ny, nx)))) for n in NAMES}
        for g, w in zip(_abi_call(D, dtype, shape, kws, flat, k), _abi_call(D, dtype, shape, kws, full, k)):
            _same_bits(g, w)
    assert nx % TR.NVS[dtype] == 0 and {to for _, to in TR.ABI_PADS} == set(TOS)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_abi_layouts(host_abi, dtype):
    abi_layout_cases(dtype)


def abi_bad_calls():
    """bad calls return the family's codes, write nothing and leave the process alone; runs on whatever library `_MEM`
    serves"""
    import xgcm_amd.device as D

    lib = D._MEM.lib()
    shape = [2, 3, 4]
    kw = torch.ones([3, 3, 4], dtype=torch.float64, device=D._MEM.device)          # room for Z:outer
    outs = [torch.full([3, 3, 4], TR.SENTINEL, dtype=torch.float64, device=D._MEM.device) for _ in range(3)]
    P = lambda x: None if x is None else x.data_ptr()  # noqa: E731

    def call(code=TR.CODE[np.float64], kwx=kw, kwy=kw, o=outs, shape=shape, ndim=3, outer=0, closed=1, bcx=_hip.BC["periodic"],
             bcy=_hip.BC["extend"], bcz=_hip.BC["fill"], mets=(None,) * 5, strides=(None,) * 5):
        margs = [x for pair in zip(mets, strides) for x in pair]
        return getattr(lib, "xg_bolus_velocity")(code, P(kwx), P(kwy), *margs, *[P(x) for x in o], None if shape is None else _hip.i64(shape),
                                     ndim, outer, closed, bcx, 0.0, bcy, 0.0, bcz, 0.0, D._stream())

    untouched = lambda: all(bool((x == TR.SENTINEL).all()) for x in outs)  # noqa: E731
    for code in (-1, _hip.DTYPE["float16"], _hip.DTYPE["int64"], _hip.DTYPE["int32"], 12, 99):
        assert call(code=code) == -1                              # any other element type: XG_ERR_INVALID
    assert call(kwx=None) == -1 and call(kwy=None) == -1 and call(shape=None) == -1          # NULL arguments
    for k in range(3):
        assert call(o=[None if j == k else x for j, x in enumerate(outs)]) == -1    # a NULL result, each of the three
    assert call(closed=2) == -1 and call(closed=-1) == -1         # the closing flag
    assert call(bcx=7) == -1 and call(bcy=-1) == -1 and call(bcz=9) == -1 and call(bcx=0) == -1 and call(bcx=_hip.BC["halo"]) == -1
    assert call(outer=2) == -1 and call(outer=-1) == -1           # unknown face position
    assert call(shape=[0, 3, 4]) == -1                            # nz = 0: no level
    for k in range(5):                                            # a metric without strides, each of the five
        assert call(mets=tuple(kw.data_ptr() if j == k else None for j in range(5))) == -1
    assert call(ndim=2) < 0 and call(ndim=2) != -1                # XG_ERR_UNSUPPORTED
    assert untouched()
    assert call(shape=[2, 0, 4]) == 0 and call(shape=[2, 3, 0]) == 0 and untouched()   # an empty plane: nothing to do
    assert call() == 0 and call(bcz=_hip.BC["periodic"], outer=1, closed=0) == 0
    assert not any(bool((x[:2] == TR.SENTINEL).any()) for x in outs)


def test_abi_refuses_bad_calls(host_abi):
    abi_bad_calls()


def test_empty_results_return_without_a_launch(host_abi, monkeypatch):
    import xgcm_amd.device as D

    monkeypatch.setattr(D, "_check", lambda rc: pytest.fail("the library was called for an empty result"))
    for shape in ((2, 3, 0, 4), (0, 3, 5, 4), (3, 5, 0)):
        fshape = shape[:-3] + (shape[-3] + 1,) + shape[-2:]
        ub, vb, wb = D.bolus_velocity(np.zeros(fshape), np.zeros(fshape), None, None, None, None, None, True, True, "periodic", "fill", "extend")
        assert tuple(ub.shape) == tuple(vb.shape) == shape and tuple(wb.shape) == fshape and ub.numel() == 0


def test_the_device_wrapper_refuses_fields_of_different_shapes_and_no_level(host_abi):
    import xgcm_amd.device as D

    with pytest.raises(ValueError, match="kwx and kwy must have the same shape"):
        D.bolus_velocity(np.zeros((4, 4, 6)), np.zeros((3, 4, 6)), None, None, None, None, None, True, True, "periodic", "fill", "extend")
    with pytest.raises(ValueError, match="a level along Z"):
        D.bolus_velocity(np.zeros((1, 4, 6)), np.zeros((1, 4, 6)), None, None, None, None, None, True, True, "periodic", "fill", "extend")
    with pytest.raises(ValueError, match="a level along Z"):
        D.bolus_velocity(np.zeros((4, 6)), np.zeros((4, 6)), None, None, None, None, None, False, True, "periodic", "fill", "extend")


def test_the_second_header_its_table_and_both_libraries_agree():
    """include/xgcm_hip.h declares xg_bolus_velocity, `_hip.SIGNATURES` binds it parameter by parameter as the header has
    it, its row is `_hip.FUSED`'s and names its slots as the header names the parameters, and both builds export it"""
    import ctypes as C
    import os

    import test_fused_marshalling as TM

    protos = {"xg_bolus_velocity": TM.PROTOS["xg_bolus_velocity"]}
    assert set(protos) <= set(_hip.SIGNATURES) and set(protos) <= set(_hip.FUSED)
    scalars = {"int": C.c_int, "double": C.c_double}
    for name, (ret, params) in protos.items():
        res, args = _hip.SIGNATURES[name]
        assert ret == "int" and res is C.c_int and len(args) == len(params)
        for (ctype, pname), a in zip(params, args):
            if ctype.endswith("*"):
                assert a is C.c_void_p or (ctype == "int64_t*" and a._type_ is C.c_int64), (name, pname)
            else:
                assert a is scalars[ctype], (name, pname)
        row = _hip.FUSED[name]
        assert _hip.forms(name) == [(name, False)] and TM._slot_names(row, False) == [pname for _, pname in params]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for lib in ("libxgcm_hip.so", "libxgcm_host.so"):
        assert hasattr(C.CDLL(os.path.join(root, "xgcm_amd", lib)), "xg_bolus_velocity")
    assert _hip.load().xg_bolus_velocity.argtypes == _hip.SIGNATURES["xg_bolus_velocity"][1]


def test_argument_order_through_the_recording_library(monkeypatch):
    """every argument of one call reaches the parameter of its name; `shape` is the LEVELS' shape, the fields and wb have
    the faces'"""
    import test_fused_marshalling as TM
    import xgcm_amd.device as D

    mem = TM.RecordingMemory()
    monkeypatch.setattr(D, "_MEM", mem)
    fshape, shape = (2, 4, 3, 4), (2, 3, 3, 4)
    kwx, kwy = TM._field(torch.float64, fshape), TM._field(torch.float64, fshape) + 1
    mets = {"mzu": TM._field(torch.float64, (1, 3, 3, 4)), "mzv": TM._field(torch.float64, (2, 1, 3, 4)), "dyG": TM._field(torch.float64, (2, 4, 1, 4)),
            "dxG": TM._field(torch.float64, (2, 4, 3, 1)), "rA": TM._field(torch.float64, (1, 1, 3, 4))}
    ub, vb, wb = D.bolus_velocity(kwx, kwy, *mets.values(), True, False, "periodic", "fill", "extend", 1.5, -0.0, 2.5)
    assert tuple(ub.shape) == tuple(vb.shape) == shape and tuple(wb.shape) == fshape
    expected = dict(dtype=_hip.DTYPE["float64"], kwx=kwx.data_ptr(), kwy=kwy.data_ptr(), out_u=ub.data_ptr(), out_v=vb.data_ptr(),
                    out_w=wb.data_ptr(), shape=shape, ndim=4, outer=1, closed=0, bc_x=_hip.BC["periodic"], fill_x=1.5,
                    bc_y=_hip.BC["fill"], fill_y=-0.0, bc_z=_hip.BC["extend"], fill_z=2.5, stream=TM.STREAM)
    for n, m in mets.items():
        expected[n] = m.data_ptr()
        expected[n + "_strides"] = tuple(0 if s == 1 else st for s, st in zip(m.shape, m.stride()))
    TM._check_call(mem.recorder, "xg_bolus_velocity", expected)


# ---- 9. the tunable call table, between guard bands ------------------------------------------------------------------------
def tunable_calls(D, dtype):
    """(calls, references) of the K7t tunable sweep: name -> thunk that calls `D` on inputs uploaded once, name -> thunk that
    gives numpy's results of the same call.  Both face positions, both closings; planes with a profile, volumes, and no
    metric.  Under `closed` the closed faces of kwx and kwy hold NaN"""
    f = lambda shape, seed: R.synthetic_field(shape, seed).astype(dtype)  # noqa: E731
    m = lambda shape, seed: R.synthetic_metric(shape, seed).astype(dtype)  # noqa: E731
    calls, references = {}, {}
    for n, shape in enumerate(((4, 40, 264), (3, 33, 131))):
        nz, ny, nx = shape
        for k, (to, pads) in enumerate((("left", ("periodic", "extend", "fill")), ("outer", ("extend", "fill", "periodic")),
                                        ("left", ("fill", "periodic", "periodic")), ("outer", ("periodic", "periodic", "fill")))):
            nf = nz + (to == "outer")
            closed = bool((n + k // 2) % 2)
            kws = [f((nf, ny, nx), 160 + 2 * k + j) for j in range(2)]
            kws[0][1, 7, 9] = kws[1][0 if not closed else 1, 0, 0] = kws[1][nf - 2, ny - 1, nx - 1] = np.nan
            if closed:
                for x in kws:
                    x[0] = np.nan
                    if to == "outer":
                        x[-1] = np.nan
            if k % 2:
                mets = [m((nz, 1, 1), 172), m((nz, 1, 1), 172), m((1, ny, nx), 170), m((1, ny, nx), 171), m((1, ny, nx), 173)]
            else:
                mets = [m((nz, ny, nx), 174), m((nz, ny, nx), 175), m((nf, ny, nx), 176), m((nf, ny, nx), 177), m((nf, ny, nx), 178)]
            if k == 2:
                mets = [None] * 5
            dk = tuple(D.asdevice(x) for x in kws)
            dm = tuple(None if x is None else D.asdevice(x) for x in mets)
            key = f"{nx}{to}{pads[2]}{'closed' if closed else 'open'}"
            fill = [FILL[x] for x in "XYZ"]
            calls[key] = lambda dk=dk, dm=dm, to=to, closed=closed, pads=pads: D.bolus_velocity(*dk, *dm, to == "outer", closed, *pads, *fill)
            references[key] = lambda kws=kws, mets=mets, to=to, closed=closed, pads=pads: _want(*kws, pads, to, closed, FILL, *mets)
    return calls, references


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_the_tunable_call_table_equals_its_numpy_references(host_abi, dtype):
    """the thunks the GPU suite sweeps over every tunable value, once through the host build (which reads no tunable)"""
    import xgcm_amd.device as D

    calls, references = tunable_calls(D, dtype)
    assert len(calls) == 8 and set(calls) == set(references)
    assert {k[-6:] == "closed" for k in calls} == {True, False}
    for name, thunk in calls.items():
        for g, want in zip(thunk(), references[name]()):
            got = D.tohost(g)
            assert got.dtype == np.dtype(dtype) and np.isnan(want).any() and np.isnan(want).mean() < 0.01, name
            assert (want[np.isfinite(want)] != 0).mean() > 0.5, name
            assert _bits_equal(got, want), name


def guarded_table(D, monkeypatch, dtype, offset, same_bits):
    """the table built and run between guard bands: a store outside any of the three results, a cell left unwritten and a
    result-changing read outside kwx, kwy or a metric (bands of NaN) all fail; returns the number of results checked"""
    checked = 0
    with GM.guarded(D, monkeypatch, offset) as g:
        calls, references = tunable_calls(D, dtype)
        assert g.placed >= 8 * 2 + 6 * 5        # kwx and kwy of every call, the metrics of the six that have them
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
        assert guarded_table(D, monkeypatch, dtype, offset, _bits_equal) == 24
