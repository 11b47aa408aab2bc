"""Implicit vertical viscosity of a C-grid velocity, `Grid.implicit_vertical_viscosity`: (u, v) mixed by one centre-point nu, on CPU.

`statement` below is the specification: nu padded left of column 0 / below row 0, `(left + nu) * 0.5` in the dtype, then
`test_implicit_vertical_diffusion.statement` per component.  The one-pass path (through the `host_abi` fixture: the product's
`xgcm_amd.device` over libxgcm_host.so) and the chain it replaces

    nu_u = grid.interp(nu, X);  nu_v = grid.interp(nu, Y)
    xu = grid.implicit_vertical_diffusion(u, nu_u, dt);  xv = grid.implicit_vertical_diffusion(v, nu_v, dt)

are compared with it bit for bit (NaN = NaN, -0.0 is not +0.0).  A counter on `device.implicit_vertical_viscosity` shows that
every case meant for the one pass reached it.  The tables, the NaN cases, the direct-ABI cases and the guarded table are
shared with the GPU suite."""

import itertools
import warnings

import numpy as np
import pytest
import torch

import guarded_memory as GM
import test_implicit_vertical_diffusion as TI
import test_vertical_diffusion as TD
from oracle import refimpl as R
from test_fused_layouts import ALIGNED, _contig, _strided
from xgcm_amd import DataArray, Dataset, Grid, _hip
from xgcm_amd.chunked import BlockArray

BCS = ["periodic", "fill", "extend"]
PAIRS = list(itertools.product(BCS, BCS))    # (X pad, Y pad)
TOS = ["left", "outer"]
DTYPES = [np.float64, np.float32]
FILLS = [0.375, -0.0, float("nan")]
MFORMS = ["1d", "full", "lead", None]        # None: no metric enters (`metric_weighted=False`)
AXES = TD.AXES
ZDIM = TD.ZDIM
U_AT, V_AT, C_AT = ("YC", "XG"), ("YG", "XC"), ("YC", "XC")
DT, DT_PLAIN = TI.DT, TI.DT_PLAIN            # the coupling dt * nu / (mf * mc) stays below 36 either way
_same_bits = TD._same_bits
_same_labelled = TD._same_labelled
_nf = TD._nf


# ---- the definition -------------------------------------------------------------------------------------------------------
def _mean_with_the_neighbour(nu, axis, bc, fv):
    """(left + nu) * 0.5 along `axis` in nu's dtype; `left` is nu one cell down the axis, padded in front of cell 0"""
    T = nu.dtype.type
    n = nu.shape[axis]
    if bc == "fill":
        shape = list(nu.shape)
        shape[axis] = 1
        pad = np.full(shape, T(fv), nu.dtype)   # the cast keeps a -0.0 and a NaN
    else:
        pad = np.take(nu, [n - 1 if bc == "periodic" else 0], axis)
    left = np.concatenate([pad, np.take(nu, np.arange(n - 1), axis)], axis)
    with np.errstate(all="ignore"):
        return (left + nu) * T(0.5)


def statement(u, v, nu, mfu, mcu, mfv, mcv, to, bcx, fvx, bcy, fvy, dt):
    """(xu, xv).  u, v (.., n, ny, nx); nu (.., n | n + 1, ny, nx) at the faces of `to`, dims of extent 1 broadcast;
    the metrics broadcast against the flux (mfu, mfv) and the field (mcu, mcv) or are None."""
    assert nu.shape[-3] in (1, u.shape[-3] + (to == "outer")) and u.shape == v.shape   # (1: the same plane at every face)
    return (TI.statement(u, _mean_with_the_neighbour(nu, -1, bcx, fvx), mfu, mcu, dt),
            TI.statement(v, _mean_with_the_neighbour(nu, -2, bcy, fvy), mfv, mcv, dt))


# ---- grids, fields, nu ------------------------------------------------------------------------------------------------------
ZS = (("F", "ZC", 0), ("Cl", "ZL", 0), ("Co", "ZO", 1))   # the Z metric at the centre, the left and the outer position


def _grid(lead, nz, ny, nx, dtype, bcx="periodic", bcy="extend", metric="1d", axes=AXES, mdtype=None, bcz="extend"):
    """C-grid with a Z axis that has a left and an outer position.  Z metrics: "1d" -- drF(ZC), drCl(ZL), drCo(ZO); "full" --
    thicknesses (Z, Y, X) at u's AND at v's points for all three Z positions (hFu, hFv, hClu, ..); "lead": the same with the
    first leading dim in front; None: no Z metric at all"""
    dims = ("time", "member")[:len(lead)]
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0),
              "YC": ("YC", np.arange(ny) + 0.5), "YG": ("YG", np.arange(ny) * 1.0),
              "ZC": ("ZC", np.arange(nz) + 0.5), "ZL": ("ZL", np.arange(nz) * 1.0), "ZO": ("ZO", np.arange(nz + 1) * 1.0)}
    for d, n in zip(dims, lead):
        coords[d] = (d, np.arange(n) * 2.0)
    m = lambda shape, seed: R.synthetic_metric(shape, seed).astype(mdtype or dtype)  # noqa: E731
    data = {}
    if metric == "1d":
        for k, (name, zd, more) in enumerate(ZS):
            data["dr" + name] = ((zd,), m((nz + more,), 63 + k))
    elif metric is not None:
        pl, pd = ((lead[0],), dims[:1]) if metric == "lead" and lead else ((), ())
        for k, (name, zd, more) in enumerate(ZS):
            for j, (c, at) in enumerate((("u", U_AT), ("v", V_AT))):
                data["h" + name + c] = (pd + (zd,) + at, m(pl + (nz + more, ny, nx), 66 + 2 * k + j))
    ds = Dataset(data, coords)
    padding = {"X": bcx, "Y": bcy, "Z": bcz}
    grid = Grid(ds, coords=axes, metrics={("Z",): list(data)} if data else {},
                padding={k: p for k, p in padding.items() if p is not None}, autoparse_metadata=False)
    return grid, ds, dims


def _fields(lead, nz, ny, nx, dtype, dims, nan=False, seed=71):
    """(u, v) at their C-grid points"""
    shape = tuple(lead) + (nz, ny, nx)
    u, v = (R.synthetic_field(shape, seed + k).astype(dtype) for k in range(2))
    if nan:
        u.reshape(-1)[5::13] = np.nan
        v[..., :, ny // 2, nx // 2] = np.nan     # a whole column
        v[..., 0, 0, 0] = np.nan
        u[..., nz - 1, ny - 1, nx - 1] = np.nan
    return DataArray(u, dims + ("ZC",) + U_AT, name="u"), DataArray(v, dims + ("ZC",) + V_AT, name="v")


def _nu(form, lead, nz, ny, nx, dtype, dims, to, seed=75):
    """nu at (Zf, YC, XC) with values in [0, 1e4] and exact zeros among them: "3d" -- no leading dim, so it is broadcast over
    all of them; "lead" -- the first leading dim in front, broadcast over the others"""
    pl, pd = ((lead[0],), dims[:1]) if form == "lead" and lead else ((), ())
    v = np.abs(R.synthetic_field(pl + (_nf(nz, to), ny, nx), seed).astype(np.float64)) * 2e4
    v[v < 2e3] = 0.0
    return DataArray(v.astype(dtype), pd + (ZDIM[to],) + C_AT, name="nu")


def _metrics_of(ds, u, v, to, weighted):
    """(mfu, mcu, mfv, mcv) as numpy arrays that broadcast against the flux / the field, from the dataset's own arrays"""
    if not weighted:
        return (None,) * 4
    face = {"left": "Cl", "outer": "Co"}[to]
    out = []
    for f, c in ((u, "u"), (v, "v")):
        f_dims = f.dims[:-3] + (ZDIM[to],) + f.dims[-2:]
        names = ("dr" + face, "drF") if "drF" in ds else ("h" + face + c, "hF" + c)
        out += [TD._aligned(ds[names[0]], f_dims), TD._aligned(ds[names[1]], f.dims)]
    return tuple(out)


def _fv(fill_value, axis):
    return 0.0 if fill_value is None or fill_value.get(axis) is None else fill_value[axis]


def _want_of(grid, ds, u, v, nu, kw):
    """`statement` for labelled inputs and the keyword arguments of one call"""
    to = kw.get("to") or ("outer" if "outer" in grid.axes["Z"].coords else "left")
    bc = dict({ax: grid.axes[ax]._padding for ax in "XY"}, **(kw.get("padding") or {}))
    nu_dims = u.dims[:-3] + (ZDIM[to],) + C_AT
    return statement(np.asarray(u.values), np.asarray(v.values), TD._aligned(nu, nu_dims),
                     *_metrics_of(ds, u, v, to, kw.get("metric_weighted", True)), to, bc["X"], _fv(kw.get("fill_value"), "X"),
                     bc["Y"], _fv(kw.get("fill_value"), "Y"), kw["dt"])


def _chain(grid, u, v, nu, dt=None, x_axis="X", y_axis="Y", z_axis="Z", to=None, padding=None, fill_value=None,
           metric_weighted=True):
    """the four calls the one pass replaces"""
    kw = dict(padding=padding, fill_value=fill_value)
    nu_u = grid.interp(nu, x_axis, **kw)
    nu_v = grid.interp(nu, y_axis, **kw)
    xu = grid.implicit_vertical_diffusion(u, nu_u, dt, z_axis=z_axis, to=to, metric_weighted=metric_weighted)
    xv = grid.implicit_vertical_diffusion(v, nu_v, dt, z_axis=z_axis, to=to, metric_weighted=metric_weighted)
    return xu, xv


def _counted(monkeypatch):
    import xgcm_amd.device as D

    calls = []
    real = D.implicit_vertical_viscosity
    monkeypatch.setattr(D, "implicit_vertical_viscosity", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def _no_fused(monkeypatch):
    import xgcm_amd.device as D

    monkeypatch.setattr(D, "implicit_vertical_viscosity", lambda *a, **k: pytest.fail("one-pass entry called"))


def test_the_statement_is_the_padded_mean_then_the_solve():
    """written out by hand for one row, so that the helper above cannot hide a wrong pad"""
    nu = np.arange(1.0, 9.0).reshape(2, 1, 4)    # (faces, ny = 1, nx = 4)
    for bc, first in (("periodic", (4.0 + 1.0) * 0.5), ("extend", 1.0), ("fill", (0.375 + 1.0) * 0.5)):
        mean = _mean_with_the_neighbour(nu, -1, bc, 0.375)
        assert mean[0, 0].tolist() == [first, 1.5, 2.5, 3.5]
    # one row: every Y pad lands on the only cell
    assert np.array_equal(_mean_with_the_neighbour(nu, -2, "periodic", 9.0), nu)
    assert np.array_equal(_mean_with_the_neighbour(nu, -2, "extend", 9.0), nu)
    assert np.signbit(_mean_with_the_neighbour(np.full((1, 1, 1), -0.0), -1, "fill", -0.0)).all()
    assert not np.signbit(_mean_with_the_neighbour(np.full((1, 1, 1), -0.0), -1, "fill", 0.0)).any()


# ---- 2. bit for bit at the smallest shapes that can go wrong --------------------------------------------------------------
NZS, NYS, NXS = [1, 2, 3, 5], [1, 2, 3, 9], [1, 2, 3, 8, 129, 130, 257]
LEADS = [(), (2,), (2, 2)]


def shape_table(nx):
    """(lead, nz, ny, nx, to, dtype, metric form, nu form, (X pad, Y pad), (X fill, Y fill)): every nz and ny with this nx --
    one level, one row, one column (every pad lands on the only cell), nx across one float64 x-tile of 128 columns and one
    float32 tile of 256, the narrow form (nx no multiple of the lane vector), a ragged last 2-row segment.  Case number k of
    the whole table picks combination (27 k + 5) mod 16 of (to, dtype, metric form), pad pair k mod 9 -- `to` alternates with
    k, so 18 consecutive cases meet all nine pairs at both positions -- and the fills rotate with k // 9.  A metric with a
    leading dim gets one; nu has the first leading dim or none, so it is broadcast over at least one."""
    out = []
    for n, (nz, ny) in enumerate(itertools.product(NZS, NYS)):
        k = n + len(NZS) * len(NYS) * NXS.index(nx)
        c = (27 * k + 5) % 16
        to, dtype, mform = TOS[c % 2], DTYPES[(c // 2) % 2], MFORMS[c // 4]
        lead = LEADS[1 + k % 2] if mform == "lead" else LEADS[k % 3]
        nuform = "lead" if (k // 3) % 2 else "3d"
        out.append((lead, nz, ny, nx, to, dtype, mform, nuform, PAIRS[k % 9], (FILLS[(k // 9) % 3], FILLS[(k // 9 + 1) % 3])))
    return out


def case_of(lead, nz, ny, nx, to, dtype, mform, nuform, pads, fills, nan=False, dt=None, seed=71, plain_metric="1d"):
    """(grid, (u, v, nu), kwargs, ds) of one row; the pads are the grid's own, the fills go with the call"""
    grid, ds, dims = _grid(lead, nz, ny, nx, dtype, *pads, metric=mform or plain_metric)
    u, v = _fields(lead, nz, ny, nx, dtype, dims, nan=nan, seed=seed)
    nu = _nu(nuform, lead, nz, ny, nx, dtype, dims, to, seed=seed + 4)
    kw = dict(dt=(DT if mform else DT_PLAIN) if dt is None else dt, to=to, metric_weighted=mform is not None,
              fill_value={"X": fills[0], "Y": fills[1]})
    return grid, (u, v, nu), kw, ds


def shape_cases(nx):
    """the table's cases; those without a metric alternate between a grid that has Z metrics and one that has none"""
    return [case_of(*row, nan=(row[1] + row[2]) % 4 == 0, plain_metric=(None, "1d")[n % 2]) for n, row in enumerate(shape_table(nx))]


def test_the_shape_table_meets_every_combination():
    rows = [r for nx in NXS for r in shape_table(nx)]
    assert {(r[4], np.dtype(r[5]).name, r[6]) for r in rows} == set(itertools.product(TOS, ("float64", "float32"), MFORMS))
    assert {(r[4], r[8]) for r in rows} == set(itertools.product(TOS, PAIRS))
    assert all(a != b for a, b in PAIRS if (a, b) not in list(zip(BCS, BCS))) and sum(a != b for a, b in PAIRS) == 6
    for axis in (0, 1):   # every fill value under a `fill` pad on either axis; NaN and -0.0 compare by their bits
        assert {np.float64(r[9][axis]).tobytes() for r in rows if r[8][axis] == "fill"} == {np.float64(f).tobytes() for f in FILLS}
    assert {r[0] for r in rows} == set(LEADS) and {r[7] for r in rows} == {"3d", "lead"}
    assert any(r[0] == (2, 2) and r[7] == "lead" for r in rows) and any(r[0] and r[7] == "3d" for r in rows)
    assert {r[1:4] for r in rows} == set(itertools.product(NZS, NYS, NXS))


def run_cases(monkeypatch, cases):
    calls = _counted(monkeypatch)
    for n, (grid, (u, v, nu), kw, ds) in enumerate(cases):
        try:
            xu, xv = grid.implicit_vertical_viscosity(u, v, nu, **kw)
            assert len(calls) == n + 1   # the one-pass entry served it
            wu, wv = _want_of(grid, ds, u, v, nu, kw)
            for got, field, want in ((xu, u, wu), (xv, v, wv)):
                assert got.dims == field.dims and got.name == field.name and list(got.coords) == list(field.coords)
                _same_bits(got.values, want)
        except AssertionError as err:
            raise AssertionError(f"case {n}: {u.shape} {np.dtype(u.values.dtype)} nu {nu.dims} pads {[grid.axes[ax]._padding for ax in 'XY']} {kw}") from err


@pytest.mark.parametrize("nx", NXS)
def test_small_shapes(host_abi, monkeypatch, nx):
    cases = shape_cases(nx)
    assert len(cases) == len(NZS) * len(NYS)
    run_cases(monkeypatch, cases)


# ---- 3. the chain -----------------------------------------------------------------------------------------------------------
# (lead, nz, ny, nx, metric form, nu form): the leading dims, metric and nu forms of the pad matrix
MATRIX = [((), 4, 5, 8, "1d", "3d"), ((2,), 3, 5, 6, "full", "lead"), ((2, 2), 3, 4, 5, "lead", "lead"), ((3,), 5, 3, 12, None, "3d"),
          ((2,), 1, 2, 4, "1d", "3d"), ((), 2, 1, 1, "full", "3d")]


def matrix_cases(pads, dtype):
    out = []
    for n, (lead, nz, ny, nx, mform, nuform) in enumerate(MATRIX):
        for to in TOS:
            out.append(case_of(lead, nz, ny, nx, to, dtype, mform, nuform, pads, (FILLS[n % 3], FILLS[(n + 1 + (to == "left")) % 3]),
                               nan=n % 2 == 1))
    return out


def compare_with_chain(monkeypatch, cases):
    """every one-pass call (counted), then the chain through the same Grid with the entry barred; values and labels"""
    calls = _counted(monkeypatch)
    got = [grid.implicit_vertical_viscosity(*f, **kw) for grid, f, kw, _ in cases]
    assert len(calls) == len(cases)
    _no_fused(monkeypatch)
    for (grid, f, kw, _), g in zip(cases, got):
        for one, other in zip(g, _chain(grid, *f, **kw)):
            _same_labelled(one, other)
            _same_bits(one.values, other.values)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("pads", PAIRS, ids=["-".join(p) for p in PAIRS])
def test_equals_the_chain_and_the_statement(host_abi, monkeypatch, pads, dtype):
    cases = matrix_cases(pads, dtype)
    run_cases(monkeypatch, cases)
    compare_with_chain(monkeypatch, cases)


def _case(pads=("periodic", "extend"), lead=(2,), nz=4, ny=5, nx=6, dtype=np.float64, to="outer", mform="1d", nuform="3d", **gk):
    grid, ds, dims = _grid(lead, nz, ny, nx, dtype, *pads, metric=mform, **gk)
    u, v = _fields(lead, nz, ny, nx, dtype, dims)
    return grid, ds, (u, v, _nu(nuform, lead, nz, ny, nx, dtype, dims, to))


def test_nu_with_its_dims_in_another_order_is_read_in_place(host_abi, monkeypatch):
    grid, ds, (u, v, nu) = _case(lead=(2, 2), nuform="lead", to="left")
    kw = dict(dt=DT, to="left")
    calls = _counted(monkeypatch)
    turned = nu.transpose("XC", "ZL", "time", "YC")
    xu, xv = grid.implicit_vertical_viscosity(u, v, turned, **kw)
    assert len(calls) == 1
    for got, want in zip((xu, xv), _want_of(grid, ds, u, v, nu, kw)):
        _same_bits(got.values, want)
    _no_fused(monkeypatch)
    for got, other in zip((xu, xv), _chain(grid, u, v, turned, **kw)):
        _same_labelled(got, other)


def test_coords_names_and_attrs_are_the_fields(host_abi, monkeypatch):
    grid, ds, (u, v, nu) = _case()
    u = DataArray(u.values, u.dims, name="u", attrs={"units": "m/s"}).assign_coords({"lon": (("YC", "XG"), np.ones((5, 6))),
                                                                                       "t2": (("time",), np.arange(2) + 7.0)})
    v = v._replace(name=None).assign_coords({"depth": (("ZC",), np.arange(4) * 10.0)})
    nu = nu.assign_coords({"depth_f": (("ZO",), np.arange(5) * 10.0)})
    calls = _counted(monkeypatch)
    xu, xv = grid.implicit_vertical_viscosity(u, v, nu, dt=DT)
    assert len(calls) == 1 and xu.attrs == {"units": "m/s"} and xv.name is None and "lon" in xu.coords and "depth" in xv.coords
    wu, wv = _want_of(grid, ds, u, v, nu, dict(dt=DT))
    _same_labelled(xu, u._replace(data=wu))
    _same_labelled(xv, v._replace(data=wv))
    _no_fused(monkeypatch)
    for got, other in zip((xu, xv), _chain(grid, u, v, nu, dt=DT)):
        _same_labelled(got, other)


def test_xarray_in_xarray_out(host_abi, monkeypatch):
    import xarray_standin

    xarray_standin.install(monkeypatch)
    import xarray as xr

    grid, ds, (u, v, nu) = _case(lead=())
    calls = _counted(monkeypatch)
    got = grid.implicit_vertical_viscosity(*(xr.DataArray(x.values, dims=x.dims, name=x.name) for x in (u, v, nu)), dt=DT)
    assert len(calls) == 1
    for g, f, want in zip(got, (u, v), _want_of(grid, ds, u, v, nu, dict(dt=DT))):
        assert type(g).__module__.split(".")[0] == "xarray" and tuple(g.dims) == f.dims and g.name == f.name
        _same_bits(np.asarray(g.values), want)


def test_to_defaults_to_outer_when_the_axis_has_it_else_left(host_abi, monkeypatch):
    calls = _counted(monkeypatch)
    grid, ds, (u, v, nu) = _case()
    for got, want in zip(grid.implicit_vertical_viscosity(u, v, nu, dt=DT), _want_of(grid, ds, u, v, nu, dict(dt=DT, to="outer"))):
        _same_bits(got.values, want)
    axes = dict(AXES, Z={"center": "ZC", "left": "ZL"})
    g2, ds2, dims = _grid((2,), 4, 5, 6, np.float64, axes=axes, metric=None)
    nl = _nu("3d", (2,), 4, 5, 6, np.float64, dims, "left")
    kw = dict(dt=DT_PLAIN, metric_weighted=False)
    for got, want in zip(g2.implicit_vertical_viscosity(u, v, nl, **kw), _want_of(g2, ds2, u, v, nl, kw)):
        _same_bits(got.values, want)
    assert len(calls) == 2


def test_the_fused_entry_runs_alone(host_abi, monkeypatch):
    """one call of the one-pass device entry and none of the operators of the chain"""
    import xgcm_amd.device as D

    grid, ds, (u, v, nu) = _case()
    calls = {"fused": 0, "other": 0}

    def counted(fn, key):
        def wrapped(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(D, "implicit_vertical_viscosity", counted(D.implicit_vertical_viscosity, "fused"))
    for name in ("binary", "stencil1d", "implicit_vertical_diffusion"):
        monkeypatch.setattr(D, name, counted(getattr(D, name), "other"))
    grid.implicit_vertical_viscosity(u, v, nu, dt=DT)
    assert calls == {"fused": 1, "other": 0}


# ---- 4. a NaN in nu (device level: shared with the GPU suite) --------------------------------------------------------------
def nan_cases(dtype):
    """one NaN in nu at face k, cell (j, i) makes exactly the columns (j, i) and (j, i+1) of xu and (j, i) and (j+1, i) of xv
    NaN; the neighbour wraps under `periodic` and is absent at the last column / row otherwise; a NaN at face 0 or nz
    changes nothing.  Cells: the corners, beside each pad, the last lane of the first x-tile's vectors and the first of the
    second tile (nx = 130), the middle"""
    import xgcm_amd.device as D

    nz, ny, nx = 4, 5, 130
    f = lambda shape, seed: R.synthetic_field(shape, seed).astype(dtype)  # noqa: E731
    u, v = f((nz, ny, nx), 201), f((nz, ny, nx), 202)
    nu = np.abs(f((nz + 1, ny, nx), 203)) * dtype(2e4)
    mets = [R.synthetic_metric(s, 204 + k).astype(dtype) for k, s in enumerate(((nz + 1, 1, 1), (nz, ny, nx), (nz + 1, ny, nx), (nz, 1, 1)))]
    checked = 0
    for (bcx, bcy), (k, j, i) in itertools.product((("periodic", "extend"), ("fill", "periodic"), ("extend", "fill")),
                                                   ((1, 0, 0), (3, 4, 129), (2, 2, 127), (2, 1, 128), (1, 4, 0), (2, 0, 129),
                                                    (2, 2, 64), (0, 2, 5), (4, 2, 5))):
        bad = nu.copy()
        bad[k, j, i] = np.nan
        xu, xv = (D.tohost(x) for x in D.implicit_vertical_viscosity(u, v, bad, *mets, True, bcx, bcy, DT, 0.375, 0.375))
        mu, mv = np.zeros((ny, nx), bool), np.zeros((ny, nx), bool)
        if 0 < k < nz:   # an interior face
            mu[j, i] = mv[j, i] = True
            if i + 1 < nx or bcx == "periodic":
                mu[j, (i + 1) % nx] = True
            if j + 1 < ny or bcy == "periodic":
                mv[(j + 1) % ny, i] = True
        assert np.array_equal(np.isnan(xu), np.broadcast_to(mu, xu.shape)), (bcx, bcy, k, j, i)
        assert np.array_equal(np.isnan(xv), np.broadcast_to(mv, xv.shape)), (bcx, bcy, k, j, i)
        wu, wv = statement(u, v, bad, *mets, "outer", bcx, 0.375, bcy, 0.375, DT)
        _same_bits(xu, wu)
        _same_bits(xv, wv)
        checked += 1
    return checked


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_a_nan_in_nu_poisons_exactly_the_columns_it_reaches(host_abi, dtype):
    assert nan_cases(dtype) == 27


# ---- 5. the residual property -----------------------------------------------------------------------------------------------
# measured on CPU with the numpy statement on exactly these inputs (printed by the test), relative to max|field|; asserted at
# 16 x the measured value, as SOLVE_MEASURED / PROPERTY_MEASURED in tests/test_implicit_vertical_diffusion.py: the margin is
# for another order of the explicit operator's roundings (it is a chain of three launches), not for a wrong coefficient,
# which gives errors of order 1
RESIDUAL_MEASURED = {np.float64: {"u": 1.335e-15, "v": 1.669e-15}, np.float32: {"u": 7.165e-07, "v": 1.972e-06}}


def property_case(dtype):
    nz, ny, nx = 17, 3, 5
    grid, ds, dims = _grid((), nz, ny, nx, dtype, "periodic", "extend")
    u, v = _fields((), nz, ny, nx, dtype, dims)
    return grid, ds, u, v, _nu("3d", (), nz, ny, nx, dtype, dims, "outer")


def residuals(grid, u, v, nu, xu, xv, values=lambda x: np.asarray(x.values)):
    """max-norm of x - dt * vertical_diffusion(x, interp(nu)) - field relative to the field's, per component"""
    out = {}
    for name, axis, f, x in (("u", "X", u, xu), ("v", "Y", v, xv)):
        back = values(x) - x.values.dtype.type(DT) * values(grid.vertical_diffusion(x, grid.interp(nu, axis), to="outer", padding="extend"))
        out[name] = TI._rel(back, values(f))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_the_explicit_operator_undoes_it(host_abi, dtype):
    """xu - dt * vertical_diffusion(xu, interp(nu, X), to="outer", padding="extend") is u again, and likewise for v"""
    grid, ds, u, v, nu = property_case(dtype)
    wu, wv = _want_of(grid, ds, u, v, nu, dict(dt=DT, to="outer"))
    measured = residuals(grid, u, v, nu, u._replace(data=wu), v._replace(data=wv))
    print(f"{np.dtype(dtype)}: residual of the numpy statement: u {measured['u']:.3e}, v {measured['v']:.3e}")
    xu, xv = grid.implicit_vertical_viscosity(u, v, nu, dt=DT)
    got = residuals(grid, u, v, nu, xu, xv)
    assert not np.array_equal(xu.values, u.values) and not np.array_equal(xv.values, v.values)   # (the solve did mix)
    for c in "uv":
        assert got[c] <= 16 * RESIDUAL_MEASURED[dtype][c], (c, got[c])


# ---- 6. the entry of the C ABI called directly, with views ----------------------------------------------------------------
NVS = {np.float64: 2, np.float32: 4}
TORCH = {np.float64: torch.float64, np.float32: torch.float32}
CODE = {np.float64: _hip.DTYPE["float64"], np.float32: _hip.DTYPE["float32"]}
ABI_NX = {np.float64: 132, np.float32: 264}   # one full 64-lane tile and a partial one
ABI_PADS = [("periodic", "extend", "left"), ("fill", "periodic", "outer"), ("extend", "fill", "outer")]
PLANES = ("nu", "mfu", "mcu", "mfv", "mcv")
SENTINEL = 12345.5


def abi_dt(planes):
    """the coupling stays near 36 whichever of the metrics (1000 .. 2000 each) are there; both components get one dt, so
    the metrics of the two come in the same pattern"""
    return DT * (1.0 if planes.get("mfu") is not None else 1e-3) * (1.0 if planes.get("mcu") is not None else 1e-3)


def _abi_call(D, dtype, shape, u, v, planes, pads, offs=(ALIGNED,) * 4, fills=(0.375, -0.0)):
    """one call of xg_implicit_vertical_viscosity: u, v contiguous views, `planes` {nu, mfu, mcu, mfv, mcv} views (nu always);
    the two workspaces and the two results are written `offs` elements into allocations full of SENTINEL, which must still
    surround all four afterwards.  Returns (xu, xv)."""
    bcx, bcy, to = pads
    fshape = shape[:-3] + [_nf(shape[-3], to)] + shape[-2:]
    args = [CODE[dtype], u.data_ptr(), v.data_ptr()]
    for name in PLANES:
        m, against = planes.get(name), (shape if name.startswith("mc") else fshape)
        if m is None:
            args += [None, None]
        else:
            assert all(n in (1, s) for n, s in zip(m.shape, against))
            args += [m.data_ptr(), _hip.i64([0 if n == 1 else m.stride(d) for d, n in enumerate(m.shape)])]
    n = int(np.prod(shape))
    bufs = [torch.full((off + n + ALIGNED,), SENTINEL, dtype=TORCH[dtype], device=D._MEM.device) for off in offs]
    views = [b[off:off + n] for b, off in zip(bufs, offs)]   # work_u, work_v, out_u, out_v
    args += [x.data_ptr() for x in views] + [_hip.i64(shape), len(shape), int(to == "outer"), _hip.BC[bcx], fills[0], _hip.BC[bcy],
                                            fills[1], abi_dt(planes)]
    D._check(D._MEM.lib().xg_implicit_vertical_viscosity(*args, D._stream()))
    whole = [b.cpu().numpy() for b in bufs]
    for w, off in zip(whole, offs):
        assert (w[:off] == SENTINEL).all() and (w[off + n:] == SENTINEL).all()
    return tuple(w[off:off + n].reshape(shape) for w, off in zip(whole[2:], offs[2:]))


def _equal(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def abi_layout_cases(dtype):
    """Runs the direct-ABI table on whatever library `xgcm_amd.device._MEM` serves.  Every input view lives in a NaN-filled
    allocation, so a read outside it shows in the result; the contiguous, aligned control of each set of planes is compared
    with the statement, every other layout with that control."""
    import xgcm_amd.device as D

    shape = [2, 4, 7, ABI_NX[dtype]]
    lead, nz, ny, nx = shape
    uv, vv = (R.synthetic_field(tuple(shape), 101 + k).astype(dtype) for k in range(2))
    uv.reshape(-1)[5::1700] = np.nan
    put = lambda x, st=None, off=ALIGNED: _strided(D, x, st or _contig(x.shape), off)  # noqa: E731
    for pads in ABI_PADS:
        nf = _nf(nz, pads[2])
        levels = {"nu": nf, "mfu": nf, "mfv": nf, "mcu": nz, "mcv": nz}

        def vals(name, form, seed):
            n = levels[name]
            sh = {"z": (1, n, 1, 1), "p": (1, 1, ny, nx), "v3": (1, n, ny, nx), "vl": (lead, n, ny, nx)}[form]
            if name == "nu":
                return (np.abs(R.synthetic_field(sh, seed)) * 2e4).astype(dtype)
            return R.synthetic_metric(sh, seed).astype(dtype)

        u, v = put(uv), put(vv)
        assert u.is_contiguous() and u.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 0
        for present in ({"nu": "v3"}, {"nu": "vl", "mfu": "z", "mcu": "z", "mfv": "z", "mcv": "z"},
                        {"nu": "v3", "mfu": "vl", "mcu": "v3", "mfv": "v3", "mcv": "p"}, {"nu": "p", "mcu": "vl", "mcv": "v3"}):
            pv = {n: vals(n, form, 111 + i) for i, (n, form) in enumerate(present.items())}
            aligned = {n: put(x) for n, x in pv.items()}
            control = _abi_call(D, dtype, shape, u, v, aligned, pads)
            want = statement(uv, vv, *(pv.get(n) for n in PLANES), pads[2], pads[0], 0.375, pads[1], -0.0, abi_dt(pv))
            assert control[0].dtype == np.dtype(dtype) and _equal(control, want), (pads, present)
            assert np.isnan(control[1]).sum() == 0 and np.isnan(control[0]).sum() == np.isnan(uv).any(axis=1).sum() * nz
            views = []
            # a field, a result, a workspace one element into its allocation, each alone and all together: any of them takes
            # the narrow form
            u1, v1 = put(uv, off=1), put(vv, off=1)
            assert u1.data_ptr() % 16 == uv.dtype.itemsize
            A = ALIGNED
            views += [(u1, v, aligned, (A, A, A, A)), (u, v1, aligned, (A, A, A, A)), (u, v, aligned, (1, A, A, A)),
                      (u, v, aligned, (A, 1, A, A)), (u, v, aligned, (A, A, 1, A)), (u, v, aligned, (A, A, A, 1)),
                      (u1, v1, aligned, (1, 1, 1, 1))]
            # the planes one element in; with an odd row pitch; with an odd level pitch (volumes)
            views.append((u, v, {n: put(x, off=1) for n, x in pv.items()}, (A,) * 4))
            pitched = {}
            for n, x in pv.items():
                s = list(x.shape)
                pitched[n] = put(x, _contig(s[:-1] + [s[-1] + 1]) if s[-1] > 1 else _contig(s))
                assert s[-1] == 1 or (pitched[n].stride(-2) == nx + 1 and pitched[n].stride(-1) == 1)
            views.append((u, v, pitched, (A,) * 4))
            for n, form in present.items():
                x = pv[n]
                if form in ("v3", "vl"):
                    st = [(x.shape[1] * (ny * nx + 1)) * (x.shape[0] > 1), ny * nx + 1, nx, 1]
                    lev = put(x, [s or 1 for s in st])
                    assert lev.stride(1) == ny * nx + 1
                    views.append((u, v, dict(aligned, **{n: lev}), (A,) * 4))
                if form == "z":   # the Z-only array three elements apart
                    views.append((u, v, dict(aligned, **{n: put(x, [3 * x.shape[1], 3, 1, 1], 1)}), (A,) * 4))
                if form == "p":   # the plane stored (X, Y): a transposed view, a non-unit stride along X
                    t = put(np.ascontiguousarray(x.transpose(0, 1, 3, 2))).permute(0, 1, 3, 2)
                    assert t.stride(-1) == ny and t.stride(-2) == 1
                    views.append((u, v, dict(aligned, **{n: t}), (A,) * 4))
            for fu, fv, planes, offs in views:
                assert _equal(_abi_call(D, dtype, shape, fu, fv, planes, pads, offs), control), (pads, present, offs)
        # nu with stride 0 along X, along Y and along both: what the expanded array gives
        for cut in ((slice(None), slice(0, 1)), (slice(0, 1), slice(None)), (slice(0, 1), slice(0, 1))):
            z = vals("nu", "v3", 121)[(slice(None), slice(None)) + cut]
            flat = put(z).expand(1, nf, ny, nx)
            assert flat.stride(-1) == 0 or flat.stride(-2) == 0
            full = put(np.ascontiguousarray(np.broadcast_to(z, (1, nf, ny, nx))))
            assert _equal(_abi_call(D, dtype, shape, u, v, {"nu": flat}, pads), _abi_call(D, dtype, shape, u, v, {"nu": full}, pads))
    assert nx % NVS[dtype] == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_abi_layouts(host_abi, dtype):
    abi_layout_cases(dtype)


def abi_bad_calls():
    """bad calls return the header's codes and write nothing; runs on whatever library `_MEM` serves"""
    import xgcm_amd.device as D

    lib = D._MEM.lib()
    shape = [2, 3, 4]
    t = torch.ones(shape, dtype=torch.float64, device=D._MEM.device)
    outs = [torch.full_like(t, SENTINEL) for _ in range(4)]   # work_u, work_v, out_u, out_v
    st = _hip.i64([12, 4, 1])
    P = lambda x: None if x is None else x.data_ptr()  # noqa: E731

    def call(code=CODE[np.float64], u=t, v=t, nu=t, ns=st, met=(None,) * 8, bufs=outs, shp=shape, ndim=3, outer=0, bcx="periodic",
             bcy="extend", dt=1.0):
        bc = lambda b: _hip.BC[b] if isinstance(b, str) else b  # noqa: E731
        return lib.xg_implicit_vertical_viscosity(code, P(u), P(v), P(nu), ns, *met, *(P(b) for b in bufs),
                                                  None if shp is None else _hip.i64(shp), ndim, outer, bc(bcx), 0.0, bc(bcy), 0.0, dt,
                                                  D._stream())

    def untouched():
        return all(bool((b == SENTINEL).all()) for b in outs)

    for code in (-1, _hip.DTYPE["float16"], _hip.DTYPE["int64"], _hip.DTYPE["int32"], 12, 99):
        assert call(code=code) == -1                                          # any other element type: XG_ERR_INVALID
    assert call(u=None) == -1 and call(v=None) == -1 and call(nu=None) == -1 and call(shp=None) == -1   # NULL arguments
    for k in range(4):
        assert call(bufs=[None if j == k else b for j, b in enumerate(outs)]) == -1   # a NULL workspace or result
    assert call(outer=2) == -1 and call(outer=-1) == -1                       # unknown flux position
    assert call(ns=None) == -1                                                # nu without strides
    for k in range(4):
        met = [None] * 8
        met[2 * k] = t.data_ptr()
        assert call(met=met) == -1                                            # a metric without strides
    none, halo = _hip.BC[None] if None in _hip.BC else 0, max(_hip.BC.values()) + 1
    for bad in (none, halo, -3, 17):
        if bad not in (_hip.BC["periodic"], _hip.BC["fill"], _hip.BC["extend"]):
            assert call(bcx=bad) == -1 and call(bcy=bad) == -1                # a bad boundary code
    for dt in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        assert call(dt=dt) == -1                                              # dt negative, NaN or infinite
    assert call(ndim=2) < 0 and call(ndim=2) != -1                            # XG_ERR_UNSUPPORTED
    assert untouched()
    assert call(shp=[2, 0, 4]) == 0 and call(shp=[0, 3, 4]) == 0 and untouched()   # an empty extent: XG_OK, nothing touched
    assert call() == 0 and call(outer=1, dt=0.0, bcx="fill", bcy="fill") == 0 and not untouched()


def test_abi_refuses_bad_calls(host_abi):
    abi_bad_calls()


# ---- 7. between guard bands ---------------------------------------------------------------------------------------------------
def tunable_calls(D, dtype):
    """(calls, references) of the K7o tunable sweep: name -> thunk that calls `D` on inputs uploaded once, name -> thunk that
    gives numpy's pair of results of the same call.  Both flux positions, 3-D and profile metrics, the flux' metrics alone,
    none, all three pads on either axis"""
    f = lambda shape, seed: R.synthetic_field(shape, seed).astype(dtype)  # noqa: E731
    m = lambda shape, seed: R.synthetic_metric(shape, seed).astype(dtype)  # noqa: E731
    calls, references = {}, {}
    for n, shape in enumerate(((5, 300, 264), (3, 65, 131))):
        nz, ny, nx = shape
        u, v = f(shape, 150 + n), f(shape, 152 + n)
        u[1, 7, 9] = u[0, 0, 0] = v[nz - 1, ny - 1, nx - 1] = np.nan
        du, dv = D.asdevice(u), D.asdevice(v)
        for k, (to, bcx, bcy) in enumerate((("left", "periodic", "extend"), ("outer", "fill", "periodic"),
                                            ("left", "extend", "fill"), ("outer", "periodic", "periodic"))):
            nf = nz + (to == "outer")
            nu = np.abs(f((nf, ny, nx), 160 + 4 * n + k)) * dtype(2e4)
            mets = [(m((nf, ny, nx), 172), m((nz, ny, nx), 173), m((nf, ny, nx), 174), m((nz, ny, nx), 175)),
                    (m((nf, 1, 1), 170), m((nz, 1, 1), 171), m((nf, 1, 1), 170), m((nz, 1, 1), 171)),
                    (m((nf, ny, nx), 176), None, m((nf, ny, nx), 177), None), (None,) * 4][k]
            d = tuple(None if x is None else D.asdevice(x) for x in (nu,) + mets)
            key = f"{nx}{to}{k}"
            dt = abi_dt({"mfu": mets[0], "mcu": mets[1]})
            calls[key] = lambda du=du, dv=dv, d=d, a=(to == "outer", bcx, bcy, dt): D.implicit_vertical_viscosity(du, dv, *d, *a, 0.375, -0.0)
            references[key] = lambda h=(u, v, nu) + mets, a=(to, bcx, 0.375, bcy, -0.0, dt): list(statement(*h, *a))
    return calls, references


def guarded_table(D, monkeypatch, dtype, offset, same_bits):
    """the table built and run between guard bands: a store outside a result or a workspace, a cell left unwritten and a
    result-changing read outside nu, a field or a metric all fail; returns the number of results checked"""
    checked = 0
    with GM.guarded(D, monkeypatch, offset) as g:
        calls, references = tunable_calls(D, dtype)
        assert g.placed >= 8 * 3
        for k, fn in calls.items():
            before = g.handed_out
            got = [D.tohost(x) for x in fn()]
            g.check(f"{k} at offset {offset}")
            assert g.handed_out - before >= 4   # two results and two workspaces, all four between guards
            for x, want in zip(got, references[k]()):
                assert same_bits(x, want), f"{k} at offset {offset}: not numpy's result"
                checked += 1
    return checked


def _bits_equal(got, want):
    try:
        _same_bits(got, want)
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_between_guard_bands_through_the_host_abi(host_abi, monkeypatch, dtype):
    import xgcm_amd.device as D

    for offset in (0, np.dtype(dtype).itemsize):
        assert guarded_table(D, monkeypatch, dtype, offset, _bits_equal) == 16


# ---- 8. what the chain itself serves ----------------------------------------------------------------------------------------
def _fallback_equals_chain(grid, u, v, nu, **kw):
    """the operator (the entry barred by the caller) and the chain written out give the same labelled results"""
    got = grid.implicit_vertical_viscosity(u, v, nu, **kw)
    for one, other in zip(got, _chain(grid, u, v, nu, **kw)):
        _same_labelled(one, other)
    return got


def _same_outcome(grid, u, v, nu, **kw):
    """the chain's results, labels included, or the chain's error"""
    try:
        want = _chain(grid, u, v, nu, **kw)
    except Exception:
        _same_error(lambda: grid.implicit_vertical_viscosity(u, v, nu, **kw), lambda: _chain(grid, u, v, nu, **kw))
    else:
        for one, other in zip(grid.implicit_vertical_viscosity(u, v, nu, **kw), want):
            _same_labelled(one, other)


def _same_error(fused, chain):
    with pytest.raises(Exception) as want:
        chain()
    with pytest.raises(type(want.value)) as got:
        fused()
    assert str(got.value) == str(want.value)


def test_nu_none_does_what_the_chain_does(host_abi, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, (u, v, nu) = _case()
    _same_error(lambda: grid.implicit_vertical_viscosity(u, v, None, dt=DT), lambda: _chain(grid, u, v, None, dt=DT))


@pytest.mark.parametrize("dtype", [np.int64, np.float16])
def test_other_dtypes_do_what_the_chain_does(host_abi, monkeypatch, dtype):
    _no_fused(monkeypatch)
    grid, ds, (u, v, nu) = _case()
    ui, vi, ni = (x._replace(data=(x.values * (100 if x.name != "nu" else 0.01)).astype(dtype)) for x in (u, v, nu))
    kw = dict(dt=DT_PLAIN, metric_weighted=False)
    _same_error(lambda: grid.implicit_vertical_viscosity(ui, vi, ni, **kw), lambda: _chain(grid, ui, vi, ni, **kw))


def test_mixed_dtypes_do_what_the_chain_does(host_abi, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, (u, v, nu) = _case(dtype=np.float32)
    n64 = nu._replace(data=nu.values.astype(np.float64))
    _same_error(lambda: grid.implicit_vertical_viscosity(u, v, n64, dt=DT), lambda: _chain(grid, u, v, n64, dt=DT))
    g2, _, _ = _case(dtype=np.float32, mdtype=np.float64)   # float32 fields over float64 metrics
    _same_error(lambda: g2.implicit_vertical_viscosity(u, v, nu, dt=DT), lambda: _chain(g2, u, v, nu, dt=DT))
    v64 = v._replace(data=v.values.astype(np.float64))
    kw = dict(dt=DT_PLAIN, metric_weighted=False)
    _same_error(lambda: grid.implicit_vertical_viscosity(u, v64, nu, **kw), lambda: _chain(grid, u, v64, nu, **kw))


def test_fields_elsewhere_or_of_different_shapes_run_the_chain(host_abi, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, (u, v, nu) = _case(lead=())
    at = lambda x, dims: DataArray(x.values, dims, name=x.name)  # noqa: E731
    _fallback_equals_chain(grid, at(u, ("ZC", "YC", "XC")), v, nu, dt=DT)                    # u at the centre
    _fallback_equals_chain(grid, u, at(v, ("ZC", "YC", "XG")), nu, dt=DT)                    # v at u's points
    _fallback_equals_chain(grid, v, u, nu, dt=DT)                                            # the two swapped
    u2 = DataArray(np.stack([u.values, u.values * 0.5]), ("time",) + u.dims, name="u")       # u with a leading dim v lacks
    _fallback_equals_chain(grid, u2, v, nu, dt=DT)


def test_nu_elsewhere_lacking_a_dim_or_with_a_dim_the_fields_lack_runs_the_chain(host_abi, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, (u, v, nu) = _case(lead=())
    _fallback_equals_chain(grid, u, v, DataArray(nu.values[0], C_AT, name="nu"), dt=DT)                       # no Z dim
    _same_outcome(grid, u, v, DataArray(nu.values[:, :, 0], ("ZO", "YC"), name="nu"), dt=DT)                  # no X dim
    extra = DataArray(np.stack([nu.values, nu.values * 0.5]), ("member",) + nu.dims, name="nu")
    xu, xv = _fallback_equals_chain(grid, u, v, extra, dt=DT)
    assert xu.dims == ("member",) + u.dims and xv.dims == ("member",) + v.dims
    # nu at the wrong face position for this `to`, and at u's points: whatever the chain raises
    for bad, kw in ((DataArray(nu.values[:4], ("ZL",) + C_AT, name="nu"), dict(dt=DT, to="outer")),
                    (DataArray(nu.values, ("ZO",) + U_AT, name="nu"), dict(dt=DT))):
        _same_outcome(grid, u, v, bad, **kw)


def test_z_not_third_from_last_runs_the_chain(host_abi, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, (u, v, nu) = _case()
    xu, xv = _fallback_equals_chain(grid, u.transpose("ZC", "time", "YC", "XG"), v.transpose("ZC", "time", "YG", "XC"), nu, dt=DT)
    wu, wv = _want_of(grid, ds, u, v, nu, dict(dt=DT))
    _same_bits(xu.transpose(*u.dims).values, wu)
    _same_bits(xv.transpose(*v.dims).values, wv)


def test_chunked_inputs_do_what_the_chain_does(host_abi, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, (u, v, nu) = _case(lead=(4,), nz=3, ny=6, nx=8)
    cu = u._replace(data=BlockArray.from_array(u.values, ((2, 2), (3,), (6,), (8,))))
    cn = nu._replace(data=BlockArray.from_array(nu.values, ((4,), (6,), (8,))))
    for f in ((cu, v, nu), (u, v, cn)):
        _same_error(lambda: grid.implicit_vertical_viscosity(*f, dt=DT), lambda: _chain(grid, *f, dt=DT))


def test_a_metric_with_a_dim_its_stage_lacks_runs_the_chain(host_abi, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, (u, v, nu) = _case(lead=())
    coords = {k: (k, np.asarray(ds.coords[k].values)) for k in ("XC", "XG", "YC", "YG", "ZC", "ZL", "ZO")}
    coords["time"] = ("time", np.arange(2) * 2.0)
    data = {"drF": (("ZC", "time"), R.synthetic_metric((4, 2), 66)), "drCo": (("ZO", "time"), R.synthetic_metric((5, 2), 67))}
    g2 = Grid(Dataset(data, coords), coords=AXES, metrics={("Z",): ["drF", "drCo"]},
              padding={"X": "periodic", "Y": "extend", "Z": "extend"}, autoparse_metadata=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)   # (the lookup says that it interpolates the metric)
        xu, xv = _fallback_equals_chain(g2, u, v, nu, dt=DT)
    assert xu.dims == ("time",) + u.dims


def test_a_chunked_metric_does_what_the_chain_does(host_abi, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, (u, v, nu) = _case(lead=())
    coords = {k: (k, np.asarray(ds.coords[k].values)) for k in ("XC", "XG", "YC", "YG", "ZC", "ZL", "ZO")}
    data = {"drF": (("ZC",), BlockArray.from_array(R.synthetic_metric((4,), 66), ((2, 2),))), "drCo": (("ZO",), R.synthetic_metric((5,), 67))}
    g2 = Grid(Dataset(data, coords), coords=AXES, metrics={("Z",): ["drF", "drCo"]},
              padding={"X": "periodic", "Y": "extend", "Z": "extend"}, autoparse_metadata=False)
    _same_error(lambda: g2.implicit_vertical_viscosity(u, v, nu, dt=DT), lambda: _chain(g2, u, v, nu, dt=DT))


def test_a_missing_metric_raises_the_lookups_error_and_is_served_unweighted(host_abi, monkeypatch):
    calls = _counted(monkeypatch)
    grid, ds, (u, v, nu) = _case(mform=None)
    _same_error(lambda: grid.implicit_vertical_viscosity(u, v, nu, dt=DT), lambda: _chain(grid, u, v, nu, dt=DT))
    assert not calls
    kw = dict(dt=DT_PLAIN, metric_weighted=False)
    for got, want in zip(grid.implicit_vertical_viscosity(u, v, nu, **kw), _want_of(grid, ds, u, v, nu, kw)):
        _same_bits(got.values, want)
    assert len(calls) == 1


@pytest.mark.parametrize("axis", ["X", "Y"])
def test_an_axis_without_a_boundary_raises_the_chains_error(host_abi, monkeypatch, axis):
    _no_fused(monkeypatch)
    pads = {"X": (None, "extend"), "Y": ("periodic", None)}[axis]
    grid, ds, (u, v, nu) = _case(pads=pads)
    _same_error(lambda: grid.implicit_vertical_viscosity(u, v, nu, dt=DT), lambda: _chain(grid, u, v, nu, dt=DT))


def test_a_boundary_given_with_the_call_is_served(host_abi, monkeypatch):
    calls = _counted(monkeypatch)
    grid, ds, (u, v, nu) = _case(pads=(None, None))
    kw = dict(dt=DT, padding={"X": "fill", "Y": "periodic"}, fill_value={"X": float("nan"), "Y": 3.0})
    for got, want in zip(grid.implicit_vertical_viscosity(u, v, nu, **kw), _want_of(grid, ds, u, v, nu, kw)):
        _same_bits(got.values, want)
    assert len(calls) == 1


@pytest.mark.parametrize("conn", ["X", "Y", "Z"])
def test_connected_faces_do_what_the_chain_does(host_abi, monkeypatch, conn):
    from test_topology import COORDS

    _no_fused(monkeypatch)
    link = {"face": {0: {conn: (None, (1, conn, False))}, 1: {conn: ((0, conn, False), None)}}}
    ds = Dataset({"drF": (("zc",), R.synthetic_metric((4,), 63)), "drC": (("zl",), R.synthetic_metric((4,), 64))},
                 coords={"x": np.arange(4), "xl": np.arange(4) - 0.5, "y": np.arange(4), "yl": np.arange(4) - 0.5,
                         "face": np.arange(2), "zc": np.arange(4) + 0.5, "zl": np.arange(4) * 1.0})
    grid = Grid(ds, coords=dict(COORDS, Z={"center": "zc", "left": "zl"}), face_connections=link,
                metrics={("Z",): ["drF", "drC"]}, padding={"X": "periodic", "Y": "extend", "Z": "extend"}, autoparse_metadata=False)
    f = lambda dims, seed: DataArray(R.synthetic_field((2, 4, 4, 4), seed), dims, name="f")  # noqa: E731
    u, v = f(("face", "zc", "y", "xl"), 82), f(("face", "zc", "yl", "x"), 83)
    nu = DataArray(np.abs(R.synthetic_field((2, 4, 4, 4), 84)) * 1e4, ("face", "zl", "y", "x"), name="nu")
    _same_outcome(grid, u, v, nu, dt=DT)


def test_a_fold_runs_the_chain(host_abi, monkeypatch):
    _no_fused(monkeypatch)
    nz, ny, nx = 4, 3, 6
    ds = Dataset({"drF": (("zc",), R.synthetic_metric((nz,), 63)), "drC": (("zl",), R.synthetic_metric((nz,), 64))},
                 coords={"xh": np.arange(nx), "xl": np.arange(nx), "yh": np.arange(ny), "yl": np.arange(ny),
                         "zc": np.arange(nz) + 0.5, "zl": np.arange(nz) * 1.0})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        grid = Grid(ds, coords={"X": {"center": "xh", "left": "xl"}, "Y": {"center": "yh", "left": "yl"},
                                "Z": {"center": "zc", "left": "zl"}}, metrics={("Z",): ["drF", "drC"]},
                    padding={"X": "periodic", "Y": {"fold": "corner"}, "Z": "extend"}, autoparse_metadata=False)
        f = lambda dims, seed: DataArray(R.synthetic_field((nz, ny, nx), seed), dims, name="f")  # noqa: E731
        u, v = f(("zc", "yh", "xl"), 92), f(("zc", "yl", "xh"), 93)
        nu = DataArray(np.abs(R.synthetic_field((nz, ny, nx), 94)) * 1e4, ("zl", "yh", "xh"), name="nu")
        _same_outcome(grid, u, v, nu, dt=DT)


# the refusals before any work
@pytest.mark.parametrize("dt", [-1.0, -1e-300, float("nan"), float("inf"), float("-inf")])
def test_a_bad_dt_raises_before_any_work(host_abi, monkeypatch, dt):
    import xgcm_amd.device as D

    _no_fused(monkeypatch)
    for name in ("stencil1d", "implicit_vertical_diffusion"):
        monkeypatch.setattr(D, name, lambda *a, **k: pytest.fail("work before the refusal"))
    grid, ds, (u, v, nu) = _case()
    with pytest.raises(ValueError, match="dt must be finite and not negative"):
        grid.implicit_vertical_viscosity(u, v, nu, dt=dt)
    with pytest.raises(ValueError, match="dt must be finite and not negative"):
        grid.implicit_vertical_diffusion(u, None, dt=dt)   # what that operator raises


def test_a_missing_dt_raises(host_abi, monkeypatch):
    _no_fused(monkeypatch)
    grid, ds, (u, v, nu) = _case()
    with pytest.raises(TypeError, match="dt, the time step, is required"):
        grid.implicit_vertical_viscosity(u, v, nu)
    with pytest.raises(TypeError, match="dt, the time step, is required"):
        grid.implicit_vertical_diffusion(u, None)
