"""The pre-gathered halo forms of the C ABI -- `stencil1d_halo`, `stencil1d_halo_w`, the `_halo` entries of vorticity,
divergence, gradient and flux, and the gather that fills their slabs -- at kernel sizes: case builders, numpy references and
their CPU twins.

Every complex topology (face connections, the tripolar fold, the sharded axis) takes its boundary cells from a slab and not
from a boundary mode inside the kernel.  The references here are plain numpy statements in the operands' own dtype: the slab
(or the pad of an ordinary mode) is attached with `np.concatenate`, then the operator is written out by slicing, in the
kernel's order of operations.  None of them calls `oracle.fake_device` or `oracle.refimpl`'s operators; the gather's reference
is `oracle.topology.gather_tokens`.  Values are compared bit for bit (`test_gpu_tunables._same_bits`: NaN where the other has
NaN, -0.0 is not +0.0).

The CPU twins run the two stencil forms through the `host_abi` fixture (the product's `xgcm_amd.device` over the host build of
the ABI, which serves those two entries) and the vector forms and the gather through `oracle.fake_device` (the host build
answers `unsupported` for them): argument order, slab layout and the references are checked before any GPU time is spent.
tests/test_gpu_halo_forms.py runs the same cases on the HIP library.

NaN cells.  `NAN_SITES` lists where they sit, in the order in which a case takes them: a case of `cells` cells per (Y, X)
stack takes `cells // 250` of them (all of them from 3000 cells on, never fewer than one).  One NaN input cell reaches at most
two cells of a two-point operator's result, so the share stays under 1 % -- asserted on every reference, with `at least one
NaN`.  A reference of fewer than 250 cells ((5, 6) planes, (1, 260) without leading dims) cannot hold one NaN cell AND stay
under 1 %: it takes one site and is held to what that one cell can reach, two cells (`TINY`)."""

import itertools

import numpy as np
import pytest

import test_gpu_tunables as TT
from oracle import refimpl as R

DTYPES = [np.float64, np.float32]
MODES = ["periodic", "extend", "fill"]
# all seven mode pairs that contain a halo
PAIRS = [("halo", "halo")] + [("halo", m) for m in MODES] + [(m, "halo") for m in MODES]
FILL_X, FILL_Y = 1.75, -0.625                      # non-zero, different per axis, exact in float32
# (ny, nx): the vector form (f64: three tiles, two lanes in the last; f32: two tiles, one lane in the last; 15 segments, the
# last of one row); the scalar form (five tiles, three lanes in the last); one segment (`nrow < SEG`; the halo row is below
# the first row and next to the last); one partial tile; what the Grid tests use
SHAPES = [(29, 260), (29, 259), (1, 260), (2, 259), (9, 64), (5, 6)]
LEADS = [(), (5,), (2, 3)]                         # ZK = 4: groups of 4 + 1 and 4 + 2; ZK = 2: an odd last group
AREAS = ["none", "shared", "face", "own", "ycol"]  # absent; (1, .., Y, X); (1, 3, Y, X) under (2, 3, Y, X); the fields'; (1, .., Y, 1)
OPS = ["diff", "interp", "min", "max"]
TINY = 250                                         # cells below which one NaN cell is 1 % or more of what it reaches


def same_bits(got, want, what=""):
    assert TT._same_bits(np.asarray(got), np.asarray(want)), what


def _field(shape, seed, dtype):
    return R.synthetic_field(tuple(shape), seed).astype(dtype)


def _metric(shape, seed, dtype):
    return R.synthetic_metric(tuple(shape), seed).astype(dtype)


# ---- numpy references -----------------------------------------------------------------------------------------------------
def _attach(a, axis, low, mode, fill, slab):
    """`a` with one cell attached along `axis`, below index 0 (`low`) or above the last one: the slab of a halo mode, or what
    the ordinary mode pads with (numpy.pad's wrap / edge / constant, written as slices)"""
    n = a.shape[axis]
    if mode == "halo":
        edge = np.expand_dims(np.asarray(slab, dtype=a.dtype), axis)
    elif mode == "periodic":
        edge = np.take(a, [n - 1 if low else 0], axis=axis)
    elif mode == "extend":
        edge = np.take(a, [0 if low else n - 1], axis=axis)
    else:
        edge = np.full_like(np.take(a, [0], axis=axis), fill)
    assert edge.dtype == a.dtype
    return np.concatenate([edge, a] if low else [a, edge], axis=axis)


def want_vorticity(u, v, area, bx, by, hx=None, hy=None):
    """((v - v_left) - (u - u_below)) / area; the slabs: the column left of i = 0 (..., Y), the row below j = 0 (..., X)"""
    vp, up = _attach(v, -1, True, bx, FILL_X, hx), _attach(u, -2, True, by, FILL_Y, hy)
    z = (vp[..., 1:] - vp[..., :-1]) - (up[..., 1:, :] - up[..., :-1, :])
    return z if area is None else z / area


def want_divergence(u, v, area, bx, by, hx=None, hy=None):
    """((u_right - u) + (v_up - v)) / area; the slabs: the column right of the last one, the row above the last one"""
    up, vp = _attach(u, -1, False, bx, FILL_X, hx), _attach(v, -2, False, by, FILL_Y, hy)
    z = (up[..., 1:] - up[..., :-1]) + (vp[..., 1:, :] - vp[..., :-1, :])
    return z if area is None else z / area


def want_gradient(a, mx, my, bx, by, hx=None, hy=None):
    """(a - a_left) / mx and (a - a_below) / my"""
    ax, ay = _attach(a, -1, True, bx, FILL_X, hx), _attach(a, -2, True, by, FILL_Y, hy)
    gx, gy = ax[..., 1:] - ax[..., :-1], ay[..., 1:, :] - ay[..., :-1, :]
    return (gx if mx is None else gx / mx), (gy if my is None else gy / my)


def want_flux(u, v, t, bx, by, hx=None, hy=None):
    """u * ((t_left + t) / 2) and v * ((t_below + t) / 2)"""
    tx, ty = _attach(t, -1, True, bx, FILL_X, hx), _attach(t, -2, True, by, FILL_Y, hy)
    return u * ((tx[..., :-1] + tx[..., 1:]) / 2.0), v * ((ty[..., :-1, :] + ty[..., 1:, :]) / 2.0)


def want_stencil(op, x, halo, axis, lo, hi, m_out=None, m_in=None):
    """the product x * m_in rounded to the dtype, the slabs attached as they are (not weighted), the operator, / m_out"""
    p = x if m_in is None else x * m_in
    assert p.dtype == x.dtype and halo.dtype == x.dtype
    p = np.concatenate([np.take(halo, range(0, lo), axis=axis), p, np.take(halo, range(lo, lo + hi), axis=axis)], axis=axis)
    n = p.shape[axis]
    a, b = np.take(p, range(0, n - 1), axis=axis), np.take(p, range(1, n), axis=axis)
    r = {"diff": lambda: b - a, "interp": lambda: (a + b) / 2.0, "min": lambda: np.minimum(a, b), "max": lambda: np.maximum(a, b)}[op]()
    assert r.dtype == x.dtype
    return r if m_out is None else r / m_out


# ---- vector cases ---------------------------------------------------------------------------------------------------------
def area_shape(form, lead, ny, nx):
    """the shape of an area / metric plane of `form` under fields of lead + (ny, nx); None: absent; False: no such form here"""
    one = (1,) * len(lead)
    if form == "face":
        return (1, 3, ny, nx) if lead == (2, 3) else False
    return {"none": None, "shared": one + (ny, nx), "own": tuple(lead) + (ny, nx), "ycol": one + (ny, 1)}[form]


# where the NaN cells sit, in the order a case takes them: (array, j, i); "fx" / "fy": the field differenced along X / Y (v and
# u of the vorticity, u and v of the divergence, the one field of gradient and flux); "hx" / "hy": the slabs, by flat index
# within an outer index; negative indices count from the end; a site is dropped where the plane does not have it
NAN_SITES = [("fx", -1, -1), ("hx", 0), ("hy", -1), ("fy", 0, 0), ("fx", 3, 127), ("fy", 4, 128), ("fx", 8, 255), ("fy", 9, 256),
             ("hx", -1), ("hy", 0), ("fy", -1, 1), ("fx", 0, 0)]


def put_nans(fx, fy, hx, hy):
    """writes NaN into the arrays at as many of NAN_SITES as the size allows (see the module docstring); site k at outer index
    (last - k) modulo the number of outer indices, so that the last level -- the short group of ZK -- has the first one"""
    ny, nx = fx.shape[-2:]
    nouter = int(np.prod(fx.shape[:-2]))
    take = max(1, (nouter * ny * nx) // TINY)
    arrays = {"fx": fx.reshape(nouter, ny, nx), "fy": fy.reshape(nouter, ny, nx),
              "hx": None if hx is None else hx.reshape(nouter, ny), "hy": None if hy is None else hy.reshape(nouter, nx)}
    k = 0
    for name, *at in NAN_SITES:
        arr = arrays[name]
        if k >= take:
            break
        if arr is None or any(not -n <= i < n for i, n in zip(at, arr.shape[1:])):
            continue
        arr[(nouter - 1 - k) % nouter][tuple(at)] = np.nan
        k += 1
    assert k >= 1
    return k


def check_nan_share(ref, what=""):
    """on the reference alone: at least one NaN, and under 1 % of the cells (TINY references: the two cells of one site)"""
    n = int(np.isnan(ref).sum())
    assert n >= 1, what
    assert (n <= 2) if ref.size < TINY else (n / ref.size < 0.01), (what, n, ref.size)


class VectorCase:
    """one (ny, nx), one set of leading dims, one dtype: three fields and both slabs of each kind with their NaN cells, shared
    by every operator, area form and mode pair (an ordinary mode ignores its axis' slab)"""

    def __init__(self, ny, nx, lead, dtype, seed=300):
        self.ny, self.nx, self.lead, self.dtype = ny, nx, tuple(lead), dtype
        s = self.shape = self.lead + (ny, nx)
        # per operator: the fields (u, v, t) and the slabs (along X: (..., Y); along Y: (..., X)).  Vorticity differences v
        # along X and u along Y and takes the column left of i = 0 and the row below j = 0; divergence differences u along X
        # and v along Y and takes the column right of the last one and the row above the last one; gradient and flux share
        # one tracer, its slabs and a NaN-free (u, v)
        self.sets = {}
        for k, op in enumerate(("vorticity", "divergence", "pair")):
            f = {name: _field(s, seed + 10 * k + j, dtype) for j, name in enumerate("uvt")}
            f["hx"], f["hy"] = _field(self.lead + (ny,), seed + 10 * k + 5, dtype), _field(self.lead + (nx,), seed + 10 * k + 6, dtype)
            along_x, along_y = {"vorticity": ("v", "u"), "divergence": ("u", "v"), "pair": ("t", "t")}[op]
            put_nans(f[along_x], f[along_y], f["hx"], f["hy"])
            self.sets[op] = f
        self.sets["gradient"] = self.sets["flux"] = self.sets["pair"]

    def __repr__(self):
        return f"{self.shape} {np.dtype(self.dtype)}"

    def area(self, form, seed=330):
        sh = area_shape(form, self.lead, self.ny, self.nx)
        return None if sh is None else _metric(sh, seed, self.dtype)

    def operands(self, op, bx, by, arrays=None):
        """(u, v, t, halo_x, halo_y) as the call takes them: None for the slab of an axis with an ordinary mode; `arrays`:
        stand-ins for this operator's set (uploaded once, or laid out by the caller)"""
        f = arrays or self.sets[op]
        return f["u"], f["v"], f["t"], (f["hx"] if bx == "halo" else None), (f["hy"] if by == "halo" else None)

    def call(self, D, op, bx, by, planes, arrays=None):
        """one call of `D`; `planes`: (area,) / (mx, my) / ()"""
        u, v, t, hx, hy = self.operands(op, bx, by, arrays)
        if op == "vorticity":
            return (D.vorticity(u, v, planes[0], bx, by, FILL_X, FILL_Y, hx, hy),)
        if op == "divergence":
            return (D.divergence(u, v, planes[0], bx, by, FILL_X, FILL_Y, hx, hy),)
        if op == "gradient":
            return D.gradient(t, bx, by, FILL_X, FILL_Y, planes[0], planes[1], hx, hy)
        return D.flux(u, v, t, bx, by, FILL_X, FILL_Y, hx, hy)

    def want(self, op, bx, by, planes):
        u, v, t, hx, hy = self.operands(op, bx, by)
        if op == "vorticity":
            return (want_vorticity(u, v, planes[0], bx, by, hx, hy),)
        if op == "divergence":
            return (want_divergence(u, v, planes[0], bx, by, hx, hy),)
        if op == "gradient":
            return want_gradient(t, planes[0], planes[1], bx, by, hx, hy)
        return want_flux(u, v, t, bx, by, hx, hy)


def curl_div_forms(case):
    """(op, area form, area) over both operators and every area form this case has"""
    for op, form in itertools.product(("vorticity", "divergence"), AREAS):
        if area_shape(form, case.lead, case.ny, case.nx) is not False:
            yield op, form, (case.area(form),)


GRAD_FORMS = ["none", "shared", "own"]   # no metrics; level-shared mx and my (banded); metrics of the field's own shape


def pair_forms(case):
    """(op, form, planes) of gradient (three metric forms) and flux"""
    for form in GRAD_FORMS:
        yield "gradient", form, (case.area(form, 331), case.area(form, 332))
    yield "flux", "none", ()


def check_vector_case(D, case, forms, tohost=np.asarray, fetched=None, upload=None):
    """every (operator, form) of `forms` under all seven mode pairs through `D`, against numpy; returns the number of calls.
    `upload`: fields and slabs go to the device once per operator; `fetched`: the set a recorder on the library fills"""
    n = 0
    resident = {}
    for (op, form, planes), (bx, by) in itertools.product(list(forms), PAIRS):
        what = f"{op} {case} area/metric {form} ({bx}, {by})"
        want = case.want(op, bx, by, planes)
        if upload is not None and op not in resident:
            resident[op] = {k: upload(a) for k, a in case.sets[op].items()}
        if fetched is not None:
            fetched.clear()
        got = case.call(D, op, bx, by, planes, resident.get(op))
        assert len(got) == len(want), what
        for g, w in zip(got, want):
            check_nan_share(w, what)
            same_bits(tohost(g), w, what)
        if fetched is not None:
            sfx = "_f64" if case.dtype is np.float64 else "_f32"
            assert f"xg_{op}_halo{sfx}" in fetched and f"xg_{op}{sfx}" not in fetched, (what, fetched)
        n += 1
    return n


# ---- stencil cases --------------------------------------------------------------------------------------------------------
# a march of at least 256 rows; odd, unaligned rows; four dims with a row length of the vector form
STENCIL_FIELDS = [(5, 300, 264), (3, 65, 131), (2, 4, 40, 260)]
STENCIL_PADS = [(1, 0), (0, 1), (1, 1)]
# m_in: absent (`stencil1d_halo`); its full shape; without the operator's axis; (Z, 1, 1); (1, Y, X)
M_IN = [None, "full", "no_axis", "z", "plane"]
M_OUT = [None, "full", "plane"]


def _m_shape(form, shape, axis):
    nd = len(shape)
    if form == "full":
        return tuple(shape)
    if form == "no_axis":
        return tuple(1 if d == axis else n for d, n in enumerate(shape))
    if form == "z":
        return tuple(n if d == nd - 3 else 1 for d, n in enumerate(shape))
    return tuple(n if d >= nd - 2 else 1 for d, n in enumerate(shape))


def stencil_field(shape, dtype):
    """the field of a stencil table: NaN cells at both ends of the flat array, at the lane-63 seam of a row and in the last row"""
    x = _field(shape, 400 + len(shape) + shape[-1], dtype)
    x.reshape(-1)[[0, -1]] = np.nan
    x[..., 1, 63] = np.nan
    x[(0,) * (len(shape) - 2) + (shape[-2] - 1, 64)] = np.nan
    return x


def stencil_cases(shape, dtype, x=None, build=True):
    """(op, axis, lo, hi, halo, m_in, m_out, form names): the full product of axes, operators, pads, m_in forms and m_out
    absent / present; a present m_out is of the result's shape or a (1, Y, X) plane in turns.  `build` False: the table alone,
    without its arrays"""
    x = stencil_field(shape, dtype) if x is None else x
    nd = len(shape)
    out = []
    for n, (axis, op, (lo, hi), fin, present) in enumerate(itertools.product(range(nd), OPS, STENCIL_PADS, M_IN, (False, True))):
        fout = M_OUT[1 + (n // 2) % 2] if present else None
        if not build:
            out.append((op, axis, lo, hi, None, None, None, (fin, fout)))
            continue
        hshape = list(shape)
        hshape[axis] = lo + hi
        halo = _field(hshape, 430 + n, dtype)
        halo.reshape(-1)[[0, -1]] = np.nan       # slab element 0 and the slab's last element
        oshape = list(shape)
        oshape[axis] += lo + hi - 1
        m_in = None if fin is None else _metric(_m_shape(fin, shape, axis), 460 + n, dtype)
        m_out = None if fout is None else _metric(_m_shape(fout, oshape, axis), 490 + n, dtype)
        out.append((op, axis, lo, hi, halo, m_in, m_out, (fin, fout)))
    return x, out


def check_stencil_cases(D, x, cases, tohost=np.asarray, xd=None, fetched=None):
    """`xd`: the field as the call takes it (uploaded once, or laid out by the caller)"""
    for op, axis, lo, hi, halo, m_in, m_out, forms in cases:
        what = f"{op} {x.shape} {x.dtype} axis {axis} pads ({lo}, {hi}) m_in / m_out {forms}"
        want = want_stencil(op, x, halo, axis, lo, hi, m_out, m_in)
        n = int(np.isnan(want).sum())
        assert 1 <= n and n / want.size < 0.01, (what, n)
        if fetched is not None:
            fetched.clear()
        got = tohost(D.stencil1d_halo(op, x if xd is None else xd, halo, axis, lo, hi, m_out, m_in))
        same_bits(got, want, what)
        if fetched is not None:
            sfx = "_f64" if x.dtype == np.float64 else "_f32"
            assert ("xg_stencil1d_halo_w" if m_in is not None else "xg_stencil1d_halo") + sfx in fetched, (what, fetched)


# ---- gather cases ---------------------------------------------------------------------------------------------------------
# (in shape, mapped flags, lo, hi, partner shape, partner perm): a long-row, a per-cell and a partner case
GATHER_CASES = [((3, 9, 200), (False, True, True), (0, 1, 2), (0, 2, 1), None, None),
                ((3, 4, 5), (False, True, True), (0, 1, 2), (0, 2, 1), None, None),
                ((4, 7, 300), (True, True, True), (0, 2, 2), (0, 2, 2), (4, 300, 7), (0, 2, 1))]
GATHER_FILLS = [0.25, -7.25, float("nan")]


def gather_case(k, dtype):
    """(field, partner, the further args of `gather`, reference): a seeded token map over the whole padded plane -- sources of
    the field and its partner, signs, fill slots.  The NaN fill slot stands on the plane's first cell (a halo cell in every
    case) and on one token in 400; the per-cell case, where one token is already 1.8 % of the result (three unmapped levels
    of 56 cells), has its NaN in the field's last cell instead, which no token names: it arrives by the interior copy"""
    from oracle import topology as T

    shape, mapped, lo, hi, pshape, perm = GATHER_CASES[k]
    rng = np.random.default_rng(170 + k)
    x = _field(shape, 93 + k, dtype)
    partner = None if pshape is None else _field(pshape, 96 + k, dtype)
    out_shape = [n + (a + b if m else 0) for n, m, a, b in zip(shape, mapped, lo, hi)]
    p_out = int(np.prod([n for n, m in zip(out_shape, mapped) if m]))
    p_in = int(np.prod([n for n, m in zip(shape, mapped) if m]))
    p_partner = 0 if partner is None else int(np.prod([pshape[j] for j in range(len(pshape)) if mapped[perm[j]]]))
    tok = rng.integers(1, p_in + p_partner + 1, size=p_out).astype(np.int64)
    tok = np.where(rng.random(p_out) < 0.2, T.FILL_BASE + rng.integers(0, 2, size=p_out), tok)
    if p_out >= 400:
        tok[rng.choice(p_out, size=p_out // 400, replace=False)] = T.FILL_BASE + 2
        tok[0] = T.FILL_BASE + 2
    else:
        x.reshape(-1)[-1] = np.nan
        tok[tok == p_in] = 1
    tok = np.where(rng.random(p_out) < 0.3, -tok, tok)
    args = (tok, mapped, lo, out_shape, GATHER_FILLS, perm)
    return x, partner, args, T.gather_tokens(x, partner, *args)


# ---- Grid on connected faces ----------------------------------------------------------------------------------------------
GRID_FILL = 2.5


def _face_pad(conn, a, dims, axis, widths, partner=None, partner_dims=None, vectoraxis=None):
    """`a` padded along `axis` through the face connections by the oracle's numpy statement (`fill` at an unconnected edge)"""
    from oracle import topology as T

    pos = lambda dd: {"X": [d for d in ("x", "xl") if d in dd][0], "Y": [d for d in ("y", "yl") if d in dd][0]}  # noqa: E731
    kw = {} if partner is None else dict(partner=partner, partner_dims=partner_dims, partner_axis_dim=pos(partner_dims), vectoraxis=vectoraxis)
    return T.pad_face_connections(a, dims, "face", pos(dims), conn["face"], ["X", "Y"], {axis: widths}, {"X": "fill", "Y": "fill"},
                                  {"X": GRID_FILL, "Y": GRID_FILL}, **kw)


def grid_case(conn, n, dtype, nz=3):
    """a connected grid of n x n faces with per-face rA / rAz, dxc / dxl, dyc / dyl, and (u, v, t) over `nz` levels with NaN
    cells on face edges; returns (grid, u, v, t, want): `want` maps an operator's name to numpy differences of the arrays
    padded through the connections"""
    from xgcm_amd import DataArray, Dataset, Grid

    nf = len(conn["face"])
    mk = lambda seed: _metric((nf, n, n), seed, dtype)  # noqa: E731
    m = {"rA": ("y", "x"), "rAz": ("yl", "xl"), "dxc": ("y", "x"), "dxl": ("y", "xl"), "dyc": ("y", "x"), "dyl": ("yl", "x")}
    ds = Dataset({k: (("face",) + d, mk(500 + j)) for j, (k, d) in enumerate(m.items())},
                 coords={"x": np.arange(n), "xl": np.arange(n) - 0.5, "y": np.arange(n), "yl": np.arange(n) - 0.5,
                         "face": np.arange(nf), "z": np.arange(nz)})
    coords = {"X": {"center": "x", "left": "xl"}, "Y": {"center": "y", "left": "yl"}}
    grid = Grid(ds, coords=coords, face_connections=conn, padding="fill", fill_value=GRID_FILL,
                metrics={("X",): ["dxc", "dxl"], ("Y",): ["dyc", "dyl"], ("X", "Y"): ["rAz", "rA"]}, autoparse_metadata=False)
    ud, vd, td = ("z", "face", "y", "xl"), ("z", "face", "yl", "x"), ("z", "face", "y", "x")
    u, v, t = (_field((nz, nf, n, n), 510 + k, dtype) + dtype(0.5) for k in range(3))
    for k, a in enumerate((u, v, t)):   # face edges: a corner, the last column, the last row, the first column
        a[0, 0, 0, 0] = a[nz - 1, nf - 1, (k + 1) % n, n - 1] = a[1 % nz, 0, n - 1, (k + 2) % n] = a[nz - 1, 1, n // 2, 0] = np.nan
    mv = {k: np.asarray(ds[k].values)[None] for k in m}
    want = {}
    vp, up = _face_pad(conn, v, vd, "X", (1, 0), u, ud, "Y"), _face_pad(conn, u, ud, "Y", (1, 0), v, vd, "X")
    want["vorticity"] = ((vp[..., 1:] - vp[..., :-1]) - (up[..., 1:, :] - up[..., :-1, :])) / mv["rAz"]
    up, vp = _face_pad(conn, u, ud, "X", (0, 1), v, vd, "X"), _face_pad(conn, v, vd, "Y", (0, 1), u, ud, "Y")
    want["divergence"] = ((up[..., 1:] - up[..., :-1]) + (vp[..., 1:, :] - vp[..., :-1, :])) / mv["rA"]
    tx, ty = _face_pad(conn, t, td, "X", (1, 0)), _face_pad(conn, t, td, "Y", (1, 0))
    want["gradient"] = ((tx[..., 1:] - tx[..., :-1]) / mv["dxl"], (ty[..., 1:, :] - ty[..., :-1, :]) / mv["dyl"])
    want["flux"] = (u * ((tx[..., :-1] + tx[..., 1:]) / 2.0), v * ((ty[..., :-1, :] + ty[..., 1:, :]) / 2.0))
    # metric_weighted interp: the product, then the pad (the fill value is not weighted), the operator, the division
    px, py = _face_pad(conn, t * mv["dxc"], td, "X", (1, 0)), _face_pad(conn, t * mv["dyc"], td, "Y", (1, 0))
    want["interp_x"] = ((px[..., :-1] + px[..., 1:]) / 2.0) / mv["dxl"]
    want["interp_y"] = ((py[..., :-1, :] + py[..., 1:, :]) / 2.0) / mv["dyl"]
    return grid, DataArray(u, ud), DataArray(v, vd), DataArray(t, td), want


def check_grid_case(conn, n, dtype):
    grid, u, v, t, want = grid_case(conn, n, dtype)
    got = {"vorticity": grid.vorticity(u, v), "divergence": grid.divergence(u, v), "gradient": grid.gradient(t, metric_weighted=True),
           "flux": grid.flux(u, v, t), "interp_x": grid.interp(t, "X", metric_weighted="X"),
           "interp_y": grid.interp(t, "Y", metric_weighted="Y")}
    for name, w in want.items():
        for g, ww in zip(got[name] if isinstance(w, tuple) else (got[name],), w if isinstance(w, tuple) else (w,)):
            assert ww.dtype == np.dtype(dtype) and np.isnan(ww).any(), name
            assert np.isnan(ww).mean() < 0.01 or ww[0, 0].size < TINY, name    # (6 x 6 faces: a NaN cell is 2.8 % of its face)
            same_bits(np.asarray(g.values), ww, f"{name} {n} x {n} {np.dtype(dtype)}")


def connections():
    import test_topology as TP

    return {"x2x": TP.X_TO_X, "x2y_rev": TP.X_TO_Y_REV, "cubed_sphere": TP.CUBED_SPHERE}


@pytest.mark.parametrize("conn", ["x2x", "x2y_rev", "cubed_sphere"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_grid_on_connected_faces_equals_numpy_at_the_smallest_size(backend, conn, dtype):
    """the Grid-level case of the GPU suite at 6 x 6 faces: its reference, dims and keywords, on the oracle double"""
    check_grid_case(connections()[conn], 6, dtype)


# ---- the CPU twins --------------------------------------------------------------------------------------------------------
def test_the_tables_meet_every_path_they_are_there_for():
    """what the shapes rely on, stated over the tables (WAVE = 64 lanes of NV = 2 / 4 columns, segments of FSEG = 2 rows)"""
    (ny, nx), (_, nxs) = SHAPES[0], SHAPES[1]
    assert nx % 4 == 0 and nx % 128 and nx % 256 and nx > 256          # the vector form in both dtypes, a partial last tile
    assert -(-nx // 128) == 3 and (nx % 128) // 2 == 2 and -(-nx // 256) == 2 and (nx % 256) // 4 == 1
    assert nxs % 2 == 1 and -(-nxs // 64) == 5 and nxs % 64 == 3       # the scalar form
    nseg = (ny + 1) // 2
    assert ny % 2 == 1 and nseg == 15 and all(nseg % segs for segs in (2, 4, 8))   # ragged against every band height
    assert (1, 260) in SHAPES and (2, 259) in SHAPES and (9, 64) in SHAPES and (5, 6) in SHAPES
    nouter = [int(np.prod(lead)) for lead in LEADS]
    assert nouter == [1, 5, 6] and {n % 4 for n in nouter} == {1, 2} and any(n % 2 for n in nouter if n > 1)
    # every mode stands on each axis beside a halo
    assert len(set(PAIRS)) == 7 and all("halo" in p for p in PAIRS)
    assert {bx for bx, by in PAIRS if by == "halo"} == {by for bx, by in PAIRS if bx == "halo"} == set(MODES) | {"halo"}
    assert FILL_X != FILL_Y and FILL_X != 0 != FILL_Y
    # the area forms: level-shared, per face under (2, 3), the fields' own, a Y column
    assert area_shape("shared", (2, 3), 29, 260) == (1, 1, 29, 260) and area_shape("face", (2, 3), 29, 260) == (1, 3, 29, 260)
    assert area_shape("ycol", (5,), 29, 260) == (1, 29, 1) and area_shape("face", (5,), 29, 260) is False
    # the stencil tables: the full product of axes, operators, pads, m_in forms and m_out absent / present; both m_out forms
    for shape in STENCIL_FIELDS:
        _, cases = stencil_cases(shape, np.float32, x=False, build=False)
        nd = len(shape)
        assert len(cases) == nd * 120 and {(c[1], c[0], (c[2], c[3]), c[7][0], c[7][1] is not None) for c in cases} == set(
            itertools.product(range(nd), OPS, STENCIL_PADS, M_IN, (False, True)))
        assert {(c[1], c[7][0], c[7][1]) for c in cases} == set(itertools.product(range(nd), M_IN, M_OUT))
    assert STENCIL_FIELDS[0][1] >= 256 and STENCIL_FIELDS[1][2] % 2 == 1 and STENCIL_FIELDS[2][3] % 4 == 0
    # the NaN sites: both ends of a row, both sides of both lane-63 seams, the last row, both ends of both slabs
    cells = {(s[0], s[-1]) for s in NAN_SITES if s[0][0] == "f"}
    assert {i for _, i in cells} >= {0, -1, 127, 128, 255, 256} and any(s[1] == -1 for s in NAN_SITES if s[0][0] == "f")
    assert {s for s in NAN_SITES if s[0][0] == "h"} == {("hx", 0), ("hx", -1), ("hy", 0), ("hy", -1)}
    assert all(int(np.prod(lead + s)) < 1_000_000 for lead in LEADS for s in SHAPES) and all(np.prod(s) < 1_000_000 for s in STENCIL_FIELDS)


def test_every_nan_site_is_taken_at_kernel_size_and_one_at_the_smallest():
    big = VectorCase(29, 260, (2, 3), np.float64)
    for op, (along_x, along_y) in (("vorticity", "vu"), ("divergence", "uv"), ("pair", "tt")):
        f = big.sets[op]
        fx, fy = f[along_x], f[along_y]
        assert all(np.isnan(fx[..., i]).any() for i in (0, 127, 255, 259)) and all(np.isnan(fy[..., i]).any() for i in (0, 128, 256))
        assert np.isnan(fx[..., -1, :]).any() and np.isnan(fy[..., -1, :]).any()
        for slab in (f["hx"], f["hy"]):
            s = slab.reshape(6, -1)
            assert np.isnan(s[:, 0]).any() and np.isnan(s[:, -1]).any()
        assert sum(int(np.isnan(a).sum()) for a in {id(a): a for a in (fx, fy, f["hx"], f["hy"])}.values()) == len(NAN_SITES)
    assert not np.isnan(big.sets["flux"]["u"]).any() and not np.isnan(big.sets["flux"]["v"]).any()
    small = VectorCase(5, 6, (), np.float32)
    for op, along_x in (("vorticity", "v"), ("divergence", "u"), ("pair", "t")):
        f = small.sets[op]
        assert [int(np.isnan(f[k]).sum()) for k in ("hx", "hy")] == [0, 0] and int(np.isnan(f[along_x]).sum()) == 1
        assert sum(int(np.isnan(f[k]).sum()) for k in "uvt") == 1


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("ny,nx", SHAPES)
def test_vector_forms_equal_numpy(backend, ny, nx, dtype):
    """vorticity, divergence, gradient and flux with slabs: the full product of leading dims, area / metric forms and mode
    pairs (every reference's NaN share is asserted on the way)"""
    import xgcm_amd.device as D

    n = 0
    for lead in LEADS:
        case = VectorCase(ny, nx, lead, dtype)
        n += check_vector_case(D, case, curl_div_forms(case), D.tohost)
        n += check_vector_case(D, case, pair_forms(case), D.tohost)
    assert n == 7 * (2 * (4 + 4 + 5) + 3 * 4)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("shape", STENCIL_FIELDS, ids=str)
def test_stencil_forms_equal_numpy(host_abi, shape, dtype):
    import xgcm_amd.device as D

    x, cases = stencil_cases(shape, dtype)
    assert len(cases) == len(shape) * 120
    check_stencil_cases(D, x, cases, D.tohost)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_gather_cases_equal_the_token_decode(backend, dtype):
    import xgcm_amd.device as D

    for k in range(len(GATHER_CASES)):
        x, partner, args, want = gather_case(k, dtype)
        n = int(np.isnan(want).sum())
        assert want.dtype == np.dtype(dtype) and n >= 1 and n / want.size < 0.01, (k, n, want.size)
        same_bits(D.tohost(D.gather(x, partner, *args)), want, f"gather case {k}")


def test_the_weighted_form_does_not_weight_its_slab(host_abi):
    """the reference's statement itself: with m_in the slab cells enter as they are -- weighting them again changes the result"""
    import xgcm_amd.device as D

    x, halo, m = _field((3, 9, 12), 1, np.float64), _field((3, 9, 1), 2, np.float64), _metric((3, 9, 12), 3, np.float64)
    got = D.tohost(D.stencil1d_halo("diff", x, halo, 2, 1, 0, None, m))
    same_bits(got, want_stencil("diff", x, halo, 2, 1, 0, None, m))
    assert np.array_equal(got[..., 0], x[..., 0] * m[..., 0] - halo[..., 0])
    assert not np.array_equal(got[..., 0], x[..., 0] * m[..., 0] - halo[..., 0] * m[..., 0])
