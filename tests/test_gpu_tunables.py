"""Every launch-shape tunable, at every value it is documented to take, computes what the defaults compute.

`xg_set_tunable` / `XG_<NAME>` choose among kernels and work orders -- speed, never results (include/xgcm_hip.h "tunables";
VERDICT r05 weak #10: "30+ knobs reachable from environment variables are a large untested configuration surface").  Here a
battery of calls -- flat and marching stencils with and without metrics, the three scans, the reductions in every mode, pads,
the fused vector operators, the one-pass operators K7d - K7k, both transforms, the pre-gathered halo forms and the gather that
fills their slabs -- is run once under the defaults and then again under each alternative value of each tunable, float64 and
float32: bit for bit the same, except along the contiguous axis where sums are re-associated by contract (rtol 1e-12 / 1e-5).

What the battery reaches is checked, not claimed: the default run records which entries of the C ABI are fetched from the
library, and every `xg_*_f64` / `xg_*_f32` entry of `_hip.SIGNATURES` has to be among them or in `NOT_IN_BATTERY` with its
reason -- the halo put and the input generator today.  The entries for the fused vector operators and K7d - K7h
(`_early_entries`), for K7i - K7k (`_one_pass_entries`) and for the halo forms and the gather (`_halo_entries`) are also
compared with plain numpy before the sweep, and tests/test_tunable_battery_entries.py
runs them on a machine without a GPU: through the host build of the ABI where it serves the entry, else on the oracle's double."""
import numpy as np
import pytest

from oracle import refimpl as R

pytestmark = pytest.mark.gpu

# name -> alternative values (the default is whatever the library starts with); values outside a kernel's template list fall
# back to a served one inside the library
ALTERNATIVES = {
    "seg": [8, 64], "nt_store": [0], "nt_load": [0], "seg_max_tiles": [1, 16], "scan_narrow_below": [0, 1 << 30], "pad_rows": [0],
    "pad_nt": [0, 1, 2, 4], "transform_lds_kb": [16, 32], "transform_win": [0], "transform_fast": [0], "transform_stage": [0, 1, 2],
    "transform_ring": [4, 16], "transform_cwin": [0, 4], "zchunk": [0, 16, 1024], "zband": [0], "zb_rows": [4, 8, 32], "scan_block": [64, 128, 512, 1024],
    "strided_gen": [0], "march_band": [0], "scan_vec": [0], "scan_dpp": [0], "contig_gen": [0], "deep_waves": [0, 1 << 30], "contig_rw": [0, 1],
    "rw_zshare": [0], "met_zk": [1, 2], "met_zk1": [1, 4], "vec_zk": [1, 4], "vec_nt": [0, 1, 2], "vec_zb_rows": [8, 32], "nb_dpp": [0],
    "met_zk2": [1, 2], "met_ys": [0], "seg_ys": [0], "contig_rw_mi": [2, 8], "met_seg": [1, 2], "met_seg1": [1, 4], "met_scalar": [0],
    "scan_pipe": [0, 2], "scan_u": [8, 16, 24], "scan_pace": [1], "scan_chain": [0, 2, 3], "scan_chain_w": [2, 104], "scan_chain_tmaj": [1, 4],
    "reduce_zl": [1, 4], "met_ys1": [0, 4], "met_ys2": [0, 6], "transform_lean": [0, 1, 2], "pad_tpw": [1, 4], "bin_idx32": [0],
    "reduce_ldsw_u": [8, 16], "march_ofast": [0], "reduce_sk": [0, 2], "reduce_ru": [0, 2], "reduce_wfast": [0], "reduce_wg": [0, 1, 8, 16, 25],
    "scan_sh1": [0], "reduce_zmarch": [0, 208, 308, 312, 316, 408, 1308, 1316], "reduce_ldsw": [0, 1], "march_lds_kb": [32],
}
NOT_SWEPT = {"scan_chain_spin": "forces the rescue path: tests/test_gpu_chain_rescue.py", "dbg": "debug switches of single experiments"}
# entries of the C ABI (without their _f64 / _f32 suffix) that no battery call reaches, and why: the test fails for an entry that
# is neither reached nor named here, and for a name here that is reached or no longer exists
NOT_IN_BATTERY = {
    "xg_halo_put": "writes halo slabs into a padded array: it reads no tunable (through Grid's padding: tests/test_topology.py)",
    "xg_fill_synthetic": "the benchmark's input generator, no operator: tests/test_gpu_kernels.py compares it with the oracle",
}


def _battery(D, dtype, references=None):
    """name -> (thunk, exact?) ; small shapes that still cross the thresholds (long marches >= 256 rows, rows >= 3 groups,
    >= 3 levels with level-shared metrics, unaligned row lengths).  `references`: a dict that receives name -> numpy
    reference thunk for the entries that have one"""
    f = lambda shape, seed: R.synthetic_field(shape, seed).astype(dtype)  # noqa: E731
    m = lambda shape, seed: R.synthetic_metric(shape, seed).astype(dtype)  # noqa: E731
    a, odd = _battery_fields(dtype)
    wide = f((2, 4, 40, 4100), 3)
    mxy, mxy2, mz, my = m((1, 300, 264), 4), m((1, 300, 264), 5), m((5, 1, 1), 6), m((1, 300, 1), 7)
    calls = {}
    for op in ("diff", "interp", "max"):
        for ax, bc in ((2, "periodic"), (1, "extend"), (0, "fill")):
            calls[f"{op}{ax}"] = (lambda op=op, ax=ax, bc=bc: D.stencil1d(op, a, ax, 1, 0, bc, 1.5), True)
            calls[f"{op}{ax}odd"] = (lambda op=op, ax=ax, bc=bc: D.stencil1d(op, odd, ax, 0, 1, bc, 1.5), True)
        calls[f"{op}w"] = (lambda op=op: D.stencil1d(op, wide, 3, 1, 0, "periodic"), True)
    for ax in (2, 1):
        calls[f"deriv{ax}"] = (lambda ax=ax: D.stencil1d("diff", a, ax, 1, 0, "extend", 0.0, None, mxy), True)
        calls[f"mw{ax}"] = (lambda ax=ax: D.stencil1d("interp", a, ax, 1, 0, "periodic", 0.0, mxy, mxy2), True)
    calls["deriv0"] = (lambda: D.stencil1d("diff", a, 0, 1, 0, "fill", 0.0, None, mz), True)
    calls["mwy1d"] = (lambda: D.stencil1d("diff", a, 1, 1, 0, "extend", 0.0, my, None), True)
    for ax in (0, 1, 2):
        exact = ax != 2
        calls[f"cum{ax}"] = (lambda ax=ax: D.cumsum1d(a, ax, 0, 1, 1, 0, "fill"), exact)
        calls[f"cum{ax}r"] = (lambda ax=ax: D.cumsum1d(a, ax, 1, 0, 0, 1, "extend", 0.0, True, True), exact)
        calls[f"cumint{ax}"] = (lambda ax=ax: D.cumsum1d(a, ax, 0, 1, 1, 0, "fill", 0.0, False, True, mxy if ax else mz, None), exact)
        calls[f"cum{ax}odd"] = (lambda ax=ax: D.cumsum1d(odd, ax, 0, 0, 0, 0, None), exact)
        for mode in (True, False, "valid", "mean_valid", "pair_all"):
            calls[f"sum{ax}{mode}"] = (lambda ax=ax, mode=mode: D.reduce1d(a, ax, mxy if ax else mz, mode), exact)
        calls[f"sum{ax}plain"] = (lambda ax=ax: D.reduce1d(a, ax, None), exact)
    calls["sumw"] = (lambda: D.reduce1d(wide, 3, None), False)
    calls["pad"] = (lambda: D.pad_nd(odd, {2: (1, 2), 1: (2, 0)}, {2: "periodic", 1: "extend"}, {2: 0.0, 1: 0.0}), True)
    calls["padz"] = (lambda: D.pad_nd(a, {0: (1, 1)}, {0: "fill"}, {0: 3.0}), True)
    calls["mul"] = (lambda: D.binary("mul", a, mxy), True)
    calls["div"] = (lambda: D.binary("div", a, mz), True)
    # the fused vector operators and the one-pass operators K7d - K7h
    for k, (fn, reference) in _early_entries(D, dtype).items():
        assert k not in calls
        calls[k] = (fn, True)
        if references is not None:
            references[k] = reference
    phi = f((20, 24, 128), 11)
    theta = np.cumsum(R.synthetic_field((20, 24, 128), 12).astype(dtype) + dtype(0.55), axis=0)
    theta_o = np.cumsum(R.synthetic_field((21, 24, 128), 13).astype(dtype) + dtype(0.55), axis=0)
    calls["tlin"] = (lambda: D.transform_linear(phi, theta, np.linspace(0.5, 9.0, 12).astype(dtype).reshape(12, 1, 1), 0), True)
    calls["tcon"] = (lambda: D.transform_conservative(phi, theta_o, np.linspace(0.0, 12.0, 14).astype(dtype), 0), True)
    # K7i - K7k; the pre-gathered halo forms and the gather
    for k, (fn, reference) in list(_one_pass_entries(D, dtype).items()) + list(_halo_entries(D, dtype).items()):
        assert k not in calls
        calls[k] = (fn, True)
        if references is not None:
            references[k] = reference
    return calls


def _early_entries(D, dtype, V=None):
    """name -> (thunk, reference) for the fused vector operators (`vort`, `divg`, `grad`, `flux`), the two-axis stencil
    (`i2`, `i2mw`) and the one-pass operators K7d - K7h: level-shared (1, Y, X) planes (band-major work order under the
    defaults; no tag), metrics of the fields' own shape (the plain order; tag "u": unshared) and the 3-D entries.  The thunk
    calls `D` on inputs uploaded once, the reference gives the plain numpy result of the same call over the host copies of
    the same inputs, by the numpy statements of the operators' CPU suites.  Every entry is exact.  `V`: the module that
    serves the vector operators and the two-axis stencil (the CPU twin passes the oracle's double, since the host build of the
    ABI has the one-axis and the one-pass operators only); `D` by default"""
    import types

    import test_flux_divergence_3d as T3
    import test_momentum_advection as TM
    import test_vertical_velocity as TV
    from test_fused_second_order import _want_flux_div, _want_laplacian

    f = lambda shape, seed: R.synthetic_field(shape, seed).astype(dtype)  # noqa: E731
    m = lambda shape, seed: R.synthetic_metric(shape, seed).astype(dtype)  # noqa: E731
    dev = lambda x: D.asdevice(x)  # noqa: E731
    u, v = f((6, 64, 256), 8), f((6, 64, 256), 9)
    area = m((1, 64, 256), 10)
    zero = {"X": 0.0, "Y": 0.0}
    V = D if V is None else V
    out = {}
    out["vort"] = (lambda: V.vorticity(u, v, area, "fill", "fill"), lambda: [R.vorticity(u, v, area, "fill", "fill")])
    out["divg"] = (lambda: V.divergence(u, v, area, "periodic", "extend"), lambda: [R.divergence(u, v, area, "periodic", "extend")])
    out["grad"] = (lambda: V.gradient(u, "periodic", "extend", 0.0, 0.0, area, area),
                   lambda: list(R.gradient(u, "periodic", "extend", 0.0, 0.0, area, area)))
    out["flux"] = (lambda: V.flux(u, v, u, "periodic", "extend"), lambda: list(R.flux(u, v, u, "periodic", "extend")))
    # the two-axis stencil: the two one-axis operators one after the other, X then Y; weighted: times the metric at the
    # current position before each axis, divided by the one at the new position after it
    out["i2"] = (lambda: V.stencil2d("interp", u, 0, (1, 0), "periodic", 0.0, (1, 0), "extend", 0.0),
                 lambda: [R.stencil1d("interp", R.stencil1d("interp", u, 2, 1, 0, "periodic", 0.0), 1, 1, 0, "extend", 0.0)])
    out["i2mw"] = (lambda: V.stencil2d("interp", u, 0, (1, 0), "periodic", 0.0, (1, 0), "extend", 0.0, (area[0], area[0], area[0])),
                   lambda: [R.stencil1d("interp", R.stencil1d("interp", u, 2, 1, 0, "periodic", 0.0, area[0], area[0]), 1, 1, 0,
                                        "extend", 0.0, area[0], area[0])])
    du, dv = dev(u), dev(v)
    fill = {"X": 1.5, "Y": -0.5, "Z": 0.25}
    shared = [m((1, 64, 256), 20 + k) for k in range(5)]
    full = [m((6, 64, 256), 30 + k) for k in range(5)]
    for tag, planes in (("", shared), ("u", full)):   # "u": unshared metrics
        m0, m1, m2, m3, m4 = planes
        d0, d1, d2, d3, d4 = (dev(x) for x in planes)
        cor = f(tuple(m0.shape), 40) * dtype(3.0)
        dcor = dev(cor)
        out["fdiv" + tag] = (lambda d4=d4: D.flux_divergence(du, dv, du, d4, "periodic", "extend", 1.5, -0.5),
                             lambda m4=m4: [_want_flux_div(u, v, u, "periodic", "extend", m4, fill=fill)])
        met = {"dxC": m0, "dyC": m1, "dyG": m2, "dxG": m3, "rA": m4}
        out["lap" + tag] = (lambda d=(d0, d1, d2, d3, d4): D.laplacian(du, "fill", "periodic", 1.5, -0.5, *d),
                            lambda met=met: [_want_laplacian(u, "fill", "periodic", met, fill=fill)])
        one = np.ones((), dtype=dtype)   # (x / 1 and x * 1 are exact: the chain with the area alone)
        only = {"dxC": one, "dyC": one, "dyG": one, "dxG": one, "rA": m4}
        out["lapa" + tag] = (lambda d4=d4: D.laplacian(du, "extend", "fill", 1.5, -0.5, area=d4),
                             lambda only=only: [_want_laplacian(u, "extend", "fill", only, fill=fill)])
        ds = {k: types.SimpleNamespace(values=x) for k, x in (("rAz", m0), ("dxC", m1), ("dyC", m2))}
        out["madv" + tag] = (lambda d=(dcor, d0, d1, d2): D.momentum_advection(du, dv, *d, "periodic", "fill", 1.5, -0.5),
                             lambda ds=ds, cor=cor: list(TM._want(u, v, "periodic", "fill", ds, cor, fill=fill)))
    out["madv0"] = (lambda: D.momentum_advection(du, dv, None, None, None, None, "extend", "periodic"),
                    lambda: list(TM._want(u, v, "extend", "periodic", None, None, fill=zero)))
    out["ke"] = (lambda: D.kinetic_energy(du, dv, "fill", "extend", 1.5, -0.5), lambda: [TM._want_ke(u, v, "fill", "extend", fill=fill)])
    h3 = [f((2, 6, 64, 256), 50 + k) for k in range(4)]
    u3, v3, w3, t3 = (dev(x) for x in h3)
    hm = [m((1, 6, 64, 256), 60 + k) for k in range(5)]
    vol, vol2, mu, mv, ar3 = (dev(x) for x in hm)
    hdrf, hra = m((1, 6, 1, 1), 66), m((1, 1, 64, 256), 67)
    drf, ra = dev(hdrf), dev(hra)
    mul = lambda a, b: R.binary("mul", a, b)  # noqa: E731
    out["fdiv3"] = (lambda: D.flux_divergence_3d(u3, v3, w3, t3, vol, vol2, "periodic", "extend", "fill", 1.5, -0.5, 0.25),
                    lambda: [T3._want(*h3, "periodic", "extend", "fill", mul(hm[0], hm[1]), fill=fill)])
    out["fdiv3p"] = (lambda: D.flux_divergence_3d(u3, v3, w3, t3, ra, drf, "fill", "periodic", "extend", 1.5, -0.5, 0.25),
                     lambda: [T3._want(*h3, "fill", "periodic", "extend", mul(hra, hdrf), fill=fill)])
    out["wcont"] = (lambda: D.vertical_velocity(u3, v3, mu, drf, mv, drf, ar3, "periodic", "extend", "fill", 1.5, -0.5, 0.25),
                    lambda: [TV._want(h3[0], h3[1], "periodic", "extend", "fill", False, faces=(mul(hm[2], hdrf), mul(hm[3], hdrf)),
                                      area=hm[4], fill=fill)])
    out["wcontr"] = (lambda: D.vertical_velocity(u3, v3, ra, drf, ra, drf, ra, "extend", "fill", "periodic", 1.5, -0.5, 0.25, True),
                     lambda: [TV._want(h3[0], h3[1], "extend", "fill", "periodic", True, faces=(mul(hra, hdrf), mul(hra, hdrf)),
                                       area=hra, fill=fill)])
    return out


# K7i - K7k.  ny = 29: 15 two-row segments, the last of one row, ragged against bands of 1, 2, 4 and 8 segments (vec_zb_rows
# 8 / 16 / 32, halved with four planes and quartered with eight).  nx = 260: the vector form, V = 2 in float64 (three tiles of
# 128 columns, the last 4 wide) and V = 4 in float32 (two tiles of 256, the last one lane wide), so lane 63 has its neighbour in
# the next tile of the same row; nx = 259: the narrow form, five tiles, the last 3 wide.
OP_NY, OP_NXS, OP_LEAD3, OP_NZ, OP_LEAD2 = 29, (260, 259), 2, 6, 3
OP_FILL = {"X": 1.75, "Y": -0.625, "Z": 0.375}
HV_PLANES = ("rA", "rAz", "dxC", "dyC", "dyG", "dxG", "nu_d", "nu_z")
# every triple holds a periodic, an extend and a fill side; K7i pads Z with fill or extend only
PADS_K7I = [("periodic", "extend", "fill"), ("periodic", "fill", "extend"), ("extend", "periodic", "fill"),
            ("fill", "periodic", "extend")]
PADS_K7J = [("fill", "extend", "periodic"), ("extend", "fill", "periodic"), ("extend", "periodic", "fill"),
            ("periodic", "fill", "extend"), ("fill", "periodic", "extend"), ("periodic", "extend", "fill")]
PADS_K7K = [("periodic", "extend"), ("extend", "fill"), ("fill", "periodic"), ("periodic", "fill"), ("fill", "extend"),
            ("extend", "periodic")]


def _one_pass_entries(D, dtype):
    """name -> (thunk, reference) for K7i `hydrostatic_pressure_gradient`, K7j `vertical_momentum_advection` and K7k
    `horizontal_viscosity`: the thunk calls `D` on inputs uploaded once, the reference gives the plain numpy result of the
    same call (the `_want` of the operator's CPU test).  Every entry is exact.  The K7k entries whose planes are (1, Y, X)
    take the band-major order under the defaults; that all their planes have a leading extent of 1 under at least two
    fields is asserted here, that `zband` is on by the test that sweeps them."""
    import types

    import test_horizontal_viscosity as TH
    import test_pressure_gradient as TP
    import test_vertical_momentum_advection as TM

    f = lambda shape, seed: R.synthetic_field(shape, seed).astype(dtype)  # noqa: E731
    m = lambda shape, seed: R.synthetic_metric(shape, seed).astype(dtype)  # noqa: E731
    dev = lambda x: None if x is None else D.asdevice(x)  # noqa: E731
    fx, fy, fz = OP_FILL["X"], OP_FILL["Y"], OP_FILL["Z"]
    out = {}
    ni = nj = nk = 0
    for nx in OP_NXS:
        s3 = (OP_LEAD3, OP_NZ, OP_NY, nx)
        b, u3, v3, w3 = (f(s3, 110 + k) for k in range(4))
        # a few NaN cells: corners, the last row, both sides of the lane-63 seam
        b[0, 0, 0, 0] = b[1, 2, 14, 63] = b[1, 5, 28, nx - 1] = np.nan
        u3[0, 1, 7, 63] = u3[1, 5, 28, 0] = np.nan
        v3[1, 0, 28, nx - 1] = v3[0, 3, 0, 64] = np.nan
        w3[0, 0, 13, 64] = w3[1, 5, 0, nx - 1] = w3[0, 2, 28, 127] = np.nan
        db, du3, dv3, dw3 = dev(b), dev(u3), dev(v3), dev(w3)
        zs, ps = (1, OP_NZ, 1, 1), (1, 1, OP_NY, nx)
        forms = {"shared": (m(zs, 120), m(ps, 121), m(ps, 122)), "own": (m(s3, 123), m(s3, 124), m(s3, 125))}
        for tag, (wz, mx, my) in forms.items():
            # K7i: the Z weight, dxC, dyC
            px, py, pz = PADS_K7I[ni % len(PADS_K7I)]
            ni += 1
            out[f"pgrad{nx}{tag}"] = (
                lambda p=(px, py, pz), d=(dev(wz), dev(mx), dev(my)), db=db: D.hydrostatic_pressure_gradient(db, *d, *p, fx, fy, fz),
                lambda p=(px, py, pz), wz=wz, mx=mx, my=my, b=b: TP._want(b, wz, *p, fill=OP_FILL, mx=mx, my=my))
            # K7j: the Z metric at u's and at v's points ("shared": drF(Z) for both, as Grid passes it)
            mu, mv = (wz, wz) if tag == "shared" else (mx, my)
            px, py, pz = PADS_K7J[nj % len(PADS_K7J)]
            nj += 1
            out[f"vmadv{nx}{tag}"] = (
                lambda p=(px, py, pz), d=(dev(mu), dev(mv)), fl=(du3, dv3, dw3): D.vertical_momentum_advection(*fl, *d, *p, fx, fy, fz),
                lambda p=(px, py, pz), mu=mu, mv=mv, fl=(u3, v3, w3): TM._want(*fl, *p, fill=OP_FILL, mu=mu, mv=mv))
        if nx == OP_NXS[0]:   # one unweighted call each, in the vector form
            px, py, pz = PADS_K7I[ni % len(PADS_K7I)]
            ni += 1
            out[f"pgrad{nx}plain"] = (
                lambda p=(px, py, pz), db=db: D.hydrostatic_pressure_gradient(db, None, None, None, *p, fx, fy, fz),
                lambda p=(px, py, pz), b=b: TP._want(b, None, *p, fill=OP_FILL))
            px, py, pz = PADS_K7J[nj % len(PADS_K7J)]
            nj += 1
            out[f"vmadv{nx}plain"] = (
                lambda p=(px, py, pz), fl=(du3, dv3, dw3): D.vertical_momentum_advection(*fl, None, None, *p, fx, fy, fz),
                lambda p=(px, py, pz), fl=(u3, v3, w3): TM._want(*fl, *p, fill=OP_FILL))
        # K7k: the six metrics and both coefficients / the metrics alone, as level-shared planes and with the fields' own
        # shape; no planes at all
        s2 = (OP_LEAD2, OP_NY, nx)
        u2, v2 = f(s2, 130), f(s2, 131)
        u2[0, 0, 0] = u2[1, 28, 63] = u2[2, 14, nx - 1] = np.nan
        v2[0, 13, 64] = v2[2, 28, 0] = np.nan
        du2, dv2 = dev(u2), dev(v2)
        for tag, ps in (("shared", (1, OP_NY, nx)), ("own", s2)):
            vals = {p: (m(ps, 140 + k) if k < 6 else f(ps, 140 + k) * dtype(3.0)) for k, p in enumerate(HV_PLANES)}
            for sub, present in (("all", HV_PLANES), ("met", HV_PLANES[:6])):
                if tag == "shared":   # what `fused_band` asks of a call before it bands it
                    assert all(vals[p].shape[0] == 1 for p in present) and s2[0] >= 2
                px, py = PADS_K7K[nk % len(PADS_K7K)]
                nk += 1
                planes = [vals[p] if p in present else None for p in HV_PLANES]
                ds = {p: types.SimpleNamespace(values=vals[p]) for p in present[:6]}
                nu = tuple(planes[6:])
                out[f"hvisc{nx}{tag}{sub}"] = (
                    lambda p=(px, py), d=[dev(x) for x in planes], fl=(du2, dv2): D.horizontal_viscosity(*fl, *d, *p, fx, fy),
                    lambda p=(px, py), ds=ds, nu=nu, fl=(u2, v2): TH._want(*fl, *p, ds, nu, fill=OP_FILL))
        px, py = PADS_K7K[nk % len(PADS_K7K)]
        nk += 1
        out[f"hvisc{nx}plain"] = (
            lambda p=(px, py), fl=(du2, dv2): D.horizontal_viscosity(*fl, *([None] * 8), *p, fx, fy),
            lambda p=(px, py), fl=(u2, v2): TH._want(*fl, *p, None, (None, None), fill=OP_FILL))
    return out


def _battery_fields(dtype):
    """the battery's own `a` (a march of 300 rows, one NaN cell) and `odd` (odd, unaligned rows)"""
    a = R.synthetic_field((5, 300, 264), 1).astype(dtype)
    a[1, 7, 9] = np.nan
    return a, R.synthetic_field((3, 65, 131), 2).astype(dtype)


def _halo_entries(D, dtype, V=None):
    """name -> (thunk, reference) for the pre-gathered halo forms and the gather: the four vector forms at (3, 29, 260) and
    (3, 29, 259), area / metrics level-shared in one and of the fields' own shape in the other, the seven mode pairs that
    contain a halo rotating; `stencil1d_halo` and `stencil1d_halo_w` on the battery's `a` and `odd` along each axis, the
    operators, the pads and the metric forms rotating; the three gather cases.  Inputs are uploaded once; the references are
    the plain numpy statements of tests/test_halo_forms.py; every entry is exact.  `V`: the module that serves the vector
    forms and the gather (the CPU twin passes the oracle's double, since the host build of the ABI has the two stencil forms
    only); `D` by default"""
    import test_halo_forms as TH

    V = D if V is None else V
    out = {}
    pairs = iter(TH.PAIRS * 2)
    for nx, form in zip(OP_NXS, ("shared", "own")):
        case = TH.VectorCase(OP_NY, nx, (OP_LEAD2,), dtype)
        if form == "shared":   # what `fused_band` asks of a call before it bands it
            assert TH.area_shape(form, case.lead, OP_NY, nx)[0] == 1 and case.lead[0] >= 2
        for op in ("vorticity", "divergence", "gradient", "flux"):
            planes = {"gradient": (case.area(form, 331), case.area(form, 332)), "flux": ()}.get(op, (case.area(form),))
            bx, by = next(pairs)
            resident = {k: V.asdevice(x) for k, x in case.sets[op].items()}
            dplanes = tuple(V.asdevice(p) for p in planes)
            out[f"h{op[:4]}{nx}{form}"] = (
                lambda case=case, op=op, p=(bx, by), d=dplanes, r=resident: case.call(V, op, *p, d, r),
                lambda case=case, op=op, p=(bx, by), planes=planes: list(case.want(op, *p, planes)))
    n = 0
    for tag, x in zip(("a", "odd"), _battery_fields(dtype)):
        xd = D.asdevice(x)
        for axis in range(x.ndim):
            for weighted in (False, True):
                op, (lo, hi) = TH.OPS[n % 4], TH.STENCIL_PADS[n % 3]
                hshape, oshape = list(x.shape), list(x.shape)
                hshape[axis], oshape[axis] = lo + hi, x.shape[axis] + lo + hi - 1
                halo = R.synthetic_field(tuple(hshape), 150 + n).astype(dtype)
                halo.reshape(-1)[[0, -1]] = np.nan
                m_in = R.synthetic_metric(TH._m_shape(TH.M_IN[1 + (n // 2) % 4], x.shape, axis), 170 + n).astype(dtype) if weighted else None
                m_out = R.synthetic_metric(TH._m_shape(TH.M_OUT[1 + n % 2], oshape, axis), 190 + n).astype(dtype) if n % 3 else None
                dev = lambda q: None if q is None else D.asdevice(q)  # noqa: E731
                out[f"hst{'w' if weighted else ''}{tag}{axis}"] = (
                    lambda a=(op, xd, dev(halo), axis, lo, hi, dev(m_out), dev(m_in)): D.stencil1d_halo(*a),
                    lambda a=(op, x, halo, axis, lo, hi, m_out, m_in): [TH.want_stencil(*a)])
                n += 1
    for k in range(len(TH.GATHER_CASES)):
        x, partner, args, want = TH.gather_case(k, dtype)
        dx, dp, tok = V.asdevice(x), (None if partner is None else V.asdevice(partner)), V.upload_tokens(args[0])
        out[f"hgather{k}"] = (lambda dx=dx, dp=dp, tok=tok, rest=args[1:]: V.gather(dx, dp, tok, *rest), lambda want=want: [want])
    return out


def _run(D, calls):
    out = {}
    for k, (fn, _) in calls.items():
        r = fn()
        out[k] = [D.tohost(x) for x in r] if isinstance(r, tuple) else [D.tohost(r)]
    return out


class _Recorder:
    """the library with every entry that is fetched from it noted down"""

    def __init__(self, lib):
        self._lib, self.fetched = lib, set()

    def __getattr__(self, name):
        self.fetched.add(name)
        return getattr(self._lib, name)


def _same_bits(got, want):
    """NaN where the other has NaN; everywhere else the same bit pattern (-0.0 is not +0.0)"""
    if got.dtype != want.dtype or got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    nan = np.isnan(want)
    return np.array_equal(np.where(nan, 0, got).view(bits), np.where(nan, 0, want).view(bits))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_every_tunable_value_computes_the_same(dtype, monkeypatch):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import warnings

    from xgcm_amd import _hip
    from xgcm_amd import device as D

    assert _hip.get_tunable("zband") == 1   # the level-shared K7k entries of `_one_pass_entries` band under the defaults
    references = {}
    calls = _battery(D, dtype, references)
    # every wrapper of xgcm_amd.device fetches its entry from `_MEM.lib()`: the default run notes which ones the battery reaches
    rec = _Recorder(D._MEM.lib())
    with monkeypatch.context() as mp:
        mp.setattr(D._MEM, "lib", lambda: rec, raising=True)
        want = _run(D, calls)
    sfx = "_f64" if dtype is np.float64 else "_f32"
    abi = {n[:-4] for n in _hip.SIGNATURES if n.startswith("xg_") and n.endswith(sfx)}
    reached = {n[:-4] for n in rec.fetched if n.endswith(sfx)}
    assert abi - reached - set(NOT_IN_BATTERY) == set(), f"ABI entries that no battery call reaches: {sorted(abi - reached - set(NOT_IN_BATTERY))}"
    assert set(NOT_IN_BATTERY) <= abi - reached, f"stale NOT_IN_BATTERY names: {sorted(set(NOT_IN_BATTERY) - (abi - reached))}"
    # the new entries against plain numpy first, so that the sweep does not only compare the library with itself
    # K7i - K7k; eight vector halo entries, twelve stencil halo entries, three gathers; the vector operators and K7d - K7h
    assert len(references) == 20 + 23 + 20
    for k, reference in references.items():
        ref = reference()
        assert len(ref) == len(want[k]) and all(_same_bits(g, w) for g, w in zip(want[k], ref)), f"{k}: the default result is not numpy's"
    rtol = 1e-12 if dtype is np.float64 else 2e-5
    names = set(ALTERNATIVES) | set(NOT_SWEPT)
    import os
    import re

    known = set(re.findall(r'\{"(\w+)", &Tune::', open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                       "xgcm_amd", "csrc", "xg_runtime.hip")).read()))
    assert known == names, f"tunables without a sweep entry: {sorted(known - names)}; entries without a tunable: {sorted(names - known)}"
    bad = []
    for name, values in ALTERNATIVES.items():
        before = _hip.get_tunable(name)
        try:
            for val in values:
                _hip.set_tunable(name, val)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    got = _run(D, calls)
                for k, (_, exact) in calls.items():
                    for g, w in zip(got[k], want[k]):
                        ok = g.shape == w.shape and (np.array_equal(g, w, equal_nan=True) if exact
                                                     else np.allclose(g, w, rtol=rtol, atol=rtol * 300, equal_nan=True))
                        if not ok:
                            bad.append((name, val, k))
        finally:
            _hip.set_tunable(name, before)
    torch.cuda.synchronize()
    _hip.chain_rearm()
    assert not bad, bad[:20]
