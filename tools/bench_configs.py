#!/usr/bin/env python3
"""All BASELINE.json configs (2-5) at full size through the public Grid API, on 1..N MI355X.

    python tools/bench_configs.py [--gpus N] [--reps 7] [--records 360] [--configs 2,3,4,5]

Not the judged bench line (that is bench.py = config 2); this is the per-config evidence table:
ms, Gcell/s, algorithmic GB/s (bytes/cell of SURVEY.md section 8(d)) and fraction of 8 TB/s.

Configs 4 and 5 are the SHARDED runs of BASELINE.json; `--gpus N` starts N
ranks (re-executing itself under torch.distributed.run when no launcher did, exactly like bench.py):
  4   cumsum(T,'Z') center->left and center->outer over `--records` records of 3600x2400x75 f64 (360 =
      1.866 TB), the record axis split over the ranks by `sharding.shard_bounds` (360 -> 45 per GPU on 8),
      each rank walking its block in HBM-resident batches sized from its free HBM;
  5   fused and unfused vorticity (diff(V,'X') - diff(U,'Y')) / rAz, `fill`, on 4320x4320x90 split along Z
      (90 -> 12,12,11,11,11,11,11,11 on 8 GPUs), rAz replicated.
No data-path collective: RCCL carries barriers, the max-over-ranks time and a checksum of checksums.
Single-GPU extras: 4x (> 2^32-cell batch checks), 5x (divergence / gradient / flux; flux_divergence / laplacian / flux_divergence_3d / vertical_velocity / kinetic_energy / momentum_advection / hydrostatic_pressure_gradient / vertical_momentum_advection / horizontal_viscosity / vertical_diffusion / richardson_number against their chains, implicit_vertical_diffusion against its level loop; 5pg, 5vm, 5hv, 5vd, 5iv, 5ri: the last six pairs, each alone; 5vv: implicit_vertical_viscosity against its chain of four calls, alone only; 5pp: richardson_mixing against its chain, alone only; 5is: isopycnal_slope against its chain, alone only; 5rt: redi_tensor against its chain, alone or after 5is; 5rf: redi_vertical_flux_divergence against its chain, alone only; 5bv: bolus_velocity against its chain, alone only; 5ru: redi_horizontal_tensor against its chain, alone only), f1, f2, f4, llc, pcie, stream.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import time  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from xgcm_amd import DataArray, Dataset, Grid  # noqa: E402
from xgcm_amd import device as D  # noqa: E402
from xgcm_amd import sharding as S  # noqa: E402


def timeit(fn, reps):
    """median device time of `fn` over `reps` back-to-back launches (events on the launch stream), after a
    warm-up of at least 0.15 s so that the first op of a config is not timed on ramping clocks"""
    import time

    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    while time.perf_counter() - t0 < 0.15:
        fn()
        torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ts = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(reps))
    return ts[len(ts) // 2]


def timeit_interleaved(fa, fb, reps):
    """medians of `fa` and `fb` timed in turns (a, b, a, b, ...) in one process: both see the same clocks and neighbours"""
    import time

    t0 = time.perf_counter()
    while True:
        fa()
        fb()
        torch.cuda.synchronize()
        if time.perf_counter() - t0 >= 0.15:
            break
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps + 1)]
    ev[0].record()
    for i in range(reps):
        fa()
        ev[2 * i + 1].record()
        fb()
        ev[2 * i + 2].record()
    torch.cuda.synchronize()
    ta = sorted(ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(reps))
    tb = sorted(ev[2 * i + 1].elapsed_time(ev[2 * i + 2]) for i in range(reps))
    return ta[len(ta) // 2], tb[len(tb) // 2]


def timeit_rounds(fa, fb, reps):
    """`fa` and `fb` timed in turns as timeit_interleaved does, every round kept: ([ms of fa], [ms of fb])"""
    fa()
    fb()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps + 1)]
    ev[0].record()
    for i in range(reps):
        fa()
        ev[2 * i + 1].record()
        fb()
        ev[2 * i + 2].record()
    torch.cuda.synchronize()
    return ([ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(reps)],
            [ev[2 * i + 1].elapsed_time(ev[2 * i + 2]) for i in range(reps)])


def run_pressure_gradient(reps, nz=90, n=4320):
    """hydrostatic_pressure_gradient in one pass against its chain of three launches (cumint to the outer position, interp,
    gradient) on the MITgcm grid (drF, dxC, dyC; periodic / extend / fill), timed in turns, every paired round reported"""
    grid = mitgcm_grid(nz, n, n)
    B = DataArray(D.synthetic((nz, n, n), 56), ("Z", "YC", "XC"))
    cells = nz * n * n

    def chain():
        pc = grid.interp(grid.cumint(B, "Z", to="outer"), "Z")
        return grid.gradient(pc, metric_weighted=True)

    gx, gy = grid.hydrostatic_pressure_gradient(B)
    wx, wy = chain()
    ok = bool(torch.equal(gx.data, wx.data) and torch.equal(gy.data, wy.data))
    del gx, gy, wx, wy
    torch.cuda.empty_cache()
    tf, tc = timeit_rounds(lambda: grid.hydrostatic_pressure_gradient(B), chain, max(3, reps // 2))
    med = lambda t: sorted(t)[len(t) // 2]  # noqa: E731
    rec(5, "hydrostatic_pressure_gradient fused gradient(interp(cumint(b, Z), Z)) / (dxC, dyC), periodic/extend/fill: 1 read + 2 writes", med(tf), cells, 24 + 16 / nz)
    rec(5, "hydrostatic_pressure_gradient as its chain (3 launches), fused-equivalent bytes", med(tc), cells, 24 + 16 / nz)
    print(json.dumps({"config": 5, "check": "fused hydrostatic_pressure_gradient == chain bit for bit at full size", "ok": ok,
                      "speedup": round(med(tc) / med(tf), 2), "rounds_ms_fused": [round(t, 3) for t in tf],
                      "rounds_ms_chain": [round(t, 3) for t in tc],
                      "fused_below_chain_in_every_round": all(a < b for a, b in zip(tf, tc))}), flush=True)


def run_vertical_momentum_advection(reps, nz=90, n=4320):
    """vertical_momentum_advection in one pass against its chain of twelve launches (two interps of w, two diffs along Z, two
    products, two interps along Z, two negations, two divisions by drF) on the MITgcm grid (periodic / extend / fill), timed
    in turns, every paired round reported"""
    grid = mitgcm_grid(nz, n, n)
    U = DataArray(D.synthetic((nz, n, n), 57), ("Z", "YC", "XG"))
    V = DataArray(D.synthetic((nz, n, n), 58), ("Z", "YG", "XC"))
    W = DataArray(D.synthetic((nz, n, n), 59), ("Zl", "YC", "XC"))
    cells = nz * n * n

    def chain():
        wu, wv = grid.interp(W, "X"), grid.interp(W, "Y")
        du, dv = grid.diff(U, "Z"), grid.diff(V, "Z")
        gu, gv = -grid.interp(wu * du, "Z"), -grid.interp(wv * dv, "Z")
        return gu / grid.get_metric(gu, ("Z",)), gv / grid.get_metric(gv, ("Z",))

    gu, gv = grid.vertical_momentum_advection(U, V, W)
    wu, wv = chain()
    ok = bool(torch.equal(gu.data, wu.data) and torch.equal(gv.data, wv.data))
    del gu, gv, wu, wv
    torch.cuda.empty_cache()
    tf, tc = timeit_rounds(lambda: grid.vertical_momentum_advection(U, V, W), chain, max(3, reps // 2))
    med = lambda t: sorted(t)[len(t) // 2]  # noqa: E731
    rec(5, "vertical_momentum_advection fused -interp(interp(w, X / Y) * diff(u / v, Z), Z) / drF, periodic/extend/fill: 3 reads + 2 writes", med(tf), cells, 40)
    rec(5, "vertical_momentum_advection as its chain (12 launches), fused-equivalent bytes", med(tc), cells, 40)
    print(json.dumps({"config": 5, "check": "fused vertical_momentum_advection == chain bit for bit at full size", "ok": ok,
                      "speedup": round(med(tc) / med(tf), 2), "rounds_ms_fused": [round(t, 3) for t in tf],
                      "rounds_ms_chain": [round(t, 3) for t in tc],
                      "fused_below_chain_in_every_round": all(a < b for a, b in zip(tf, tc))}), flush=True)


def run_horizontal_viscosity(reps, nz=90, n=4320):
    """horizontal_viscosity in one pass against its chain of nine launches (divergence, vorticity, two products with the
    coefficient planes, gradient, two derivatives of zeta, two combinations) with the six 2-D metric planes and both 2-D
    coefficient planes (periodic / extend), timed in turns, every paired round reported"""
    coords = {"XC": ("XC", np.arange(n) + 0.5), "XG": ("XG", np.arange(n) * 1.0), "YC": ("YC", np.arange(n) + 0.5),
              "YG": ("YG", np.arange(n) * 1.0), "Z": ("Z", np.arange(nz) + 0.5)}
    m = lambda seed, dims: DataArray(D.synthetic((n, n), seed, 0, 1000.0, 1000.0), dims)  # noqa: E731
    ds = Dataset({"dxC": m(31, ("YC", "XG")), "dyC": m(32, ("YG", "XC")), "dyG": m(35, ("YC", "XG")), "dxG": m(36, ("YG", "XC")),
                  "rA": m(37, ("YC", "XC")), "rAz": m(33, ("YG", "XG"))}, coords)
    grid = Grid(ds, coords={"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"}},
                padding={"X": "periodic", "Y": "extend"}, autoparse_metadata=False,
                metrics={("X",): ["dxC", "dxG"], ("Y",): ["dyC", "dyG"], ("X", "Y"): ["rA", "rAz"]})
    U = DataArray(D.synthetic((nz, n, n), 51), ("Z", "YC", "XG"))
    V = DataArray(D.synthetic((nz, n, n), 52), ("Z", "YG", "XC"))
    ND = DataArray(D.synthetic((n, n), 38, 0, 50.0, 100.0), ("YC", "XC"))
    NZ = DataArray(D.synthetic((n, n), 39, 0, 50.0, 100.0), ("YG", "XG"))
    cells = nz * n * n

    def chain():
        div = grid.divergence(U, V) * ND
        zeta = grid.vorticity(U, V) * NZ
        dx, dy = grid.gradient(div, metric_weighted=True)
        return dx - grid.derivative(zeta, "Y"), dy + grid.derivative(zeta, "X")

    gu, gv = grid.horizontal_viscosity(U, V, ND, NZ)
    wu, wv = chain()
    ok = bool(torch.equal(gu.data, wu.data) and torch.equal(gv.data, wv.data))
    del gu, gv, wu, wv
    torch.cuda.empty_cache()
    tf, tc = timeit_rounds(lambda: grid.horizontal_viscosity(U, V, ND, NZ), chain, max(3, reps // 2))
    med = lambda t: sorted(t)[len(t) // 2]  # noqa: E731
    bpc = 32 + 64 / nz
    rec(5, "horizontal_viscosity fused (rA, rAz, dxC, dyC, dyG, dxG, nu_d, nu_z), periodic/extend: 2 reads + 2 writes", med(tf), cells, bpc)
    rec(5, "horizontal_viscosity as its chain (9 launches), fused-equivalent bytes", med(tc), cells, bpc)
    print(json.dumps({"config": 5, "check": "fused horizontal_viscosity == chain bit for bit at full size", "ok": ok,
                      "speedup": round(med(tc) / med(tf), 2), "rounds_ms_fused": [round(t, 3) for t in tf],
                      "rounds_ms_chain": [round(t, 3) for t in tc],
                      "fused_below_chain_in_every_round": all(a < b for a, b in zip(tf, tc))}), flush=True)


def run_vertical_diffusion(reps, nz=90, n=4320):
    """vertical_diffusion in one pass against its chain of three launches (derivative to Z:outer, the product with a 3-D
    kappa, derivative back to the centre; drC(Zp1), drF(Z); `extend`: no flux through the top and the bottom), timed in
    turns, every paired round reported"""
    coords = {"XC": ("XC", np.arange(n) + 0.5), "XG": ("XG", np.arange(n) * 1.0), "YC": ("YC", np.arange(n) + 0.5),
              "YG": ("YG", np.arange(n) * 1.0), "Z": ("Z", np.arange(nz) + 0.5), "Zp1": ("Zp1", np.arange(nz + 1) * 1.0)}
    ds = Dataset({"drF": DataArray(D.synthetic((nz,), 33, 0, 1000.0, 1000.0), ("Z",)),
                  "drC": DataArray(D.synthetic((nz + 1,), 34, 0, 1000.0, 1000.0), ("Zp1",))}, coords)
    grid = Grid(ds, coords={"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"},
                            "Z": {"center": "Z", "outer": "Zp1"}},
                padding={"X": "periodic", "Y": "extend", "Z": "extend"}, metrics={("Z",): ["drF", "drC"]}, autoparse_metadata=False)
    T = DataArray(D.synthetic((nz, n, n), 61), ("Z", "YC", "XC"))
    K = DataArray(D.synthetic((nz + 1, n, n), 62, 0, 50.0, 100.0), ("Zp1", "YC", "XC"))
    cells = nz * n * n

    def chain():
        return grid.derivative(grid.derivative(T, "Z", to="outer") * K, "Z")

    got, want = grid.vertical_diffusion(T, K), chain()
    ok = bool(torch.equal(got.data, want.data))
    del got, want
    torch.cuda.empty_cache()
    tf, tc = timeit_rounds(lambda: grid.vertical_diffusion(T, K), chain, max(3, reps // 2))
    med = lambda t: sorted(t)[len(t) // 2]  # noqa: E731
    bpc = 24 + 8 / nz   # a and out, nz + 1 levels of kappa
    rec(5, "vertical_diffusion fused derivative(derivative(a, Z, to=outer) * kappa, Z), 3-D kappa, drC / drF, extend: 2 reads + 1 write", med(tf), cells, bpc)
    rec(5, "vertical_diffusion as its chain (3 launches), fused-equivalent bytes", med(tc), cells, bpc)
    print(json.dumps({"config": 5, "check": "fused vertical_diffusion == chain bit for bit at full size", "ok": ok,
                      "speedup": round(med(tc) / med(tf), 2), "rounds_ms_fused": [round(t, 3) for t in tf],
                      "rounds_ms_chain": [round(t, 3) for t in tc],
                      "fused_below_chain_in_every_round": all(a < b for a, b in zip(tf, tc))}), flush=True)


def run_implicit_vertical_diffusion(reps, nz=90, n=4320):
    """implicit_vertical_diffusion in one pass (a forward and a backward sweep in one launch) against the level loop of
    xgcm_amd/grid.py (a dozen plane-sized operations per level and sweep) on resident tensors: 3-D kappa at Z:outer,
    drC(Zp1), drF(Z), timed in turns, every paired round reported"""
    from xgcm_amd.grid import _implicit_vertical_diffusion_levels as levels

    coords = {"XC": ("XC", np.arange(n) + 0.5), "XG": ("XG", np.arange(n) * 1.0), "YC": ("YC", np.arange(n) + 0.5),
              "YG": ("YG", np.arange(n) * 1.0), "Z": ("Z", np.arange(nz) + 0.5), "Zp1": ("Zp1", np.arange(nz + 1) * 1.0)}
    drf, drc = D.synthetic((nz,), 33, 0, 10.0, 10.0), D.synthetic((nz + 1,), 34, 0, 10.0, 10.0)
    ds = Dataset({"drF": DataArray(drf, ("Z",)), "drC": DataArray(drc, ("Zp1",))}, coords)
    grid = Grid(ds, coords={"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"},
                            "Z": {"center": "Z", "outer": "Zp1"}},
                padding={"X": "periodic", "Y": "extend", "Z": "extend"}, metrics={("Z",): ["drF", "drC"]}, autoparse_metadata=False)
    T = DataArray(D.synthetic((nz, n, n), 61), ("Z", "YC", "XC"))
    K = DataArray(D.synthetic((nz + 1, n, n), 62, 0, 0.1, 0.0), ("Zp1", "YC", "XC"))   # 0 .. 0.1 m2/s over 10 .. 20 m layers
    dt = 3600.0                                                                        # coupling dt kappa / (drC drF) <= 3.6
    cells = nz * n * n

    def loop():
        return levels(T.data, K.data, drc[:, None, None], drf[:, None, None], 0, dt)

    got, want = grid.implicit_vertical_diffusion(T, K, dt=dt), loop()
    ok = bool(torch.equal(got.data.view(torch.int64), want.view(torch.int64)))
    del got, want
    torch.cuda.empty_cache()
    tf, tc = timeit_rounds(lambda: grid.implicit_vertical_diffusion(T, K, dt=dt), loop, max(3, reps // 2))
    med = lambda t: sorted(t)[len(t) // 2]  # noqa: E731
    bpc = 56   # a, kappa, d out and back, c out and back, x (the 91st level of kappa is not counted)
    rec(5, "implicit_vertical_diffusion one pass (Thomas solve along Z), 3-D kappa, drC / drF: a, kappa, d and c out and back, x", med(tf), cells, bpc)
    rec(5, "implicit_vertical_diffusion as the level loop over planes, one-pass-equivalent bytes", med(tc), cells, bpc)
    print(json.dumps({"config": 5, "check": "one-pass implicit_vertical_diffusion == level loop bit for bit at full size", "ok": ok,
                      "speedup": round(med(tc) / med(tf), 2), "rounds_ms_fused": [round(t, 3) for t in tf],
                      "rounds_ms_loop": [round(t, 3) for t in tc],
                      "fused_below_loop_in_every_round": all(a < b for a, b in zip(tf, tc))}), flush=True)


def run_richardson_number(reps, nz=90, n=4320):
    """richardson_number in one pass against its chain of nine launches (three derivatives to Z:outer, two interps to the
    centre, two squares, their sum, the quotient; a profile drC(Zp1); periodic / extend / extend: no shear through the top
    and the bottom, where Ri is 0 / 0), timed in turns, every paired round reported"""
    coords = {"XC": ("XC", np.arange(n) + 0.5), "XG": ("XG", np.arange(n) * 1.0), "YC": ("YC", np.arange(n) + 0.5),
              "YG": ("YG", np.arange(n) * 1.0), "Z": ("Z", np.arange(nz) + 0.5), "Zp1": ("Zp1", np.arange(nz + 1) * 1.0)}
    ds = Dataset({"drC": DataArray(D.synthetic((nz + 1,), 34, 0, 10.0, 10.0), ("Zp1",))}, coords)
    grid = Grid(ds, coords={"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"},
                            "Z": {"center": "Z", "outer": "Zp1"}},
                padding={"X": "periodic", "Y": "extend", "Z": "extend"}, metrics={("Z",): ["drC"]}, autoparse_metadata=False)
    B = DataArray(D.synthetic((nz, n, n), 63), ("Z", "YC", "XC"))
    U = DataArray(D.synthetic((nz, n, n), 51), ("Z", "YC", "XG"))
    V = DataArray(D.synthetic((nz, n, n), 52), ("Z", "YG", "XC"))
    cells = nz * n * n

    def chain():
        uz = grid.interp(grid.derivative(U, "Z", to="outer"), "X")
        vz = grid.interp(grid.derivative(V, "Z", to="outer"), "Y")
        return grid.derivative(B, "Z", to="outer") / (uz * uz + vz * vz)

    got, want = grid.richardson_number(B, U, V), chain()
    ok = bool(torch.equal(got.data.view(torch.int64), want.data.view(torch.int64)))   # (the bits: Ri is NaN at faces 0 and nz)
    del got, want
    torch.cuda.empty_cache()
    tf, tc = timeit_rounds(lambda: grid.richardson_number(B, U, V), chain, max(3, reps // 2))
    med = lambda t: sorted(t)[len(t) // 2]  # noqa: E731
    bpc = 32   # b, u, v and Ri (the 91st face of Ri is not counted)
    rec(5, "richardson_number fused derivative(b, Z) / (interp(derivative(u, Z), X)^2 + interp(derivative(v, Z), Y)^2), to=outer, drC(Zp1), extend: 3 reads + 1 write", med(tf), cells, bpc)
    rec(5, "richardson_number as its chain (9 launches), fused-equivalent bytes", med(tc), cells, bpc)
    print(json.dumps({"config": 5, "check": "fused richardson_number == chain bit for bit at full size", "ok": ok,
                      "speedup": round(med(tc) / med(tf), 2), "rounds_ms_fused": [round(t, 3) for t in tf],
                      "rounds_ms_chain": [round(t, 3) for t in tc],
                      "fused_below_chain_in_every_round": all(a < b for a, b in zip(tf, tc))}), flush=True)


def run_richardson_mixing(reps, nz=90, n=4320):
    """richardson_mixing in one pass against its chain (vertical_shear_squared, itself one pass, the derivative of b and the
    closure as twelve launches of array arithmetic; a profile drC(Zp1); periodic / extend / extend, to="outer", a shear floor
    of 2^-10 so that the outermost faces are finite), timed in turns, every paired round reported.  Fields 40 GB, the two
    results 27 GB, the chain's live temporaries about 110 GB: some 180 GB at the peak of the comparison."""
    coords = {"XC": ("XC", np.arange(n) + 0.5), "XG": ("XG", np.arange(n) * 1.0), "YC": ("YC", np.arange(n) + 0.5),
              "YG": ("YG", np.arange(n) * 1.0), "Z": ("Z", np.arange(nz) + 0.5), "Zp1": ("Zp1", np.arange(nz + 1) * 1.0)}
    ds = Dataset({"drC": DataArray(D.synthetic((nz + 1,), 34, 0, 10.0, 10.0), ("Zp1",))}, coords)
    grid = Grid(ds, coords={"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"},
                            "Z": {"center": "Z", "outer": "Zp1"}},
                padding={"X": "periodic", "Y": "extend", "Z": "extend"}, metrics={("Z",): ["drC"]}, autoparse_metadata=False)
    B = DataArray(D.synthetic((nz, n, n), 63), ("Z", "YC", "XC"))
    U = DataArray(D.synthetic((nz, n, n), 51), ("Z", "YC", "XG"))
    V = DataArray(D.synthetic((nz, n, n), 52), ("Z", "YG", "XC"))
    cells = nz * n * n
    nu0, alpha, nu_b, kappa_b, floor = 5e-3, 5.0, 1e-4, 1e-5, 2.0 ** -10

    def chain():
        s2 = grid.vertical_shear_squared(U, V, to="outer")
        n2 = grid.derivative(B, "Z", to="outer")
        ri = n2 / (s2 + floor)
        rp = (ri + abs(ri)) * 0.5
        den = 1.0 + alpha * rp
        nu = nu0 / (den * den) + nu_b
        return nu, nu / den + kappa_b

    one = lambda: grid.richardson_mixing(B, U, V, nu0, alpha, nu_b, kappa_b, floor, to="outer")  # noqa: E731
    got, want = one(), chain()
    ok = all(bool(torch.equal(g.data.view(torch.int64), w.data.view(torch.int64))) for g, w in zip(got, want))   # (the bits)
    finite = all(bool(torch.isfinite(g.data).all()) for g in got)
    del got, want
    torch.cuda.empty_cache()
    tf, tc = timeit_rounds(one, chain, max(3, reps // 2))
    med = lambda t: sorted(t)[len(t) // 2]  # noqa: E731
    bpc = 40   # b, u, v, nu and kappa (the 91st face of the results is not counted)
    rec(5, "richardson_mixing one pass: nu, kappa of the Pacanowski-Philander closure from b, u, v, to=outer, drC(Zp1), extend: 3 reads + 2 writes", med(tf), cells, bpc)
    rec(5, "richardson_mixing as its chain (vertical_shear_squared + derivative + 12 launches of arithmetic), one-pass-equivalent bytes", med(tc), cells, bpc)
    print(json.dumps({"config": 5, "check": "one-pass richardson_mixing == chain bit for bit at full size, both results", "ok": ok,
                      "results_finite": finite, "speedup": round(med(tc) / med(tf), 2), "rounds_ms_fused": [round(t, 3) for t in tf],
                      "rounds_ms_chain": [round(t, 3) for t in tc],
                      "fused_below_chain_in_every_round": all(a < b for a, b in zip(tf, tc))}), flush=True)


def run_isopycnal_slope(reps, nz=90, n=4320):
    """isopycnal_slope in one pass against its chain of eleven launches (three derivatives, four interpolations, two
    quotients, two negations; dxC, dyC and a profile drC(Zp1); periodic / extend / extend, to="outer"), timed in turns,
    every paired round reported.  The field 13 GB, the four results of the comparison 54 GB, the chain's live temporaries
    about 55 GB.  Under `extend` the outermost faces are x / 0: the comparison is of the bits, a NaN equal to a NaN."""
    coords = {"XC": ("XC", np.arange(n) + 0.5), "XG": ("XG", np.arange(n) * 1.0), "YC": ("YC", np.arange(n) + 0.5),
              "YG": ("YG", np.arange(n) * 1.0), "Z": ("Z", np.arange(nz) + 0.5), "Zp1": ("Zp1", np.arange(nz + 1) * 1.0)}
    ds = Dataset({"dxC": DataArray(D.synthetic((n, n), 31, 0, 1000.0, 1000.0), ("YC", "XG")),
                  "dyC": DataArray(D.synthetic((n, n), 32, 0, 1000.0, 1000.0), ("YG", "XC")),
                  "drC": DataArray(D.synthetic((nz + 1,), 34, 0, 10.0, 10.0), ("Zp1",))}, coords)
    grid = Grid(ds, coords={"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"},
                            "Z": {"center": "Z", "outer": "Zp1"}},
                padding={"X": "periodic", "Y": "extend", "Z": "extend"},
                metrics={("X",): ["dxC"], ("Y",): ["dyC"], ("Z",): ["drC"]}, autoparse_metadata=False)
    B = DataArray(D.synthetic((nz, n, n), 63), ("Z", "YC", "XC"))
    cells = nz * n * n

    def chain():
        gx = grid.interp(grid.interp(grid.derivative(B, "X"), "X"), "Z", to="outer")
        gy = grid.interp(grid.interp(grid.derivative(B, "Y"), "Y"), "Z", to="outer")
        bz = grid.derivative(B, "Z", to="outer")
        return -(gx / bz), -(gy / bz)

    def same(g, w):
        eq = g.data.view(torch.int64) == w.data.view(torch.int64)
        eq |= torch.isnan(g.data) & torch.isnan(w.data)
        return bool(eq.all())

    one = lambda: grid.isopycnal_slope(B, to="outer")  # noqa: E731
    got, want = one(), chain()
    ok = all(same(g, w) for g, w in zip(got, want))
    interior_finite = all(bool(torch.isfinite(g.data[1:nz]).all()) for g in got)
    del got, want
    torch.cuda.empty_cache()
    tf, tc = timeit_rounds(one, chain, max(3, reps // 2))
    med = lambda t: sorted(t)[len(t) // 2]  # noqa: E731
    bpc = 24   # b, sx and sy (the 91st face of the results is not counted)
    rec(5, "isopycnal_slope one pass: sx, sy from b, to=outer, dxC, dyC, drC(Zp1), periodic/extend/extend: 1 read + 2 writes", med(tf), cells, bpc)
    rec(5, "isopycnal_slope as its chain (11 launches), one-pass-equivalent bytes", med(tc), cells, bpc)
    print(json.dumps({"config": 5, "check": "one-pass isopycnal_slope == chain bit for bit at full size, both results", "ok": ok,
                      "interior_faces_finite": interior_finite, "speedup": round(med(tc) / med(tf), 2),
                      "rounds_ms_fused": [round(t, 3) for t in tf], "rounds_ms_chain": [round(t, 3) for t in tc],
                      "fused_below_chain_in_every_round": all(a < b for a, b in zip(tf, tc))}), flush=True)


def run_redi_tensor(reps, nz=90, n=4320):
    """redi_tensor in one pass against its chain (isopycnal_slope's one pass, then thirteen launches of array arithmetic:
    the squares, their sum, the taper min(1, m2 / s2) without a branch, the three products; dxC, dyC and a profile drC(Zp1);
    periodic / extend / extend, to="outer", kappa 1000, slope_max 1e-2), timed in turns, every paired round reported.  The
    field 13 GB, the six results of the comparison 82 GB, the chain's live temporaries (the expression frees each as it
    goes) about 95 GB beside the one pass's three results: about 190 GB at the peak, all 90 levels.  Under `extend` the
    outermost faces are 0 * inf: the comparison is of the bits, a NaN equal to a NaN."""
    coords = {"XC": ("XC", np.arange(n) + 0.5), "XG": ("XG", np.arange(n) * 1.0), "YC": ("YC", np.arange(n) + 0.5),
              "YG": ("YG", np.arange(n) * 1.0), "Z": ("Z", np.arange(nz) + 0.5), "Zp1": ("Zp1", np.arange(nz + 1) * 1.0)}
    ds = Dataset({"dxC": DataArray(D.synthetic((n, n), 31, 0, 1000.0, 1000.0), ("YC", "XG")),
                  "dyC": DataArray(D.synthetic((n, n), 32, 0, 1000.0, 1000.0), ("YG", "XC")),
                  "drC": DataArray(D.synthetic((nz + 1,), 34, 0, 10.0, 10.0), ("Zp1",))}, coords)
    grid = Grid(ds, coords={"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"},
                            "Z": {"center": "Z", "outer": "Zp1"}},
                padding={"X": "periodic", "Y": "extend", "Z": "extend"},
                metrics={("X",): ["dxC"], ("Y",): ["dyC"], ("Z",): ["drC"]}, autoparse_metadata=False)
    B = DataArray(D.synthetic((nz, n, n), 63), ("Z", "YC", "XC"))
    cells = nz * n * n
    kappa, slope_max = 1000.0, 1e-2   # (the operator's defaults)

    def chain():
        sx, sy = grid.isopycnal_slope(B, to="outer")
        s2 = sx * sx + sy * sy
        m2 = float(slope_max) * float(slope_max)
        ex = s2 - m2
        den = m2 + (ex + abs(ex)) * 0.5
        kt = kappa * (m2 / den)
        return kt * sx, kt * sy, kt * s2

    def same(g, w):
        eq = g.data.view(torch.int64) == w.data.view(torch.int64)
        eq |= torch.isnan(g.data) & torch.isnan(w.data)
        return bool(eq.all())

    one = lambda: grid.redi_tensor(B, kappa, slope_max, to="outer")  # noqa: E731
    got, want = one(), chain()
    ok = all(same(g, w) for g, w in zip(got, want))
    interior_finite = all(bool(torch.isfinite(g.data[1:nz]).all()) for g in got)
    tapered = float((got[2].data[1:nz] > 0.999 * kappa * slope_max * slope_max).double().mean())   # faces above the limit
    del got, want
    torch.cuda.empty_cache()
    tf, tc = timeit_rounds(one, chain, max(3, reps // 2))
    med = lambda t: sorted(t)[len(t) // 2]  # noqa: E731
    bpc = 32   # b, kwx, kwy and kwz (the 91st face of the results is not counted)
    rec(5, "redi_tensor one pass: kwx, kwy, kwz from b, to=outer, dxC, dyC, drC(Zp1), periodic/extend/extend: 1 read + 3 writes", med(tf), cells, bpc)
    rec(5, "redi_tensor as its chain (isopycnal_slope + 13 launches), one-pass-equivalent bytes", med(tc), cells, bpc)
    print(json.dumps({"config": 5, "check": "one-pass redi_tensor == chain bit for bit at full size, all three results", "ok": ok,
                      "interior_faces_finite": interior_finite, "fraction_of_interior_faces_tapered": round(tapered, 4),
                      "speedup": round(med(tc) / med(tf), 2),
                      "rounds_ms_fused": [round(t, 3) for t in tf], "rounds_ms_chain": [round(t, 3) for t in tc],
                      "fused_below_chain_in_every_round": all(a < b for a, b in zip(tf, tc))}), flush=True)


def run_redi_vertical_flux_divergence(reps, nz=90, n=4320):
    """redi_vertical_flux_divergence in one pass against its chain (two derivatives, four interpolations, two products, their
    sum, the copy that closes the top and the bottom faces, the derivative back to the centre: ten launches and the copy;
    dxC, dyC, drF(Z); periodic / extend / extend, to="outer", closed=True), timed in turns, every paired round reported.
    kwx and kwy are `redi_tensor(b)`'s at its defaults, as they are: their outermost faces are NaN (0 * inf), which a closed
    call never reads; the tracer is a second synthetic field.  By the count of its launches the chain moves about 200 B/cell
    (3 x 16 for each of gx and gy, 24 for each product and for the sum, 16 for the copy, 16 for the last derivative) against
    the one pass's 32.  The tracer and the two tensor columns 40 GB, the two results of the comparison 27 GB, the chain's live
    temporaries (the expression frees each as it goes) about 55 GB; b and kwz are freed before the timing: about 125 GB at the
    peak, all 90 levels."""
    coords = {"XC": ("XC", np.arange(n) + 0.5), "XG": ("XG", np.arange(n) * 1.0), "YC": ("YC", np.arange(n) + 0.5),
              "YG": ("YG", np.arange(n) * 1.0), "Z": ("Z", np.arange(nz) + 0.5), "Zp1": ("Zp1", np.arange(nz + 1) * 1.0)}
    ds = Dataset({"dxC": DataArray(D.synthetic((n, n), 31, 0, 1000.0, 1000.0), ("YC", "XG")),
                  "dyC": DataArray(D.synthetic((n, n), 32, 0, 1000.0, 1000.0), ("YG", "XC")),
                  "drC": DataArray(D.synthetic((nz + 1,), 34, 0, 10.0, 10.0), ("Zp1",)),
                  "drF": DataArray(D.synthetic((nz,), 33, 0, 10.0, 10.0), ("Z",))}, coords)
    grid = Grid(ds, coords={"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"},
                            "Z": {"center": "Z", "outer": "Zp1"}},
                padding={"X": "periodic", "Y": "extend", "Z": "extend"},
                metrics={("X",): ["dxC"], ("Y",): ["dyC"], ("Z",): ["drC", "drF"]}, autoparse_metadata=False)
    B = DataArray(D.synthetic((nz, n, n), 63), ("Z", "YC", "XC"))
    kwx, kwy, kwz = grid.redi_tensor(B)
    del B, kwz
    torch.cuda.empty_cache()
    A = DataArray(D.synthetic((nz, n, n), 64), ("Z", "YC", "XC"))
    cells = nz * n * n

    def chain():
        gx = grid.interp(grid.interp(grid.derivative(A, "X"), "X"), "Z", to="outer")
        gy = grid.interp(grid.interp(grid.derivative(A, "Y"), "Y"), "Z", to="outer")
        f = kwx * gx + kwy * gy
        del gx, gy
        data = f.data.clone()     # the closed top and bottom: no flux
        data[0] = 0.0
        data[nz] = 0.0
        return grid.derivative(f._replace(data=data), "Z")

    one = lambda: grid.redi_vertical_flux_divergence(A, kwx, kwy)  # noqa: E731   (the defaults: to="outer", closed=True)
    got, want = one(), chain()
    eq = got.data.view(torch.int64) == want.data.view(torch.int64)
    eq |= torch.isnan(got.data) & torch.isnan(want.data)
    ok = bool(eq.all())
    finite = bool(torch.isfinite(got.data).all())
    nonzero = float((got.data != 0).double().mean())
    nan_faces = bool(torch.isnan(kwx.data[0]).all() and torch.isnan(kwx.data[nz]).all())
    del got, want, eq
    torch.cuda.empty_cache()
    tf, tc = timeit_rounds(one, chain, max(3, reps // 2))
    med = lambda t: sorted(t)[len(t) // 2]  # noqa: E731
    bpc = 32   # a, kwx, kwy and the result (the 91st face of kwx and kwy is not counted)
    rec(5, "redi_vertical_flux_divergence one pass: a, kwx, kwy in, to=outer, closed, dxC, dyC, drF(Z), periodic/extend/extend: 3 reads + 1 write", med(tf), cells, bpc)
    rec(5, "redi_vertical_flux_divergence as its chain (10 launches and the closing copy), one-pass-equivalent bytes", med(tc), cells, bpc)
    print(json.dumps({"config": 5, "check": "one-pass redi_vertical_flux_divergence == chain bit for bit at full size", "ok": ok,
                      "result_finite_everywhere": finite, "fraction_of_cells_nonzero": round(nonzero, 4),
                      "outermost_faces_of_kwx_are_nan": nan_faces, "speedup": round(med(tc) / med(tf), 2),
                      "rounds_ms_fused": [round(t, 3) for t in tf], "rounds_ms_chain": [round(t, 3) for t in tc],
                      "fused_below_chain_in_every_round": all(a < b for a, b in zip(tf, tc))}), flush=True)


def run_bolus_velocity(reps, nz=90, n=4320):
    """bolus_velocity in one pass against its chain (two interpolations, the two copies that close the top and the bottom
    faces, two derivatives along Z, two negations, two metric products and the fused divergence: eleven launches; dyG, dxG, rA,
    drF(Z); periodic / extend / extend, Z:outer, closed=True), timed in turns, every paired round reported.  kwx and kwy are
    `redi_tensor(b)`'s at its defaults, as they are: their outermost faces are NaN (0 * inf), which a closed call never reads.
    By the count of its launches the chain moves about 184 B/cell (16 for each interpolation, closing copy and negation, 16
    for each derivative, 16 for each product, 24 for the divergence) against the one pass's 40: two reads and three writes.
    The two tensor columns 27 GB, the three results twice for the comparison 81 GB, the chain's live temporaries about 80 GB;
    b and kwz are freed before: about 190 GB at the peak, all 90 levels."""
    coords = {"XC": ("XC", np.arange(n) + 0.5), "XG": ("XG", np.arange(n) * 1.0), "YC": ("YC", np.arange(n) + 0.5),
              "YG": ("YG", np.arange(n) * 1.0), "Z": ("Z", np.arange(nz) + 0.5), "Zp1": ("Zp1", np.arange(nz + 1) * 1.0)}
    ds = Dataset({"dxC": DataArray(D.synthetic((n, n), 31, 0, 1000.0, 1000.0), ("YC", "XG")),
                  "dyC": DataArray(D.synthetic((n, n), 32, 0, 1000.0, 1000.0), ("YG", "XC")),
                  "dyG": DataArray(D.synthetic((n, n), 35, 0, 1000.0, 1000.0), ("YC", "XG")),
                  "dxG": DataArray(D.synthetic((n, n), 36, 0, 1000.0, 1000.0), ("YG", "XC")),
                  "rA": DataArray(D.synthetic((n, n), 37, 0, 1e6, 1e6), ("YC", "XC")),
                  "drC": DataArray(D.synthetic((nz + 1,), 34, 0, 10.0, 10.0), ("Zp1",)),
                  "drF": DataArray(D.synthetic((nz,), 33, 0, 10.0, 10.0), ("Z",))}, coords)
    grid = Grid(ds, coords={"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"},
                            "Z": {"center": "Z", "outer": "Zp1"}},
                padding={"X": "periodic", "Y": "extend", "Z": "extend"},
                metrics={("X",): ["dxC", "dxG"], ("Y",): ["dyC", "dyG"], ("X", "Y"): ["rA"], ("Z",): ["drC", "drF"]},
                autoparse_metadata=False)
    B = DataArray(D.synthetic((nz, n, n), 63), ("Z", "YC", "XC"))
    kwx, kwy, kwz = grid.redi_tensor(B)
    del B, kwz
    torch.cuda.empty_cache()
    cells = nz * n * n

    def closed(p):
        data = p.data.clone()     # the closed top and bottom: no eddy transport
        data[0] = 0.0
        data[nz] = 0.0
        return p._replace(data=data)

    def chain():
        px, py = closed(grid.interp(kwx, "X")), closed(grid.interp(kwy, "Y"))
        ub = -grid.derivative(px, "Z")
        vb = -grid.derivative(py, "Z")
        tx = px * grid.get_metric(px, ("Y",))
        ty = py * grid.get_metric(py, ("X",))
        del px, py
        return ub, vb, grid.divergence(tx, ty)

    one = lambda: grid.bolus_velocity(kwx, kwy)  # noqa: E731   (the defaults: closed=True)
    got, want = list(one()), list(chain())
    ok, finite, nonzero = [], [], []
    while got:
        g, w = got.pop(0), want.pop(0)
        eq = g.data.view(torch.int64) == w.data.view(torch.int64)
        eq |= torch.isnan(g.data) & torch.isnan(w.data)
        ok.append(bool(eq.all()) and g.dims == w.dims)
        finite.append(bool(torch.isfinite(g.data).all()))
        nonzero.append(round(float((g.data != 0).double().mean()), 4))
        del g, w, eq
        torch.cuda.empty_cache()
    nan_faces = bool(torch.isnan(kwx.data[0]).all() and torch.isnan(kwx.data[nz]).all())
    tf, tc = timeit_rounds(one, chain, max(3, reps // 2))
    med = lambda t: sorted(t)[len(t) // 2]  # noqa: E731
    bpc = 40   # kwx, kwy in, ub, vb, wb out (the 91st face of kwx, kwy and wb is not counted)
    rec(5, "bolus_velocity one pass: kwx, kwy in, Z:outer, closed, dyG, dxG, rA, drF(Z), periodic/extend/extend: 2 reads + 3 writes", med(tf), cells, bpc)
    rec(5, "bolus_velocity as its chain (11 launches and the two closing copies), one-pass-equivalent bytes", med(tc), cells, bpc)
    print(json.dumps({"config": 5, "check": "one-pass bolus_velocity == chain bit for bit at full size (ub, vb, wb)", "ok": ok,
                      "result_finite_everywhere": finite, "fraction_of_cells_nonzero": nonzero,
                      "outermost_faces_of_kwx_are_nan": nan_faces, "bytes_per_cell_one_pass": bpc, "bytes_per_cell_chain": 184,
                      "bound_by_bytes": round(184 / bpc, 2), "speedup": round(med(tc) / med(tf), 2),
                      "fraction_of_8TBps_at_40B_per_cell": round(cells * bpc / (med(tf) * 1e-3) / 8e12, 4),
                      "rounds_ms_fused": [round(t, 3) for t in tf], "rounds_ms_chain": [round(t, 3) for t in tc],
                      "fused_below_chain_in_every_round": all(a < b for a, b in zip(tf, tc))}), flush=True)


def run_redi_horizontal_tensor(reps, nz=90, n=4320):
    """redi_horizontal_tensor in one pass against its chain of 40 launches (three derivatives, the mean of db/dz back to the
    levels, two means of it towards u's and v's points, the two cross means of two interpolations each, four quotients, four
    negations, twice eleven launches of taper arithmetic; dxC, dyC and a profile drC(Zp1); periodic / extend / extend,
    to="outer", kappa 1000, slope_max 1e-2), timed in turns, every paired round reported.  The chain frees its temporaries as
    it goes.  By the count of its launches it moves about 720 B/cell in float64 (ten stencils and four negations at 16, four
    quotients at 24, twice eleven launches of taper arithmetic at about 200 together) against the one pass's 24: one read,
    two writes.  The field 13 GB, the six results of the comparison 81 GB, the chain's live temporaries about 70 GB: about
    165 GB at the peak, all 90 levels."""
    coords = {"XC": ("XC", np.arange(n) + 0.5), "XG": ("XG", np.arange(n) * 1.0), "YC": ("YC", np.arange(n) + 0.5),
              "YG": ("YG", np.arange(n) * 1.0), "Z": ("Z", np.arange(nz) + 0.5), "Zp1": ("Zp1", np.arange(nz + 1) * 1.0)}
    ds = Dataset({"dxC": DataArray(D.synthetic((n, n), 31, 0, 1000.0, 1000.0), ("YC", "XG")),
                  "dyC": DataArray(D.synthetic((n, n), 32, 0, 1000.0, 1000.0), ("YG", "XC")),
                  "drC": DataArray(D.synthetic((nz + 1,), 34, 0, 10.0, 10.0), ("Zp1",))}, coords)
    grid = Grid(ds, coords={"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"},
                            "Z": {"center": "Z", "outer": "Zp1"}},
                padding={"X": "periodic", "Y": "extend", "Z": "extend"},
                metrics={("X",): ["dxC"], ("Y",): ["dyC"], ("Z",): ["drC"]}, autoparse_metadata=False)
    B = DataArray(D.synthetic((nz, n, n), 63), ("Z", "YC", "XC"))
    cells = nz * n * n
    kappa, slope_max = 1000.0, 1e-2   # (the operator's defaults)

    def taper(sa, sb, pick):
        s2 = sa * sa + sb * sb
        m2 = float(slope_max) * float(slope_max)
        ex = s2 - m2
        den = m2 + (ex + abs(ex)) * 0.5
        del s2, ex
        kt = kappa * (m2 / den)
        del den
        return kt * pick

    def chain():
        gx = grid.derivative(B, "X")
        gy = grid.derivative(B, "Y")
        bzc = grid.interp(grid.derivative(B, "Z", to="outer"), "Z", to="center")
        bzu = grid.interp(bzc, "X", to="left")
        bzv = grid.interp(bzc, "Y", to="left")
        del bzc
        gyu = grid.interp(grid.interp(gy, "Y", to="center"), "X", to="left")
        gxv = grid.interp(grid.interp(gx, "X", to="center"), "Y", to="left")
        sxu, syu = -(gx / bzu), -(gyu / bzu)
        del bzu, gyu, gx
        sxv, syv = -(gxv / bzv), -(gy / bzv)
        del bzv, gxv, gy
        kuz = taper(sxu, syu, sxu)
        del sxu, syu
        kvz = taper(sxv, syv, syv)
        return kuz, kvz

    one = lambda: grid.redi_horizontal_tensor(B, kappa, slope_max, to="outer")  # noqa: E731
    got, want = list(one()), list(chain())
    free = list(grid.redi_horizontal_tensor(B, kappa, None, to="outer"))
    ok, finite, tapered = [], [], []
    while got:
        g, w, f = got.pop(0), want.pop(0), free.pop(0)
        eq = g.data.view(torch.int64) == w.data.view(torch.int64)
        eq |= torch.isnan(g.data) & torch.isnan(w.data)
        ok.append(bool(eq.all()) and g.dims == w.dims)
        finite.append(bool(torch.isfinite(g.data).all()))
        tapered.append(round(float((g.data != f.data).double().mean()), 4))   # the taper is exactly 1 below the limit
        del g, w, f, eq
        torch.cuda.empty_cache()
    tf, tc = timeit_rounds(one, chain, max(4, reps // 2))
    med = lambda t: sorted(t)[len(t) // 2]  # noqa: E731
    bpc = 24   # b in, kuz and kvz out
    rec(5, "redi_horizontal_tensor one pass: kuz, kvz from b, to=outer, dxC, dyC, drC(Zp1), periodic/extend/extend: 1 read + 2 writes", med(tf), cells, bpc)
    rec(5, "redi_horizontal_tensor as its chain (40 launches), one-pass-equivalent bytes", med(tc), cells, bpc)
    print(json.dumps({"config": 5, "check": "one-pass redi_horizontal_tensor == chain bit for bit at full size (kuz, kvz)", "ok": ok,
                      "result_finite_everywhere": finite, "fraction_of_cells_tapered": tapered, "levels": nz,
                      "bytes_per_cell_one_pass": bpc, "bytes_per_cell_chain": 720, "bound_by_bytes": round(720 / bpc, 1),
                      "speedup": round(med(tc) / med(tf), 2),
                      "fraction_of_8TBps_at_24B_per_cell": round(cells * bpc / (med(tf) * 1e-3) / 8e12, 4),
                      "rounds_ms_fused": [round(t, 3) for t in tf], "rounds_ms_chain": [round(t, 3) for t in tc],
                      "fused_below_chain_in_every_round": all(a < b for a, b in zip(tf, tc))}), flush=True)


def run_implicit_vertical_viscosity(reps, nz=90, ny=4320, nx=4320):
    """implicit_vertical_viscosity in one pass (one launch per component) against its chain of four calls (two interps of nu,
    two implicit_vertical_diffusion solves; two face-sized temporaries) on resident tensors: nu (nz + 1, ny, nx) at Z:outer,
    drC(Zp1), drF(Z), X periodic, Y extend, timed in turns, every paired round reported.  Fields, results, workspaces and the
    chain's temporaries take about 120 GB at 4320 x 4320 x 90; when that allocation fails the pair runs at 75 x 2400 x 3600
    and the records say so."""
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0), "YC": ("YC", np.arange(ny) + 0.5),
              "YG": ("YG", np.arange(ny) * 1.0), "Z": ("Z", np.arange(nz) + 0.5), "Zp1": ("Zp1", np.arange(nz + 1) * 1.0)}
    drf, drc = D.synthetic((nz,), 33, 0, 10.0, 10.0), D.synthetic((nz + 1,), 34, 0, 10.0, 10.0)
    ds = Dataset({"drF": DataArray(drf, ("Z",)), "drC": DataArray(drc, ("Zp1",))}, coords)
    grid = Grid(ds, coords={"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"},
                            "Z": {"center": "Z", "outer": "Zp1"}},
                padding={"X": "periodic", "Y": "extend", "Z": "extend"}, metrics={("Z",): ["drF", "drC"]}, autoparse_metadata=False)
    dt = 3600.0                                                                        # coupling dt nu / (drC drF) <= 3.6
    cells = nz * ny * nx
    try:
        U = DataArray(D.synthetic((nz, ny, nx), 51), ("Z", "YC", "XG"))
        V = DataArray(D.synthetic((nz, ny, nx), 52), ("Z", "YG", "XC"))
        NU = DataArray(D.synthetic((nz + 1, ny, nx), 62, 0, 0.1, 0.0), ("Zp1", "YC", "XC"))   # 0 .. 0.1 m2/s over 10 .. 20 m layers

        def chain():
            nu_u, nu_v = grid.interp(NU, "X"), grid.interp(NU, "Y")
            return grid.implicit_vertical_diffusion(U, nu_u, dt), grid.implicit_vertical_diffusion(V, nu_v, dt)

        got, want = grid.implicit_vertical_viscosity(U, V, NU, dt=dt), chain()
        ok = all(bool(torch.equal(g.data.view(torch.int64), w.data.view(torch.int64))) for g, w in zip(got, want))
        del got, want
        torch.cuda.empty_cache()
        tf, tc = timeit_rounds(lambda: grid.implicit_vertical_viscosity(U, V, NU, dt=dt), chain, max(3, reps // 2))
    except torch.cuda.OutOfMemoryError:
        if (nz, ny, nx) == (75, 2400, 3600):
            raise
        print(json.dumps({"config": 5, "note": f"{nz} x {ny} x {nx} does not fit: implicit_vertical_viscosity at 75 x 2400 x 3600"}), flush=True)
        U = V = NU = None
        torch.cuda.empty_cache()
        return run_implicit_vertical_viscosity(reps, 75, 2400, 3600)
    med = lambda t: sorted(t)[len(t) // 2]  # noqa: E731
    # per component a, nu, d out and back, c out and back, x: 56; nu is read by each of the two launches (its 91st face is not
    # counted).  The chain asks for 144: the two interps 16 + 16, the two solves 2 x 56
    bpc = 112
    size = f"{nz} x {ny} x {nx}"
    rec(5, f"implicit_vertical_viscosity one pass (u and v, one launch each, nu averaged in the coefficient stage), {size}, drC / drF: per component a, nu, d and c out and back, x", med(tf), cells, bpc)
    rec(5, f"implicit_vertical_viscosity as its chain (2 interps of nu + 2 implicit_vertical_diffusion), {size}, one-pass-equivalent bytes", med(tc), cells, bpc)
    print(json.dumps({"config": 5, "check": f"one-pass implicit_vertical_viscosity == chain bit for bit at {size}", "ok": ok,
                      "speedup": round(med(tc) / med(tf), 2), "rounds_ms_fused": [round(t, 3) for t in tf],
                      "rounds_ms_chain": [round(t, 3) for t in tc],
                      "fused_below_chain_in_every_round": all(a < b for a, b in zip(tf, tc))}), flush=True)


def rec(cfg, name, ms, cells, bpc):
    gbs = cells * bpc / (ms * 1e-3) / 1e9
    print(json.dumps({"config": cfg, "op": name, "ms": round(ms, 3), "gcell_s": round(cells / ms / 1e6, 2),
                      "bytes_per_cell": round(bpc, 3), "GBps": round(gbs, 1), "frac_8TBps": round(gbs / 8000, 4)}), flush=True)


def mitgcm_grid(nz, ny, nx, nt=None):
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0),
              "YC": ("YC", np.arange(ny) + 0.5), "YG": ("YG", np.arange(ny) * 1.0),
              "Z": ("Z", np.arange(nz) + 0.5), "Zl": ("Zl", np.arange(nz) * 1.0), "Zp1": ("Zp1", np.arange(nz + 1) * 1.0)}
    dv = {"dxC": DataArray(D.synthetic((ny, nx), 31, 0, 1000.0, 1000.0), ("YC", "XG")),
          "dyC": DataArray(D.synthetic((ny, nx), 32, 0, 1000.0, 1000.0), ("YG", "XC")),
          "rAz": DataArray(D.synthetic((ny, nx), 53, 0, 1000.0, 1000.0), ("YG", "XG")),
          "drF": DataArray(D.synthetic((nz,), 33, 0, 1000.0, 1000.0), ("Z",)),
          "drC": DataArray(D.synthetic((nz,), 34, 0, 1000.0, 1000.0), ("Zl",))}
    ds = Dataset(dv, coords)
    return Grid(ds, coords={"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"},
                            "Z": {"center": "Z", "left": "Zl", "outer": "Zp1"}},
                padding={"X": "periodic", "Y": "extend", "Z": "fill"},
                metrics={("X",): ["dxC"], ("Y",): ["dyC"], ("Z",): ["drF", "drC"], ("X", "Y"): ["rAz"]},
                autoparse_metadata=False)


# ------------------------------------------------------------------------------------------------------
# Sharded configs (4, 5): N ranks, one per GPU, the record / level axis split by sharding.shard_bounds
# ------------------------------------------------------------------------------------------------------
class SpanClock:
    """device time of the spans between start() and stop(): HIP events on the launch stream on a GPU,
    perf_counter on the CPU test double"""

    def __init__(self):
        self.gpu = torch.cuda.is_available()
        self.pairs, self.host_s = [], 0.0

    def start(self):
        if self.gpu:
            self._e0 = torch.cuda.Event(enable_timing=True)
            self._e0.record()
        else:
            self._t0 = time.perf_counter()

    def stop(self):
        if self.gpu:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self.pairs.append((self._e0, e1))
        else:
            self.host_s += time.perf_counter() - self._t0

    def ms(self):
        if self.gpu:
            torch.cuda.synchronize()
            return float(sum(a.elapsed_time(b) for a, b in self.pairs))
        return self.host_s * 1e3


def bits_checksum(x) -> int:
    """sum modulo 2^64 of the 64-bit patterns of a float64 array: order-independent, so the sum over the
    shards of any split equals the single-process value (checksum of checksums)"""
    if isinstance(x, torch.Tensor):
        return int(x.contiguous().view(torch.int64).sum().item()) & 0xFFFFFFFFFFFFFFFF
    return int(np.ascontiguousarray(x, dtype=np.float64).view(np.uint64).sum(dtype=np.uint64))


def _shard_line(ranks, cfg, op, wall_s, dev_ms, local_cells, bpc, chk, extra):
    """reduce the per-rank figures and let rank 0 print one JSON line"""
    per_rank_ms = ranks.gather_floats(dev_ms)
    per_rank_cells = ranks.gather_floats(float(local_cells))
    wall = ranks.max(wall_s)
    total = sum(per_rank_cells)
    chk = ranks.sum_u64(chk)
    line = {"config": cfg, "op": op, "n_gpus": ranks.world, "backend": ranks.backend or "single process",
            "cells": int(total), "wall_ms_between_barriers": round(wall * 1e3, 3),
            "gcell_s": round(total / wall / 1e9, 2) if wall > 0 else None, "bytes_per_cell": round(bpc, 3),
            "GBps_all_gpus": round(total * bpc / wall / 1e9, 1) if wall > 0 else None,
            "frac_8TBps_per_gpu": round(total * bpc / wall / 1e9 / 8000 / ranks.world, 4) if wall > 0 else None,
            "per_rank_device_ms": [round(v, 3) for v in per_rank_ms],
            # min / max over the ranks that had work: 1.0 = perfectly balanced.  Load balance inside ONE run, not scaling
            # efficiency (that is the driver's to compute against N = 1 from the per-N lines)
            "rank_balance_min_over_max": (round(min(v for v in per_rank_ms if v > 0) / max(per_rank_ms), 4) if max(per_rank_ms) > 0 else None),
            "per_rank_cells": [int(v) for v in per_rank_cells], "checksum_u64": f"{chk:016x}"}
    line.update(extra)
    if ranks.rank == 0:
        print(json.dumps(line), flush=True)
    return line


def run_config4(ranks, n_records=360, shape=(75, 2400, 3600), per_batch=None, ops=("left", "outer")):
    """cumsum(T,'Z') over `n_records` records sharded over the record axis; every rank walks its block in
    HBM-resident batches (inputs generated in HBM before the timed span, outputs checksummed after it)."""
    nz, ny, nx = shape
    cells = nz * ny * nx
    grid = mitgcm_grid(nz, ny, nx)
    lo, hi = S.shard_bounds(n_records, ranks.world, ranks.rank)
    # resident per record: the input, the output ((nz + 1) levels for center->outer) and the int64 view the
    # checksum reads in place => 2 records + one level; the caching allocator keeps the previous batch's blocks
    bytes_per_record = 8 * (2 * cells + ny * nx)
    per = per_batch or S.records_per_batch(hi - lo, bytes_per_record, headroom=0.8)
    # (a rank without records has no say in the batch size: it contributes the job's upper bound, not 0)
    per = max(1, int(ranks.min(per if hi > lo else max(1, n_records))))
    batches = S.record_batches(n_records, ranks.world, ranks.rank, per)
    rounds = int(ranks.max(len(batches)))
    dims = ("time", "Z", "YC", "XC")
    lines = []
    if batches:  # untimed warm-up on one record: code objects, allocator pool, clocks
        w = DataArray(D.synthetic((1, nz, ny, nx), 4, offset=lo * cells), dims)
        for _ in range(3):
            grid.cumsum(w, "Z")
            grid.cumsum(w, "Z", to="outer")
        del w
    for to in ops:
        kw = {} if to == "left" else {"to": to}
        if torch.cuda.is_available():
            torch.cuda.empty_cache()  # the two ops' outputs differ in size: do not keep the other op's blocks cached
        clock, wall, chk, local_cells = SpanClock(), 0.0, 0, 0
        for b in range(rounds):
            T4 = out = None
            if b < len(batches):
                s, e = batches[b]
                T4 = DataArray(D.synthetic((e - s, nz, ny, nx), 4, offset=s * cells), dims)
            if T4 is not None and torch.cuda.is_available():
                # the output block comes from torch's caching allocator: make sure it is in the pool before the
                # timed span (a first-time hipMalloc of 120 GB costs more than the scan itself)
                del_me = torch.empty((e - s, nz + (1 if to == "outer" else 0), ny, nx), dtype=torch.float64, device="cuda")
                del del_me
            ranks.barrier()
            t0 = time.perf_counter()
            if T4 is not None:
                clock.start()
                out = grid.cumsum(T4, "Z", **kw)
                clock.stop()
            ranks.barrier()
            wall += time.perf_counter() - t0
            if T4 is not None:
                chk = (chk + bits_checksum(out.data)) & 0xFFFFFFFFFFFFFFFF
                local_cells += (e - s) * cells
            del T4, out
        lines.append(_shard_line(
            ranks, 4, f"cumsum(T,'Z') center->{to} fill, {n_records} records of {nx}x{ny}x{nz} f64 over the record axis",
            wall, clock.ms(), local_cells, 16, chk,
            {"records": n_records, "records_per_rank": [S.shard_bounds(n_records, ranks.world, r)[1] - S.shard_bounds(n_records, ranks.world, r)[0] for r in range(ranks.world)],
             "records_per_resident_batch": per, "batch_rounds": rounds}))
    return lines


def config5_grid(ny, nx):
    coords = {"XC": ("XC", np.arange(nx) + 0.5), "XG": ("XG", np.arange(nx) * 1.0),
              "YC": ("YC", np.arange(ny) + 0.5), "YG": ("YG", np.arange(ny) * 1.0)}
    ds = Dataset({"rAz": DataArray(D.synthetic((ny, nx), 53, 0, 1000.0, 1000.0), ("YG", "XG"))}, coords)
    return Grid(ds, coords={"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"}},
                padding="fill", metrics={("X", "Y"): ["rAz"]}, autoparse_metadata=False)


def run_config5(ranks, shape=(90, 4320, 4320), reps=7):
    """(diff(V,'X') - diff(U,'Y')) / rAz with `fill` on a field split along Z (whole levels per rank, rAz
    replicated): the fused kernel and the reference's operator chain, each `reps` passes between two barriers."""
    nz, ny, nx = shape
    lo, hi = S.shard_bounds(nz, ranks.world, ranks.rank)
    grid = config5_grid(ny, nx)
    nl = hi - lo
    plane = ny * nx
    U = DataArray(D.synthetic((nl, ny, nx), 51, offset=lo * plane), ("Z", "YC", "XG")) if nl else None
    V = DataArray(D.synthetic((nl, ny, nx), 52, offset=lo * plane), ("Z", "YG", "XC")) if nl else None
    area = grid._ds["rAz"].reset_coords(drop=True)

    def fused():
        return grid.vorticity(U, V)

    def chain():
        return (grid.diff(V, "X") - grid.diff(U, "Y")) / area

    def as_written():
        # the SAME text inside `grid.fused()`: deferred results, matched against xg_vorticity when the value is used
        with grid.fused():
            zeta = (grid.diff(V, "X") - grid.diff(U, "Y")) / area
        zeta.data  # the use
        return zeta

    lines = []
    levels = [S.shard_bounds(nz, ranks.world, r)[1] - S.shard_bounds(nz, ranks.world, r)[0] for r in range(ranks.world)]
    for name, fn, n in (("vorticity fused (diff(v,X)-diff(u,Y))/rAz, fill", fused, reps),
                        ("vorticity unfused operator chain (4 kernels), fused-equivalent bytes", chain, max(3, reps // 2)),
                        ("vorticity chain as written, fused on use (with grid.fused(): the same text, one launch)", as_written, reps)):
        out = None
        if nl:
            # warm clocks AND reach the allocators' steady state: `out = fn()` holds the previous result while the next one
            # is made, the chain needs four 13 GB intermediates, and the FIRST time the process reaches a new high-water
            # mark of HBM a 13 GB allocation costs ~0.8 s (tools/placement_probe.py --alloc-cost) -- none of which is the
            # operator's rate.  Warm until a call costs no more than 1.3 x the cheapest one seen (at least 3, at most 12 calls).
            t0 = time.perf_counter()
            best, calls = None, 0
            while torch.cuda.is_available():
                t1 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t1
                calls += 1
                settled = best is not None and dt <= 1.3 * best
                best = dt if best is None else min(best, dt)
                if calls >= 12 or (calls >= 3 and settled and time.perf_counter() - t0 >= 0.15):
                    break
            if not torch.cuda.is_available():
                out = fn()
        clock = SpanClock()
        ranks.barrier()
        t0 = time.perf_counter()
        if nl:
            for _ in range(n):
                clock.start()
                out = fn()
                clock.stop()
        ranks.barrier()
        wall = (time.perf_counter() - t0) / n
        chk = bits_checksum(out.data) if nl else 0
        lines.append(_shard_line(ranks, 5, f"{name}; {nx}x{ny}x{nz} f64 split along Z", wall, clock.ms() / n, nl * plane,
                                 24 + 8 / nz, chk, {"levels_per_rank": levels, "passes": n}))
        del out
    # (every rank takes part in the reduction, also one without levels -- more ranks than levels -- or the others wait for ever)
    same = bool(np.array_equal(D.tohost(fused().data[:1]), D.tohost(chain().data[:1]))
                and np.array_equal(D.tohost(as_written().data[:1]), D.tohost(chain().data[:1]))) if nl else True
    allsame = ranks.min(1.0 if same else 0.0) == 1.0
    if ranks.rank == 0:
        print(json.dumps({"config": 5, "check": "fused == unfused chain == chain as written under grid.fused(), bit for bit (first level of every rank)", "ok": allsame}), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--records", type=int, default=360, help="config 4: records in the whole job (360 = BASELINE)")
    ap.add_argument("--batch-records", type=int, default=0, help="config 4: records per resident batch (0: from free HBM)")
    ap.add_argument("--xrecords", type=int, default=8, help="config 4x: records in the single resident batch")
    ap.add_argument("--configs", default="2,3,4,5")
    ap.add_argument("--gpus", type=int, default=1, help="ranks (one per GPU); only configs 4 and 5 shard")
    ap.add_argument("--shape", default="", help="Z,Y,X override for configs 4 and 5 (tests; default = BASELINE sizes)")
    a = ap.parse_args()
    cfgs = set(a.configs.split(","))
    S.ensure_ranks(a.gpus, os.path.abspath(__file__), sys.argv[1:])
    ranks = S.init_ranks(a.gpus)
    if ranks.world > 1 and cfgs - {"4", "5"}:
        raise SystemExit("only configs 4 and 5 are sharded runs; run the other configs with --gpus 1")
    shp = tuple(int(v) for v in a.shape.split(",")) if a.shape else None
    if ranks.world > 1 or (cfgs and cfgs <= {"4", "5"}):
        try:
            if "4" in cfgs:
                run_config4(ranks, a.records, shape=shp or (75, 2400, 3600), per_batch=a.batch_records or None)
            if "5" in cfgs:
                run_config5(ranks, shape=shp or (90, 4320, 4320), reps=a.reps)
        finally:
            ranks.close()
        return
    nz, ny, nx = 75, 2400, 3600
    cells = nz * ny * nx
    if cfgs & {"2", "3", "f1"}:
        grid = mitgcm_grid(nz, ny, nx)
        T = DataArray(D.synthetic((nz, ny, nx), 2), ("Z", "YC", "XC"))
        if "2" in cfgs:
            for fn in ("interp", "diff"):
                rec(2, f"{fn}(T,'X') periodic", timeit(lambda: getattr(grid, fn)(T, "X"), a.reps), cells, 16)
                rec(2, f"{fn}(T,'Y') extend", timeit(lambda: getattr(grid, fn)(T, "Y"), a.reps), cells, 16)
        if "f1" in cfgs:
            for fn in ("interp", "diff"):
                rec("f1", f"{fn}(T,['X','Y']) ONE pass (xg_stencil2d_f64)", timeit(lambda: getattr(grid, fn)(T, ["X", "Y"]), a.reps), cells, 16)
                rec("f1", f"{fn}(T,'X') then {fn}(.,'Y') two passes (reference order), same 16 B/cell basis",
                    timeit(lambda: getattr(grid, fn)(getattr(grid, fn)(T, "X"), "Y"), a.reps), cells, 16)
            same = bool(torch.equal(grid.interp(T, ["X", "Y"]).data, grid.interp(grid.interp(T, "X"), "Y").data)
                        and torch.equal(grid.diff(T, ["Y", "X"]).data, grid.diff(grid.diff(T, "Y"), "X").data))
            print(json.dumps({"config": "f1", "check": "fused two-axis == sequential, bit for bit, full size", "ok": same}), flush=True)
        if "3" in cfgs:
            rec(3, "derivative(T,'X') / dxC(YC,XG)", timeit(lambda: grid.derivative(T, "X"), a.reps), cells, 16 + 8 / nz)
            rec(3, "derivative(T,'Y') / dyC(YG,XC)", timeit(lambda: grid.derivative(T, "Y"), a.reps), cells, 16 + 8 / nz)
            rec(3, "derivative(T,'Z') / drC(Zl)", timeit(lambda: grid.derivative(T, "Z"), a.reps), cells, 16)
            rec(3, "integrate(T,'Z') * drF(Z)", timeit(lambda: grid.integrate(T, "Z"), a.reps), cells, 8 + 8 / nz)
            rec(3, "average(T,'Z') weighted by drF(Z): sum(T*w) / sum(w | T valid) in ONE pass over T", timeit(lambda: grid.average(T, "Z"), a.reps), cells, 8 + 16 / nz)
        del T, grid
        torch.cuda.empty_cache()
    if "pcie" in cfgs:
        import time

        grid = mitgcm_grid(8, ny, nx)
        host = DataArray(np.random.default_rng(2).random((8, ny, nx)) - 0.5, ("Z", "YC", "XC"))  # numpy in -> numpy out
        grid.diff(host, "X")
        t0 = time.perf_counter()
        for _ in range(3):
            grid.diff(host, "X")
        ms = (time.perf_counter() - t0) / 3 * 1e3
        rec("pcie", "diff(T,'X') with HOST numpy in/out, 8 levels (0.55 GB): above the streaming threshold => block-wise, copies overlapped", ms, 8 * ny * nx, 16)
        D.HOST_STREAM_MIN_BYTES = 1 << 60
        t0 = time.perf_counter()
        for _ in range(3):
            grid.diff(host, "X")
        rec("pcie", "same with the pipelined path switched off (one pageable H2D, kernel, one D2H)", (time.perf_counter() - t0) / 3 * 1e3, 8 * ny * nx, 16)
        D.HOST_STREAM_MIN_BYTES = 256 << 20
        big = DataArray(np.random.default_rng(3).random((75, ny, nx)) - 0.5, ("Z", "YC", "XC"))
        gb = mitgcm_grid(75, ny, nx)
        gb.diff(big, "X")
        t0 = time.perf_counter()
        gb.diff(big, "X")
        rec("pcie", "diff(T,'X') of the full 75-level record held in HOST memory (5.2 GB in, 5.2 GB out), pipelined", (time.perf_counter() - t0) * 1e3, 75 * ny * nx, 16)
        del host, grid, big, gb
    if "stream" in cfgs:
        # f4 (first half): host-resident records streamed through HBM with H2D / kernels / D2H overlapped
        import time

        from xgcm_amd.streaming import stream_records
        nr, nzs = 8, 25
        grid_s = mitgcm_grid(nzs, ny, nx)
        host = np.empty((nr, nzs, ny, nx))
        for r in range(nr):  # synthetic records generated in HBM, copied out once (set-up, untimed)
            host[r] = D.synthetic((nzs, ny, nx), 4, offset=r * nzs * ny * nx).cpu().numpy()
        out = np.empty_like(host)

        def diff_x(block):
            return grid_s.diff(DataArray(block, ("time", "Z", "YC", "XC")), "X").data

        for reg, label in ((True, "page-locked in place block by block"), (False, "pageable copies, D2H in a worker thread")):
            stream_records(diff_x, host[:2], block=1, out=out[:2], register=reg)
            t0 = time.perf_counter()
            stream_records(diff_x, host, block=1, out=out, register=reg)
            ms = (time.perf_counter() - t0) * 1e3
            cs = nr * nzs * ny * nx
            rec("stream", f"diff(T,'X') of {nr} HOST records ({cs * 8 / 1e9:.1f} GB in, same out), 3-stream pipeline, {label}",
                ms, cs, 16)
        t0 = time.perf_counter()
        for r in range(nr):
            out[r] = grid_s.diff(DataArray(host[r], ("Z", "YC", "XC")), "X").values
        rec("stream", "same records one by one through the synchronous numpy-in/numpy-out path", (time.perf_counter() - t0) * 1e3,
            nr * nzs * ny * nx, 16)
        from xgcm_amd.streaming import stream_blocks
        got = []
        t0 = time.perf_counter()
        stream_blocks(diff_x, (host[r:r + 1] for r in range(nr)), sink=lambda k, res: got.append(res[0, 0, 0, 0]))
        rec("stream", f"same records handed over as an ITERABLE of blocks (stream_blocks: read-ahead; in-memory blocks page-locked in place, others staged)",
            (time.perf_counter() - t0) * 1e3, nr * nzs * ny * nx, 16)
        ok = bool(np.array_equal(out[nr - 1], host[nr - 1] - np.roll(host[nr - 1], 1, axis=-1)))
        print(json.dumps({"config": "stream", "check": "last record == host - roll(host, 1) (periodic diff)", "ok": ok}), flush=True)
        del host, out, grid_s
    if "4" in cfgs:
        run_config4(ranks, a.records, per_batch=a.batch_records or None)
    if "4x" in cfgs:
        nt = a.xrecords
        grid = mitgcm_grid(nz, ny, nx)
        T4 = DataArray(D.synthetic((nt, nz, ny, nx), 4), ("time", "Z", "YC", "XC"))
        c4 = nt * cells
        rec("4x", f"cumsum(T,'Z') center->left fill, {nt} records ({c4 / 1e9:.2f} Gcell)", timeit(lambda: grid.cumsum(T4, "Z"), a.reps), c4, 16)
        rec("4x", f"cumsum(T,'Z') center->outer fill, {nt} records", timeit(lambda: grid.cumsum(T4, "Z", to="outer"), a.reps), c4, 16)
        rec("4x", f"diff(T,'X') periodic, {nt} records (>2^32 cells)", timeit(lambda: grid.diff(T4, "X"), a.reps), c4, 16)
        # spot parity on the last record (exercises 64-bit offsets): recompute it alone
        last = DataArray(T4.data[nt - 1].contiguous(), ("Z", "YC", "XC"))
        ok = bool(torch.equal(grid.cumsum(T4, "Z").data[nt - 1], grid.cumsum(last, "Z").data)
                  and torch.equal(grid.diff(T4, "X").data[nt - 1], grid.diff(last, "X").data)
                  and torch.equal(grid.diff(T4, "Y").data[nt - 1], grid.diff(last, "Y").data))
        print(json.dumps({"config": "4x", "check": "last record of the batch == same record processed alone", "ok": ok}), flush=True)
        del T4, last, grid
        torch.cuda.empty_cache()
    if "f2" in cfgs:
        # next-row f2: complex topology at scale -- a cubed sphere of 6 faces x 2160 x 2160 x 25 levels
        # (700 M cells, 5.6 GB f64, MITgcm dim order (Z, face, j, i)); every halo comes from a
        # neighbouring face (rotated / reversed links), no boundary condition anywhere
        nzc, nf, n = 25, 6, 2160
        links = {
            0: {"X": ((3, "X", False), (1, "X", False)), "Y": ((4, "Y", False), (5, "Y", False))},
            1: {"X": ((0, "X", False), (2, "X", False)), "Y": ((4, "X", False), (5, "X", True))},
            2: {"X": ((1, "X", False), (3, "X", False)), "Y": ((4, "Y", True), (5, "Y", True))},
            3: {"X": ((2, "X", False), (0, "X", False)), "Y": ((4, "X", True), (5, "X", False))},
            4: {"X": ((3, "Y", True), (1, "Y", False)), "Y": ((2, "Y", True), (0, "Y", False))},
            5: {"X": ((3, "Y", False), (1, "Y", True)), "Y": ((0, "Y", False), (2, "Y", True))},
        }
        metf = lambda seed: D.synthetic((nf, n, n), seed, 0, 1000.0, 1000.0)  # noqa: E731
        dsf = Dataset({"dxc": DataArray(metf(64), ("face", "j", "i")), "dxg": DataArray(metf(65), ("face", "j", "i_g")),
                       "dyc": DataArray(metf(66), ("face", "j", "i")), "dyg": DataArray(metf(67), ("face", "j_g", "i"))},
                      {"i": ("i", np.arange(n) + 0.5), "i_g": ("i_g", np.arange(n) * 1.0),
                       "j": ("j", np.arange(n) + 0.5), "j_g": ("j_g", np.arange(n) * 1.0),
                       "face": ("face", np.arange(nf))})
        gridf = Grid(dsf, coords={"X": {"center": "i", "left": "i_g"}, "Y": {"center": "j", "left": "j_g"}},
                     face_connections={"face": links}, metrics={("X",): ["dxc", "dxg"], ("Y",): ["dyc", "dyg"]}, autoparse_metadata=False)
        Tf = DataArray(D.synthetic((nzc, nf, n, n), 61), ("Z", "face", "j", "i"))
        cf = nzc * nf * n * n
        import time as _time
        t0 = _time.perf_counter(); gridf.diff(Tf, "X"); torch.cuda.synchronize()
        print(json.dumps({"config": "f2", "note": "first call incl. halo-map construction + upload", "s": round(_time.perf_counter() - t0, 2)}), flush=True)
        for fn in ("diff", "interp"):
            for ax in ("X", "Y"):
                rec("f2", f"{fn}(T,'{ax}') on the cubed sphere (6x2160x2160x25), halos from face connections",
                    timeit(lambda: getattr(gridf, fn)(Tf, ax), a.reps), cf, 16)
        # round 4: the two rows that used to take extra passes -- cumsum along a connected axis (scan into the padded layout,
        # halo cells of the cumulative field put in place) and metric_weighted operators (product halo from two slab gathers)
        for ax in ("X", "Y"):
            # (center -> left along an axis whose links swap axes: the reference's pad of the TRIMMED cumulative field fails in its
            # concat -- tests/golden/grid_reference.json -- and so does the operator here since round 5; the reversed scan needs no
            # halo and is what both can compute)
            rec("f2", f"cumsum(T,'{ax}', reverse=True) on the cubed sphere", timeit(lambda: gridf.cumsum(Tf, ax, reverse=True), a.reps), cf, 16)
            rec("f2", f"interp(T,'{ax}', metric_weighted) on the cubed sphere: one pass, product halo from two slab gathers",
                timeit(lambda: gridf.interp(Tf, ax, metric_weighted=ax), a.reps), cf, 16 + 16 / nzc)
            rec("f2", f"derivative(T,'{ax}') on the cubed sphere", timeit(lambda: gridf.derivative(Tf, ax), a.reps), cf, 16 + 8 / nzc)
        from xgcm_amd.padding import pad as _pad
        rec("f2", "pad(T, X:(1,1), Y:(1,1)) alone (xg_gather)", timeit(lambda: _pad(Tf, gridf, {"X": (1, 1), "Y": (1, 1)}), a.reps), cf, 16)
        # full-size check: halo columns of the X difference against neighbour-face data (host arithmetic on slices)
        d = gridf.diff(Tf, "X").data
        t = Tf.data
        ok = bool(torch.equal(d[:, 1, :, 0], t[:, 1, :, 0] - t[:, 0, :, -1])            # same-axis link 1 <- 0
                  and torch.equal(d[:, 4, :, 0], t[:, 4, :, 0] - t[:, 3, 0, :])  # face 4 left <- face 3 low-Y edge (reversed link)
                  and torch.equal(d[..., 1:], t[..., 1:] - t[..., :-1]))
        print(json.dumps({"config": "f2", "check": "cubed-sphere diff: interior and connected halos at full size", "ok": ok}), flush=True)
        del Tf, d, t
        torch.cuda.empty_cache()
        Uf = DataArray(D.synthetic((nzc, nf, n, n), 62), ("Z", "face", "j", "i_g"))
        Vf = DataArray(D.synthetic((nzc, nf, n, n), 63), ("Z", "face", "j_g", "i"))
        rec("f2", "vorticity fused on the cubed sphere (vector halos: rotated / sign-flipped partner component)",
            timeit(lambda: gridf.vorticity(Uf, Vf, metric_weighted=False), a.reps), cf, 24)

        def chain_f():
            return (gridf.diff({"Y": Vf}, "X", other_component={"X": Uf}) - gridf.diff({"X": Uf}, "Y", other_component={"Y": Vf}))

        rec("f2", "same through the operator chain (2 halo-fused diffs + subtract), fused-equivalent bytes",
            timeit(chain_f, max(3, a.reps // 2)), cf, 24)
        okv = bool(torch.equal(gridf.vorticity(Uf, Vf, metric_weighted=False).data, chain_f().data))
        print(json.dumps({"config": "f2", "check": "cubed-sphere fused vorticity == operator chain bit for bit at full size", "ok": okv}), flush=True)
        del Uf, Vf, gridf
        torch.cuda.empty_cache()
    if "f4" in cfgs:
        # next-row f4: vertical coordinate transform of a (Z, Y, X) = (75, 2400, 3600) f64 field onto 50
        # density-like levels / bins; theta is a full 3-D tracer (the expensive, common case)
        from xgcm_amd import transform as XT
        nzt, nyt, nxt, mt = 75, 2400, 3600, 50
        dsz = Dataset({}, {"Z": ("Z", np.arange(nzt) + 0.5), "Zp1": ("Zp1", np.arange(nzt + 1) * 1.0)})
        gz = Grid(dsz, coords={"Z": {"center": "Z", "outer": "Zp1"}}, autoparse_metadata=False)
        phi = DataArray(D.synthetic((nzt, nyt, nxt), 71), ("Z", "Y", "X"), name="salt")
        # monotonic "density": running sum of positive increments along Z (built with the cumsum kernel)
        inc = D.synthetic((nzt, nyt, nxt), 72, 0, 1.0, 0.55)
        sigma = DataArray(D.cumsum1d(inc, 0, 0, 0, 0, 0, None, 0.0, False, False), ("Z", "Y", "X"), name="sigma")
        inc_o = D.synthetic((nzt + 1, nyt, nxt), 73, 0, 1.0, 0.55)
        sigma_o = DataArray(D.cumsum1d(inc_o, 0, 0, 0, 0, 0, None, 0.0, False, False), ("Zp1", "Y", "X"), name="sigma")
        levels = np.linspace(1.0, 0.9 * nzt, mt)
        edges = np.linspace(0.0, 1.6 * (nzt + 1), mt + 1)
        cols = nyt * nxt
        rec("f4", f"transform linear: {nzt} levels -> {mt} sigma levels (numpy.interp per column), cells = input cells",
            timeit(lambda: gz.transform(phi, "Z", levels, target_data=sigma), a.reps), nzt * cols, (2 * nzt + mt) * 8 / nzt)
        rec("f4", f"transform conservative: {nzt} cells -> {mt} sigma bins, cells = input cells",
            timeit(lambda: gz.transform(phi, "Z", edges, target_data=sigma_o, method="conservative"), max(3, a.reps // 2)),
            nzt * cols, (2 * nzt + 1 + mt) * 8 / nzt)
        # the same with a smooth stratification (neighbouring columns cross a level at nearly the same depth,
        # as in ocean data): lanes of a wave then emit together instead of at 64 different source levels
        zz = torch.arange(nzt, dtype=torch.float64, device="cuda")[:, None, None]
        yy = torch.arange(nyt, dtype=torch.float64, device="cuda")[None, :, None]
        xx = torch.arange(nxt, dtype=torch.float64, device="cuda")[None, None, :]
        smooth = 1.05 * (zz + 0.5) + 2.0 * torch.sin(2 * np.pi * xx / nxt) * torch.cos(2 * np.pi * yy / nyt)
        sigma_s = DataArray(smooth.contiguous(), ("Z", "Y", "X"), name="sigma")
        rec("f4", "transform linear, smooth stratification (same sizes)",
            timeit(lambda: gz.transform(phi, "Z", levels, target_data=sigma_s), a.reps), nzt * cols, (2 * nzt + mt) * 8 / nzt)
        zo = torch.arange(nzt + 1, dtype=torch.float64, device="cuda")[:, None, None]
        smooth_o = 1.05 * zo + 2.0 * torch.sin(2 * np.pi * xx / nxt) * torch.cos(2 * np.pi * yy / nyt)
        sigma_so = DataArray(smooth_o.contiguous(), ("Zp1", "Y", "X"), name="sigma")
        rec("f4", "transform conservative, smooth stratification (same sizes)",
            timeit(lambda: gz.transform(phi, "Z", edges, target_data=sigma_so, method="conservative"), max(3, a.reps // 2)),
            nzt * cols, (2 * nzt + 1 + mt) * 8 / nzt)
        del zz, yy, xx, smooth, smooth_o, sigma_s, sigma_so
        out = gz.transform(phi, "Z", levels, target_data=sigma)
        oc = gz.transform(phi, "Z", edges, target_data=sigma_o, method="conservative")
        # full-size properties: a target equal to a column's own theta returns the column; integral conserved
        ident = XT.interp_1d_linear(phi.data.permute(1, 2, 0)[:64].contiguous(), sigma.data.permute(1, 2, 0)[:64].contiguous(),
                                    sigma.data[:, 7, 11].contiguous(), mask_edges=False)
        ok_ident = bool(torch.equal(ident[7, 11], phi.data[:, 7, 11]))
        tot_in = phi.data.sum(0)
        tot_out = torch.nan_to_num(oc.data, nan=0.0).sum(-1)
        ok_cons = bool(torch.allclose(tot_in, tot_out, rtol=1e-10, atol=1e-9))
        print(json.dumps({"config": "f4", "check": "linear identity column; conservative column integrals at full size",
                          "ok": ok_ident and ok_cons, "dims": list(out.dims)}), flush=True)
        del phi, inc, sigma, inc_o, sigma_o, out, oc
        torch.cuda.empty_cache()
    if "llc" in cfgs:
        # f2 at its motivating scale: the 13-face LLC topology (MITgcm / ECCO), LLC1080 x 50 levels and the
        # real LLC4320 horizontal grid x 3 levels (one-time halo-map construction is reported separately)
        import time as _time

        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        from test_topology import LLC  # the connectivity table (data)

        for n, nzl in ((1080, 50), (4320, 3)):
            dsl = Dataset({}, {"i": ("i", np.arange(n) + 0.5), "i_g": ("i_g", np.arange(n) * 1.0),
                               "j": ("j", np.arange(n) + 0.5), "j_g": ("j_g", np.arange(n) * 1.0),
                               "face": ("face", np.arange(13))})
            gl = Grid(dsl, coords={"X": {"center": "i", "left": "i_g"}, "Y": {"center": "j", "left": "j_g"}},
                      face_connections=LLC, padding="fill", autoparse_metadata=False)
            Tl = DataArray(D.synthetic((nzl, 13, n, n), 81), ("k", "face", "j", "i"))
            cl = nzl * 13 * n * n
            t0 = _time.perf_counter(); gl.diff(Tl, "X"); torch.cuda.synchronize()
            print(json.dumps({"config": "llc", "note": f"LLC{n}: first diff incl. token-map construction + upload", "s": round(_time.perf_counter() - t0, 2)}), flush=True)
            for ax in ("X", "Y"):
                rec("llc", f"diff(T,'{ax}') on LLC{n} x {nzl} levels (13 faces, f64)", timeit(lambda: gl.diff(Tl, ax), a.reps), cl, 16)
            del Tl
            torch.cuda.empty_cache()
            Ul = DataArray(D.synthetic((nzl, 13, n, n), 82), ("k", "face", "j", "i_g"))
            Vl = DataArray(D.synthetic((nzl, 13, n, n), 83), ("k", "face", "j_g", "i"))
            gl.vorticity(Ul, Vl, metric_weighted=False)
            rec("llc", f"vorticity fused on LLC{n} x {nzl} levels (vector halos)", timeit(lambda: gl.vorticity(Ul, Vl, metric_weighted=False), a.reps), cl, 24)
            if n == 1080:
                ch = gl.diff({"Y": Vl}, "X", other_component={"X": Ul}) - gl.diff({"X": Ul}, "Y", other_component={"Y": Vl})
                print(json.dumps({"config": "llc", "check": "LLC1080 fused vorticity == operator chain bit for bit", "ok": bool(torch.equal(gl.vorticity(Ul, Vl, metric_weighted=False).data, ch.data))}), flush=True)
                del ch
            del Ul, Vl, gl
            torch.cuda.empty_cache()
    if "5" in cfgs:
        run_config5(ranks, reps=a.reps)
    if "5x" in cfgs:
        nz5, n5 = 90, 4320
        grid = mitgcm_grid(nz5, n5, n5)
        grid_fill = Grid(grid._ds, coords={"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"}},
                         padding="fill", metrics={("X", "Y"): ["rAz"]}, autoparse_metadata=False)
        U = DataArray(D.synthetic((nz5, n5, n5), 51), ("Z", "YC", "XG"))
        V = DataArray(D.synthetic((nz5, n5, n5), 52), ("Z", "YG", "XC"))
        c5 = nz5 * n5 * n5
        rec(5, "vorticity fused (diff(v,X)-diff(u,Y))/rAz, fill", timeit(lambda: grid_fill.vorticity(U, V), a.reps), c5, 24 + 8 / nz5)

        def chain():
            return (grid_fill.diff(V, "X") - grid_fill.diff(U, "Y")) / grid_fill._ds["rAz"].reset_coords(drop=True)

        rec(5, "vorticity unfused operator chain (4 kernels), fused-equivalent bytes", timeit(chain, max(3, a.reps // 2)), c5, 24 + 8 / nz5)
        ok = bool(torch.equal(grid_fill.vorticity(U, V).data, chain().data))
        print(json.dumps({"config": 5, "check": "fused == unfused chain bit for bit at full size", "ok": ok}), flush=True)
        grid_div = Grid(grid._ds, coords={"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"}},
                        padding="fill", autoparse_metadata=False)
        rec(5, "divergence fused diff(u,X)+diff(v,Y) (f1, docs/ufunc_examples.md), fill", timeit(lambda: grid_div.divergence(U, V, metric_weighted=False), a.reps), c5, 24)
        okd = bool(torch.equal(grid_div.divergence(U, V, metric_weighted=False).data, (grid_div.diff(U, "X") + grid_div.diff(V, "Y")).data))
        print(json.dumps({"config": 5, "check": "fused divergence == operator chain bit for bit at full size", "ok": okd}), flush=True)
        T5 = DataArray(D.synthetic((nz5, n5, n5), 53), ("Z", "YC", "XC"))
        rec(5, "gradient fused (diff(T,X), diff(T,Y)) (f1), fill: 1 read + 2 writes", timeit(lambda: grid_div.gradient(T5), a.reps), c5, 24)
        rec(5, "gradient as two diff calls, fused-equivalent bytes", timeit(lambda: (grid_div.diff(T5, "X"), grid_div.diff(T5, "Y")), a.reps), c5, 24)
        gx, gy = grid_div.gradient(T5)
        okg = bool(torch.equal(gx.data, grid_div.diff(T5, "X").data) and torch.equal(gy.data, grid_div.diff(T5, "Y").data))
        del gx, gy
        rec(5, "flux fused (u*interp(T,X), v*interp(T,Y)) (f1), fill: 3 reads + 2 writes", timeit(lambda: grid_div.flux(U, V, T5), a.reps), c5, 40)
        rec(5, "flux as operator chain (4 kernels), fused-equivalent bytes", timeit(lambda: (U * grid_div.interp(T5, "X"), V * grid_div.interp(T5, "Y")), max(3, a.reps // 2)), c5, 40)
        fx, fy = grid_div.flux(U, V, T5)
        okf = bool(torch.equal(fx.data, (U * grid_div.interp(T5, "X")).data) and torch.equal(fy.data, (V * grid_div.interp(T5, "Y")).data))
        print(json.dumps({"config": 5, "check": "fused gradient / flux == operator chains bit for bit at full size", "ok": okg and okf}), flush=True)
        del fx, fy
        # the second-order chains in one pass: divergence(flux(u, v, T)) and the finite-volume del2 (five 2-D metric planes)
        m2 = lambda seed, dims: DataArray(D.synthetic((n5, n5), seed, 0, 1000.0, 1000.0), dims)  # noqa: E731
        ds2 = Dataset({"dxC": grid._ds["dxC"], "dyC": grid._ds["dyC"], "dyG": m2(35, ("YC", "XG")), "dxG": m2(36, ("YG", "XC")),
                       "rA": m2(37, ("YC", "XC"))},
                      {"XC": ("XC", np.arange(n5) + 0.5), "XG": ("XG", np.arange(n5) * 1.0),
                       "YC": ("YC", np.arange(n5) + 0.5), "YG": ("YG", np.arange(n5) * 1.0), "Z": ("Z", np.arange(nz5) + 0.5)})
        g2 = Grid(ds2, coords={"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"}},
                  padding={"X": "periodic", "Y": "extend"}, autoparse_metadata=False,
                  metrics={("X",): ["dxC", "dxG"], ("Y",): ["dyC", "dyG"], ("X", "Y"): ["rA"]})

        def adv_chain():
            return g2.divergence(*g2.flux(U, V, T5))

        def lap_chain():
            gx, gy = g2.gradient(T5, metric_weighted=True)
            return g2.divergence(gx * g2.get_metric(gx, ("Y",)), gy * g2.get_metric(gy, ("X",)))

        rec(5, "flux_divergence fused divergence(flux(u,v,T))/rA, periodic/extend: 3 reads + 1 write", timeit(lambda: g2.flux_divergence(U, V, T5), a.reps), c5, 32 + 8 / nz5)
        rec(5, "flux_divergence as its chain (flux + divergence), fused-equivalent bytes", timeit(adv_chain, a.reps), c5, 32 + 8 / nz5)
        oka = bool(torch.equal(g2.flux_divergence(U, V, T5).data, adv_chain().data))
        print(json.dumps({"config": 5, "check": "fused flux_divergence == chain bit for bit at full size", "ok": oka}), flush=True)
        rec(5, "laplacian fused (dxC, dyC, dyG, dxG, rA), periodic/extend: 1 read + 1 write", timeit(lambda: g2.laplacian(T5), a.reps), c5, 16 + 40 / nz5)
        rec(5, "laplacian as its chain (gradient, 2 products, divergence), fused-equivalent bytes", timeit(lap_chain, a.reps), c5, 16 + 40 / nz5)
        okl = bool(torch.equal(g2.laplacian(T5).data, lap_chain().data))
        print(json.dumps({"config": 5, "check": "fused laplacian == chain bit for bit at full size", "ok": okl}), flush=True)
        # the 3-D tracer flux divergence (u, v, w, T) / (rA * drF) in one pass against its seven-launch chain
        ds3 = Dataset({"rA": g2._ds["rA"], "drF": grid._ds["drF"]},
                      {"XC": ("XC", np.arange(n5) + 0.5), "XG": ("XG", np.arange(n5) * 1.0), "YC": ("YC", np.arange(n5) + 0.5),
                       "YG": ("YG", np.arange(n5) * 1.0), "Z": ("Z", np.arange(nz5) + 0.5), "Zl": ("Zl", np.arange(nz5) * 1.0)})
        g3 = Grid(ds3, coords={"X": {"center": "XC", "left": "XG"}, "Y": {"center": "YC", "left": "YG"},
                               "Z": {"center": "Z", "left": "Zl"}},
                  padding={"X": "periodic", "Y": "extend", "Z": "fill"}, autoparse_metadata=False,
                  metrics={("X", "Y"): ["rA"], ("Z",): ["drF"]})
        U3 = U._replace(dims=("Z", "YC", "XG"))
        V3 = V._replace(dims=("Z", "YG", "XC"))
        W3 = DataArray(D.synthetic((nz5, n5, n5), 54), ("Zl", "YC", "XC"))

        def adv3_chain():
            fx, fy = g3.flux(U3, V3, T5)
            fz = W3 * g3.interp(T5, "Z")
            out = g3.divergence(fx, fy, metric_weighted=False) + g3.diff(fz, "Z")
            return out / g3.get_metric(out, ("X", "Y", "Z"))

        rec(5, "flux_divergence_3d fused (u, v, w, T) / (rA * drF), periodic/extend/fill: 4 reads + 1 write", timeit(lambda: g3.flux_divergence_3d(U3, V3, W3, T5), a.reps), c5, 40)
        rec(5, "flux_divergence_3d as its chain (7 launches), fused-equivalent bytes", timeit(adv3_chain, max(3, a.reps // 2)), c5, 40)
        ok3 = bool(torch.equal(g3.flux_divergence_3d(U3, V3, W3, T5).data, adv3_chain().data))
        print(json.dumps({"config": 5, "check": "fused flux_divergence_3d == chain bit for bit at full size", "ok": ok3}), flush=True)
        del W3
        # w from continuity, -cumsum(divergence(u, v), Z) / rA, in one pass against its four-launch chain (transports in)

        def wcont_chain():
            d = g3.divergence(U3, V3, metric_weighted=False)
            w = -g3.cumsum(d, "Z", to="left")
            return w / g3.get_metric(w, ("X", "Y"))

        rec(5, "vertical_velocity fused -cumsum(divergence(u, v), Z) / rA, periodic/extend/fill: 2 reads + 1 write", timeit(lambda: g3.vertical_velocity(U3, V3), a.reps), c5, 24 + 8 / nz5)
        rec(5, "vertical_velocity as its chain (4 launches), fused-equivalent bytes", timeit(wcont_chain, max(3, a.reps // 2)), c5, 24 + 8 / nz5)
        okw = bool(torch.equal(g3.vertical_velocity(U3, V3).data, wcont_chain().data))
        print(json.dumps({"config": 5, "check": "fused vertical_velocity == chain bit for bit at full size", "ok": okw}), flush=True)
        del T5, U3, V3
        torch.cuda.empty_cache()
        # the momentum side on the MITgcm grid (dxC, dyC, rAz; periodic / extend) with f at the vorticity point: kinetic energy
        # and the vector-invariant advection term in one pass each against their chains of six / twenty launches of the
        # operators above, timed in turns with them
        F5 = DataArray(D.synthetic((n5, n5), 55, 0, 1.0e-4, 0.0), ("YG", "XG"))

        def ke_chain():
            return 0.5 * (grid.interp(U * U, "X") + grid.interp(V * V, "Y"))

        def mom_chain():
            zeta = grid.vorticity(U, V) + F5
            ke = 0.5 * (grid.interp(U * U, "X") + grid.interp(V * V, "Y"))
            vbar = grid.interp(grid.interp(V, "X"), "Y")
            ubar = grid.interp(grid.interp(U, "Y"), "X")
            gx, gy = grid.gradient(ke, metric_weighted=True)
            return grid.interp(zeta, "Y") * vbar - gx, -(grid.interp(zeta, "X") * ubar) - gy

        rk = max(3, a.reps // 2)
        t_f, t_c = timeit_interleaved(lambda: grid.kinetic_energy(U, V), ke_chain, rk)
        rec(5, "kinetic_energy fused 0.5*(interp(u*u,X)+interp(v*v,Y)), periodic/extend: 2 reads + 1 write", t_f, c5, 24)
        rec(5, "kinetic_energy as its chain (6 launches), fused-equivalent bytes", t_c, c5, 24)
        okk = bool(torch.equal(grid.kinetic_energy(U, V).data, ke_chain().data))
        print(json.dumps({"config": 5, "check": "fused kinetic_energy == chain bit for bit at full size", "ok": okk,
                          "speedup": round(t_c / t_f, 2)}), flush=True)
        t_f, t_c = timeit_interleaved(lambda: grid.momentum_advection(U, V, F5), mom_chain, rk)
        rec(5, "momentum_advection fused (rAz, dxC, dyC, coriolis), periodic/extend: 2 reads + 2 writes", t_f, c5, 32 + 32 / nz5)
        rec(5, "momentum_advection as its chain (20 launches), fused-equivalent bytes", t_c, c5, 32 + 32 / nz5)
        gu, gv = grid.momentum_advection(U, V, F5)
        wu, wv = mom_chain()
        okm = bool(torch.equal(gu.data, wu.data) and torch.equal(gv.data, wv.data))
        print(json.dumps({"config": 5, "check": "fused momentum_advection == chain bit for bit at full size", "ok": okm,
                          "speedup": round(t_c / t_f, 2)}), flush=True)
        del U, V, F5
        torch.cuda.empty_cache()
    if cfgs & {"5x", "5pg"}:
        run_pressure_gradient(a.reps)
    if cfgs & {"5x", "5vm"}:
        run_vertical_momentum_advection(a.reps)
    if cfgs & {"5x", "5hv"}:
        run_horizontal_viscosity(a.reps)
    if cfgs & {"5x", "5vd"}:
        run_vertical_diffusion(a.reps)
    if cfgs & {"5x", "5iv"}:
        run_implicit_vertical_diffusion(a.reps)
    if cfgs & {"5x", "5ri"}:
        run_richardson_number(a.reps)
    if "5vv" in cfgs:   # (not part of 5x: about 120 GB)
        run_implicit_vertical_viscosity(a.reps, *(shp or (90, 4320, 4320)))
    if "5pp" in cfgs:   # (not part of 5x: about 180 GB)
        run_richardson_mixing(a.reps)
    if "5is" in cfgs:   # (not part of 5x: about 120 GB)
        run_isopycnal_slope(a.reps)
    if "5rt" in cfgs:   # (not part of 5x: about 190 GB)
        run_redi_tensor(a.reps)
    if "5rf" in cfgs:   # (not part of 5x: about 125 GB)
        run_redi_vertical_flux_divergence(a.reps)
    if "5bv" in cfgs:   # (not part of 5x: about 190 GB)
        run_bolus_velocity(a.reps, *((shp[0], shp[2]) if shp else (90, 4320)))
    if "5ru" in cfgs:   # (not part of 5x: about 165 GB)
        run_redi_horizontal_tensor(a.reps, *((shp[0], shp[2]) if shp else (90, 4320)))
    ranks.close()


if __name__ == "__main__":
    main()
