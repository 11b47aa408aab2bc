#!/usr/bin/env python3
"""Compact golden fixture of the reference's answers to `oracle/fuzz_against_reference.py`'s seeds 101, 102 and 103.

TEST INFRASTRUCTURE -- needs the reference package importable; the fixture it writes is all the tests need.

`fuzz_against_reference.record_stable` records, per call, the exception type the reference raised or the dims / name /
coordinates / shape of every result and its values (every k-th cell of a big one).  Stored here instead of the values:

- `digest`: 64-bit hash of the values (native byte order, -0.0 as 0.0, NaNs by position) -- equal digests = equal arrays;
- `coords_digest`: one hash over every coordinate (name, dims, values) -- coordinates must match exactly;
- `fallback`: what a result that is NOT bit for bit the reference's is held to, within the re-association tolerance of
  `fuzz_against_reference.compare`: all its values up to FULL cells; above that, SAMPLES evenly spaced cells (compared cell
  by cell) and a sketch of every cell -- the number of non-finite cells, a seeded +-1 projection of where they are, max |x|,
  sum |x| and PROJECTIONS seeded +-1 projections of the finite values.  A result within the per-cell tolerance of every
  cell is within `tolerance` on each projection; a shifted, mirrored or otherwise moved result is far outside it.

    tests/golden/fuzz_live_s{101,102,103}.npz     `meta` (JSON: seed, cases, expected outcomes) + `fallback` (float64)

`tests/test_reference_suite_live.py::test_differential_fuzz_against_the_reference` replays it.

    python oracle/make_golden_fuzz_live.py
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "fuzz_live_s{seed}.npz")
SEEDS = (101, 102, 103)
CASES = 400
FULL = 16
SAMPLES = 8
PROJECTIONS = 4


def digest(a) -> str:
    a = np.asarray(a)
    a = a.astype(a.dtype.newbyteorder("=")) if a.dtype.byteorder not in ("=", "|") else a
    h = hashlib.blake2b(repr(a.shape).encode(), digest_size=8)
    if a.dtype.kind in "fc":
        nan = np.isnan(a)
        a = np.where(nan, 0, a) + 0  # (NaNs by position; -0.0 == 0.0 as for numpy.array_equal)
        h.update(nan.tobytes())
    h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def coords_digest(named) -> str:
    """named: [(coordinate name, dims, values)] in name order; numbers by value, whatever their dtype (as numpy's array_equal)"""
    h = hashlib.blake2b(digest_size=8)
    for name, dims, values in named:
        values = np.asarray(values)
        values = values.astype(np.float64) if values.dtype.kind in "biuf" else values
        h.update(repr((name, list(dims))).encode() + digest(values).encode())
    return h.hexdigest()


def _signs(n, k):
    return np.random.default_rng([n, k]).integers(0, 2, n) * 2.0 - 1.0


def fallback(a) -> np.ndarray:
    """all values (up to FULL cells), else [non-finite count, their projection, max |x|, sum |x|, PROJECTIONS projections,
    SAMPLES sampled values]"""
    v = np.asarray(a).reshape(-1).astype(np.float64)
    n = v.size
    if n <= FULL:
        return v
    bad = ~np.isfinite(v)
    f = np.where(bad, 0.0, v)
    head = [bad.sum(), _signs(n, 0) @ bad, np.abs(f).max(), np.abs(f).sum()]
    return np.concatenate([head, [_signs(n, k) @ f for k in range(1, PROJECTIONS + 1)], v[np.linspace(0, n - 1, SAMPLES).astype(int)]])


def within(want, got, n, tol) -> str:
    """'' when fallback `got` of an n-cell result is within `tol` (per cell: tol * max(1, max |x|) + tol * |x|) of `want`,
    else what is not"""
    if n <= FULL:
        finite = np.abs(want[np.isfinite(want)])
        scale = max(1.0, float(finite.max())) if finite.size else 1.0
        ok = np.isclose(got, want, rtol=tol, atol=tol * scale, equal_nan=True)
        return "" if ok.all() else f"cells {np.flatnonzero(~ok).tolist()}"
    if got[0] != want[0] or got[1] != want[1]:
        return "non-finite cells"
    scale = max(1.0, want[2])
    if abs(got[2] - want[2]) > tol * scale + tol * want[2]:
        return "max |x|"
    # |sum w_i e_i| <= sum |e_i| <= n * tol * scale + tol * sum |x_i| (+ the rounding of the sums themselves)
    bound = n * tol * scale + tol * want[3] + 64 * np.finfo(np.float64).eps * want[3]
    if np.any(np.abs(got[3:4 + PROJECTIONS] - want[3:4 + PROJECTIONS]) > bound):
        return "sum |x| or a projection"
    s, t = want[4 + PROJECTIONS:], got[4 + PROJECTIONS:]
    if not np.isclose(t, s, rtol=tol, atol=tol * scale, equal_nan=True).all():
        return "sampled cells"
    return ""


def pack(seed, prefix):
    """a record_stable recording (`prefix`.json + .npz) -> the compact fixture of its seed"""
    with open(prefix + ".json") as f:
        rec = json.load(f)
    z = np.load(prefix + ".npz")
    chunks, at = [], 0
    for case, outcome in enumerate(rec["outcomes"]):
        for k, call in enumerate(outcome.get("calls", [])):
            for j, res in enumerate(call.get("results", [])):
                x = z[f"{case}/{k}/{j}"]
                fb = fallback(x)
                res.update(dtype=x.dtype.str, digest=digest(x), fallback=[at, int(fb.size)],
                           coords_digest=coords_digest([(c, d, z[f"{case}/{k}/{j}/coord/{c}"]) for c, d in sorted(res["coords"].items())]))
                chunks.append(fb)
                at += fb.size
    meta = {k: rec[k] for k in ("seed", "cases", "calls_per_case", "outcomes")}
    meta["what"] = ("expected outcomes of oracle/fuzz_against_reference.py's seeded calls, produced by the reference's own Grid (over the "
                    "xarray stand-in), as digests (oracle/make_golden_fuzz_live.py)")
    out = OUT.format(seed=seed)
    np.savez_compressed(out, meta=np.frombuffer(json.dumps(meta, separators=(",", ":")).encode(), dtype=np.uint8),
                        fallback=np.concatenate(chunks))
    print(f"seed {seed} -> {out} ({os.path.getsize(out)} bytes)")


def main():
    from oracle import fuzz_against_reference as F

    tmp = tempfile.mkdtemp(prefix="xgcm_fuzz_live_")
    for seed in SEEDS:
        prefix = os.path.join(tmp, f"s{seed}")
        F.record_stable(CASES, seed, prefix)
        pack(seed, prefix)


if __name__ == "__main__":
    main()
