#!/usr/bin/env python3
"""Times `device.richardson_number` (K7n) at 4320 x 4320 x 90 in its forms: with / without b, with / without the metrics (a
profile, or three volumes), Z:left / Z:outer, float64 / float32 -- five repetitions each, the median and every round, one JSON
line per form on stdout.

    python tools/ri_forms.py > profiles/richardson_number/forms_full_size.jsonl"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xgcm_amd import device as D  # noqa: E402

nz, n = 90, 4320


def timed(fn, reps=5):
    fn()
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)


for dtype, item in ((torch.float64, 8), (torch.float32, 4)):
    B, U, V = (D.synthetic((nz, n, n), s).to(dtype) for s in (63, 51, 52))
    for outer in (True, False):
        nf = nz + outer
        prof = D.synthetic((nf, 1, 1), 34, 0, 10.0, 10.0).to(dtype)
        forms = [("Ri profile metric", B, (prof, prof, prof)), ("Ri no metric", B, (None, None, None)),
                 ("S2 profile metric", None, (prof, prof, None)), ("S2 no metric", None, (None, None, None))]
        if outer and item == 8:
            vol = [D.synthetic((nf, n, n), 35 + k, 0, 10.0, 10.0) for k in range(3)]
            forms.append(("Ri volume metrics", B, tuple(vol)))
        for name, b, mets in forms:
            ts = timed(lambda: D.richardson_number(b, U, V, *mets, outer, "periodic", "extend", "extend"))
            fields = (3 if b is not None else 2) + 1 + (3 if "volume" in name else 0)
            ms = ts[len(ts) // 2]
            rec = {"dtype": str(dtype), "to": "outer" if outer else "left", "form": name, "ms": round(ms, 3),
                   "rounds_ms": [round(t, 3) for t in ts], "bytes_per_cell": fields * item,
                   "frac_8TBps": round(nz * n * n * fields * item / (ms * 1e-3) / 8e12, 4)}
            print(json.dumps(rec), flush=True)
        del forms
    del B, U, V
    torch.cuda.empty_cache()
