#!/usr/bin/env python3
"""TFLOP/s of the probe's low-precision GEMM (fp8, mxfp8, mxfp4: lowp.h, 128x128x128 tile, plain
double-buffered loop) beside the bf16 production kernel of the same tree, at 2048^3 and 4096^3.
One process; after a warm-up every round runs the four GEMMs back to back on one stream (overlap=0,
a 1 MiB HBM test), each timed by device events around its launch, so the dtypes alternate. Prints
the median per dtype and the ratio to bf16.

    python scripts/gemm_lowp_rates.py [rounds] > profiles/lowp_gemm_rates.json
"""
from __future__ import annotations

import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpupool.ops import lowp, probe  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 20
probe.init()
out = {"rounds": rounds, "what": "median TFLOP/s of one N^3 GEMM launch, device events, dtypes alternating",
       "sizes": {}}
for n in (2048, 4096):
    kw = dict(hbm_bytes=1 << 20, patterns=1, gemm_n=n, overlap=0, mfma_low_precision=lowp.DTYPES)
    for _ in range(3):
        assert probe.run(0, **kw)["passed"]
    t: dict[str, list[float]] = {"bf16": [], **{d: [] for d in lowp.DTYPES}}
    for _ in range(rounds):
        r = probe.run(0, **kw)
        assert r["passed"], r
        t["bf16"].append(r["mfma"]["tflops"])
        for d in lowp.DTYPES:
            t[d].append(r["lowp"][d]["tflops"])
    med = {k: round(statistics.median(v), 1) for k, v in t.items()}
    out["sizes"][str(n)] = {"tflops": med, "min": {k: round(min(v), 1) for k, v in t.items()},
                            "max": {k: round(max(v), 1) for k, v in t.items()},
                            "ratio_to_bf16": {k: round(med[k] / med["bf16"], 3) for k in lowp.DTYPES}}
probe.trim(0)
print(json.dumps(out, indent=1))
