#!/usr/bin/env python3
"""What spec.probe.mfmaLowPrecision costs in the claim-time probe, and that the default probe did
not move.

(a) One process: probe.run(1 GiB, gemm_n=2048) with no dtype, each dtype and all three, alternating
    for ``rounds`` rounds; p50 of the probe's own ms per option set.
(b) With ``--parent-lib DIR`` (a build of the parent commit's libmi355x_probe.so): child processes
    that load this tree's library or the parent's, alternating, ``rounds`` each; a child warms up
    and reports the p50 of 30 default probes. The margin a difference must exceed is the parent's
    own spread: the p50 of its odd rounds against its even rounds.

    python scripts/lowp_claim_probe_cost.py [--rounds 40] [--parent-lib DIR] > profiles/lowp_claim_probe_cost.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KW = dict(hbm_bytes=1 << 30, gemm_n=2048)


def child() -> None:
    from gpupool.ops import probe
    probe.init()
    for _ in range(5):
        assert probe.run(0, **KW)["passed"]
    print(json.dumps(statistics.median(probe.run(0, **KW)["ms"] for _ in range(30))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child()
    out: dict = {"rounds": a.rounds, "probe": "hbmBytes 1 GiB x 2 patterns, gemmN 2048, two streams"}
    if a.parent_lib:  # children first: this process has not touched the GPU yet
        ms: dict[str, list[float]] = {"this": [], "parent": []}
        for r in range(a.rounds):
            for which in (("this", "parent") if r % 2 == 0 else ("parent", "this")):
                env = dict(os.environ)
                if which == "parent":
                    env["GPUPOOL_NATIVE_DIR"] = os.path.abspath(a.parent_lib)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env,
                                   capture_output=True, text=True, timeout=120, check=True)
                ms[which].append(float(p.stdout.strip().splitlines()[-1]))
        med = statistics.median
        out["default_path"] = {
            "what": "p50 over child processes of each child's p50 probe ms (30 default probes)",
            "this_ms": round(med(ms["this"]), 4), "parent_ms": round(med(ms["parent"]), 4),
            "parent_even_rounds_ms": round(med(ms["parent"][0::2]), 4),
            "parent_odd_rounds_ms": round(med(ms["parent"][1::2]), 4),
            "difference_ms": round(med(ms["this"]) - med(ms["parent"]), 4),
            "margin_ms": round(abs(med(ms["parent"][0::2]) - med(ms["parent"][1::2])), 4)}
    from gpupool.ops import lowp, probe
    probe.init()
    sets = [(), *[(d,) for d in lowp.DTYPES], lowp.DTYPES]
    for s in sets:
        for _ in range(3):
            assert probe.run(0, mfma_low_precision=s, **KW)["passed"]
    t: dict[str, list[float]] = {"+".join(s) or "none": [] for s in sets}
    for r in range(a.rounds):
        for s in (sets if r % 2 == 0 else sets[::-1]):
            res = probe.run(0, mfma_low_precision=s, **KW)
            assert res["passed"], res
            t["+".join(s) or "none"].append(res["ms"])
    p50 = {k: round(statistics.median(v), 4) for k, v in t.items()}
    out["claim_probe_ms_p50"] = p50
    out["added_ms_p50"] = {k: round(v - p50["none"], 4) for k, v in p50.items() if k != "none"}
    probe.trim(0)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
