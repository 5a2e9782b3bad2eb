#!/usr/bin/env python3
"""What spec.probe.mfmaLowPrecision costs in the claim-time probe, and that the default probe did
not move.

(a) One process: probe.run(1 GiB, gemm_n=2048) with no dtype, each dtype and all three, alternating
    for ``rounds`` rounds; p50 of the probe's own ms per option set.
(b) With ``--parent-lib DIR`` (a build of the parent commit's libmi355x_probe.so): child processes
    that load this tree's library or the parent's, alternating, ``rounds`` each; a child warms up
    and reports the p50 of 30 default probes. With ``--parent-lib-copy DIR2`` (a second copy of the
    same build) the same procedure runs on the parent's library against itself: the difference of
    that null pair is what a difference must exceed (scripts/parent_lib_ab.py).

    python scripts/lowp_claim_probe_cost.py [--rounds 40] [--parent-lib DIR [--parent-lib-copy DIR2]] > profiles/lowp_claim_probe_cost.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import parent_lib_ab  # noqa: E402  (beside this script)
KW = dict(hbm_bytes=1 << 30, gemm_n=2048)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40)
    parent_lib_ab.add_arguments(ap)
    a = ap.parse_args()
    if a.child:
        return parent_lib_ab.child()
    out: dict = {"rounds": a.rounds, "probe": "hbmBytes 1 GiB x 2 patterns, gemmN 2048, two streams"}
    # children first: this process has not touched the GPU yet
    out.update(parent_lib_ab.compare([sys.executable, os.path.abspath(__file__), "--child"], a))
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
