#!/usr/bin/env python3
"""What spec.probe.registerCheck needs to reach every CU, what it costs in the claim-time probe, and
that the default probe did not move.

(a) ``regsBlocksPerCU`` 1, 2, 4, 8, 16: the register-file phase alone on the GPU (probe.regs) and
    inside the overlapped claim probe (probe.run, 1 GiB, gemm_n=2048) at both positions on the MFMA
    stream ("regsFirst" 0 and 1), ``--runs`` runs each, the factors interleaved. Per factor and
    setting: the minimum and the histogram of cusTested, the runs with a workgroup on fewer than
    four SIMDs, the p50 of the kernel's ms and of the claim probe's ms. A workgroup of this kernel
    needs a CU empty of every other wave, so inside the probe it may wait for the HBM test's waves
    to drain. The default factor is the smallest one whose every run tested every CU alone and
    inside the probe at the default position.
(b) Claim probe without the phase, with it behind the MFMA phase ("regsFirst":0) and ahead of it
    ("regsFirst":1), at the library's default factor, alternating for ``--rounds`` rounds: p50 of
    the probe's own ms per option set.
(c) With ``--parent-lib DIR`` (a build of the parent commit's libmi355x_probe.so): child processes
    that load this tree's library or the parent's, alternating, ``--rounds`` each; a child warms up
    and reports the p50 of 30 default probes. With ``--parent-lib-copy DIR2`` (a second copy of the
    same build) the same procedure runs on the parent's library against itself: the difference of
    that null pair, not the odd/even spread of one run, is what a difference must exceed.

    python scripts/regs_claim_probe_cost.py [--runs 200] [--rounds 40] [--parent-lib DIR [--parent-lib-copy DIR2]] \\
        > profiles/regs_claim_probe_cost.json
"""
from __future__ import annotations

import argparse
import collections
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import parent_lib_ab  # noqa: E402  (beside this script)
KW = dict(hbm_bytes=1 << 30, gemm_n=2048)
FACTORS = (1, 2, 4, 8, 16)
med = statistics.median


def sweep(probe, cus: int, runs: int) -> dict:
    alone = {f: {"tested": [], "short": [], "ms": []} for f in FACTORS}
    inside = {first: {f: {"tested": [], "short": [], "ms": [], "probe_ms": []} for f in FACTORS} for first in (0, 1)}
    for r in range(runs):
        for f in (FACTORS if r % 2 == 0 else FACTORS[::-1]):
            a = probe.regs(0, regsBlocksPerCU=f, requireAllCUs=0)
            assert a["badBits"] == 0 and a["workgroups"] == f * cus, a
            alone[f]["tested"].append(a["cusTested"])
            alone[f]["short"].append(a["simdShort"])
            alone[f]["ms"].append(a["ms"])
        for first in (0, 1):
            for f in (FACTORS if r % 2 == 0 else FACTORS[::-1]):
                p = probe.run(0, reg_check=True, regsBlocksPerCU=f, regsFirst=first, requireAllCUs=0, **KW)
                assert p["regs"]["badBits"] == 0 and p["hbm"]["ok"] and p["mfma"]["ok"], p
                inside[first][f]["tested"].append(p["regs"]["cusTested"])
                inside[first][f]["short"].append(p["regs"]["simdShort"])
                inside[first][f]["ms"].append(p["regs"]["ms"])
                inside[first][f]["probe_ms"].append(p["ms"])
        if (r + 1) % 50 == 0:
            print(f"sweep: run {r + 1}/{runs}", file=sys.stderr, flush=True)

    def fold(d: dict) -> dict:
        out = {"min_cus_tested": min(d["tested"]),
               "runs_short_of_every_cu": sum(t < cus for t in d["tested"]),
               "runs_with_a_workgroup_on_fewer_than_4_simds": sum(s > 0 for s in d["short"]),
               "cus_tested_histogram": dict(sorted(collections.Counter(d["tested"]).items())),
               "regs_ms_p50": round(med(d["ms"]), 4)}
        if "probe_ms" in d:
            out["claim_probe_ms_p50"] = round(med(d["probe_ms"]), 4)
        return out
    names = {0: "inside_the_claim_probe_behind_the_mfma_phase", 1: "inside_the_claim_probe_ahead_of_the_mfma_phase"}
    res = {"runs": runs, "cus": cus, "alone": {str(f): fold(alone[f]) for f in FACTORS}}
    for first in (0, 1):
        res[names[first]] = {str(f): fold(inside[first][f]) for f in FACTORS}
        full = [f for f in FACTORS
                if min(alone[f]["tested"]) == cus and min(inside[first][f]["tested"]) == cus
                and not any(alone[f]["short"]) and not any(inside[first][f]["short"])]
        res["smallest_factor_with_every_cu_in_every_run_regsFirst_%d" % first] = full[0] if full else None
    return res


def cost(probe, rounds: int) -> dict:
    sets = [("none", {}), ("regs behind the MFMA phase", {"reg_check": True, "regsFirst": 0}),
            ("regs ahead of the MFMA phase", {"reg_check": True, "regsFirst": 1})]
    for _, kw in sets:
        for _ in range(3):
            assert probe.run(0, **kw, **KW)["hbm"]["ok"]
    t: dict[str, list[float]] = {k: [] for k, _ in sets}
    kernel: dict[str, list[float]] = {k: [] for k, _ in sets[1:]}
    short = {k: 0 for k, _ in sets[1:]}
    for r in range(rounds):
        for k, kw in (sets if r % 2 == 0 else sets[::-1]):
            res = probe.run(0, **kw, **KW)
            assert res["hbm"]["ok"] and res["mfma"]["ok"], res
            t[k].append(res["ms"])
            if kw:
                assert res["regs"]["badBits"] == 0, res
                kernel[k].append(res["regs"]["ms"])
                short[k] += 0 if res["regs"]["ok"] else 1
    p50 = {k: round(med(v), 4) for k, v in t.items()}
    return {"rounds": rounds, "claim_probe_ms_p50": p50,
            "added_ms_p50": {k: round(v - p50["none"], 4) for k, v in p50.items() if k != "none"},
            "none_even_odd_rounds_ms": [round(med(t["none"][0::2]), 4), round(med(t["none"][1::2]), 4)],
            "regs_kernel_ms_beside_the_probe_p50": {k: round(med(v), 4) for k, v in kernel.items()},
            "runs_short_of_coverage_at_the_default_factor": short}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=40)
    parent_lib_ab.add_arguments(ap)
    ap.add_argument("--default-path-only", action="store_true", help="only (c)")
    a = ap.parse_args()
    if a.child:
        return parent_lib_ab.child()
    out: dict = {"probe": "hbmBytes 1 GiB x 2 patterns, gemmN 2048, two streams"}
    # children first: this process has not touched the GPU yet
    out.update(parent_lib_ab.compare([sys.executable, os.path.abspath(__file__), "--child"], a))
    if a.default_path_only:
        print(json.dumps(out, indent=1))
        return
    from gpupool.ops import probe
    probe.init()
    cus = int(probe.identify(0)["computeUnits"])
    out["blocks_per_cu_sweep"] = sweep(probe, cus, a.runs)
    out["cost"] = cost(probe, a.rounds)
    probe.trim(0)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
