#!/usr/bin/env python3
"""What spec.probe.aluCheck needs to cover every SIMD, what it costs in the claim-time probe at which
step count, and that the default probe did not move.

(a) ``aluBlocksPerCU`` 1, 2, 4, 8, 16: the vector-ALU phase alone on the GPU (probe.alu) and inside the
    overlapped claim probe (probe.run, 1 GiB, gemm_n=2048) at both positions on the MFMA stream
    ("aluFirst" 0 and 1), ``--runs`` runs each, the factors interleaved. Per factor and setting: the
    minimum and the histogram of simdsVerified, the p50 of the kernel's ms and of the claim probe's
    ms. The kernel owns nothing (ordinary register counts, no LDS), so coverage is per (CU, SIMD)
    and rests on the dispatcher. The default factor is the smallest one whose every run verified
    4 x CUs SIMDs alone and inside the probe at the default position.
(b) ``aluIters`` 1, 2, 4, ... 1024 at the library's default factor and position, each alternating with the
    claim probe without the phase for ``--rounds`` rounds (one step count at a time: the library keeps one
    expectation table per context): p50 of the probe's own ms per step count,
    what the phase adds, and the kernel's time per step (slope of its p50 ms alone on the GPU over
    the step count). The default is the largest power of two that adds no more than the register
    check's recorded +0.060 ms (README, profiles/regs_claim_probe_cost.json).
(c) Claim probe without the phase, with it behind the MFMA phase ("aluFirst":0) and ahead of it
    ("aluFirst":1), at the library's defaults, alternating for ``--rounds`` rounds.
(d) With ``--parent-lib DIR`` (a build of the parent commit's libmi355x_probe.so): child processes
    that load this tree's library or the parent's, alternating, ``--rounds`` each; a child warms up
    and reports the p50 of 30 default probes. With ``--parent-lib-copy DIR2`` (a second copy of the
    same build) the same procedure runs on the parent's library against itself: the difference of
    that null pair is what a difference must exceed.

    python scripts/alu_claim_probe_cost.py [--runs 200] [--rounds 40] [--parent-lib DIR [--parent-lib-copy DIR2]] \\
        > profiles/alu_claim_probe_cost.json
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
ITERS = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024)
BUDGET_MS = 0.060  # what the register check adds (README)
med = statistics.median


def sweep(probe, cus: int, runs: int) -> dict:
    alone = {f: {"verified": [], "ms": []} for f in FACTORS}
    inside = {first: {f: {"verified": [], "ms": [], "probe_ms": []} for f in FACTORS} for first in (0, 1)}
    for r in range(runs):
        for f in (FACTORS if r % 2 == 0 else FACTORS[::-1]):
            a = probe.alu(0, aluBlocksPerCU=f, requireAllCUs=0)
            assert a["badWaves"] == 0 and a["splitWaves"] == 0 and a["workgroups"] == f * cus, a
            alone[f]["verified"].append(a["simdsVerified"])
            alone[f]["ms"].append(a["ms"])
        for first in (0, 1):
            for f in (FACTORS if r % 2 == 0 else FACTORS[::-1]):
                p = probe.run(0, alu_check=True, aluBlocksPerCU=f, aluFirst=first, requireAllCUs=0, **KW)
                assert p["alu"]["badWaves"] == 0 and p["alu"]["splitWaves"] == 0 and p["hbm"]["ok"] and p["mfma"]["ok"], p
                inside[first][f]["verified"].append(p["alu"]["simdsVerified"])
                inside[first][f]["ms"].append(p["alu"]["ms"])
                inside[first][f]["probe_ms"].append(p["ms"])
        if (r + 1) % 50 == 0:
            print(f"sweep: run {r + 1}/{runs}", file=sys.stderr, flush=True)

    def fold(d: dict) -> dict:
        out = {"min_simds_verified": min(d["verified"]),
               "runs_short_of_every_simd": sum(v < 4 * cus for v in d["verified"]),
               "simds_verified_histogram": dict(sorted(collections.Counter(d["verified"]).items())),
               "alu_ms_p50": round(med(d["ms"]), 4)}
        if "probe_ms" in d:
            out["claim_probe_ms_p50"] = round(med(d["probe_ms"]), 4)
        return out
    names = {0: "inside_the_claim_probe_behind_the_mfma_phase", 1: "inside_the_claim_probe_ahead_of_the_mfma_phase"}
    res = {"runs": runs, "cus": cus, "alone": {str(f): fold(alone[f]) for f in FACTORS}}
    for first in (0, 1):
        res[names[first]] = {str(f): fold(inside[first][f]) for f in FACTORS}
        full = [f for f in FACTORS
                if min(alone[f]["verified"]) == 4 * cus and min(inside[first][f]["verified"]) == 4 * cus]
        res["smallest_factor_with_every_simd_in_every_run_aluFirst_%d" % first] = full[0] if full else None
    return res


def alternate(probe, sets: list, rounds: int) -> tuple[dict, dict, dict]:
    """Alternating rounds over option sets (name, kwargs): the probe's ms, the kernel's ms, the runs not ok."""
    for _, kw in sets:
        for _ in range(3):
            assert probe.run(0, **kw, **KW)["hbm"]["ok"]
    t: dict = {k: [] for k, _ in sets}
    kernel: dict = {k: [] for k, kw in sets if kw}
    short = {k: 0 for k, kw in sets if kw}
    for r in range(rounds):
        for k, kw in (sets if r % 2 == 0 else sets[::-1]):
            res = probe.run(0, **kw, **KW)
            assert res["hbm"]["ok"] and res["mfma"]["ok"], res
            t[k].append(res["ms"])
            if kw:
                assert res["alu"]["badWaves"] == 0 and res["alu"]["splitWaves"] == 0, res
                kernel[k].append(res["alu"]["ms"])
                short[k] += 0 if res["alu"]["ok"] else 1
    return t, kernel, short


def iters_cost(probe, rounds: int) -> dict:
    # one step count at a time against the plain probe: the library keeps ONE expectation table per
    # context, so alternating step counts would recompute it on the host inside every probe's clock,
    # which a pool (one step count for its lifetime) never does
    p50, added, kernel, short, none = {}, {}, {}, {}, []
    for n in ITERS:
        t, k, s = alternate(probe, [("none", {}), (str(n), {"alu_check": True, "aluIters": n})], rounds)
        none += t["none"]
        p50[str(n)] = round(med(t[str(n)]), 4)
        added[str(n)] = round(med(t[str(n)]) - med(t["none"]), 4)
        kernel.update(k)
        short.update(s)
    t = {"none": none}
    p50["none"] = round(med(none), 4)
    alone = {n: med(probe.alu(0, iters=n)["ms"] for _ in range(15)) for n in ITERS}
    fits = [n for n in ITERS if added[str(n)] <= BUDGET_MS]
    return {"rounds": rounds, "budget_ms": BUDGET_MS, "claim_probe_ms_p50": p50, "added_ms_p50": added,
            "none_even_odd_rounds_ms": [round(med(t["none"][0::2]), 4), round(med(t["none"][1::2]), 4)],
            "alu_kernel_ms_beside_the_probe_p50": {k: round(med(v), 4) for k, v in kernel.items()},
            "alu_kernel_ms_alone_p50": {str(n): round(v, 4) for n, v in alone.items()},
            "kernel_us_per_step_alone": round((alone[ITERS[-1]] - alone[ITERS[0]]) / (ITERS[-1] - ITERS[0]) * 1e3, 4),
            "largest_power_of_two_within_budget": max(fits) if fits else None,
            "runs_short_of_coverage": short}


def position_cost(probe, rounds: int) -> dict:
    sets = [("none", {}), ("alu behind the MFMA phase", {"alu_check": True, "aluFirst": 0}),
            ("alu ahead of the MFMA phase", {"alu_check": True, "aluFirst": 1})]
    t, kernel, short = alternate(probe, sets, rounds)
    p50 = {k: round(med(v), 4) for k, v in t.items()}
    return {"rounds": rounds, "claim_probe_ms_p50": p50,
            "added_ms_p50": {k: round(v - p50["none"], 4) for k, v in p50.items() if k != "none"},
            "none_even_odd_rounds_ms": [round(med(t["none"][0::2]), 4), round(med(t["none"][1::2]), 4)],
            "alu_kernel_ms_beside_the_probe_p50": {k: round(med(v), 4) for k, v in kernel.items()},
            "runs_short_of_coverage_at_the_defaults": short}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=40)
    parent_lib_ab.add_arguments(ap)
    ap.add_argument("--default-path-only", action="store_true", help="only (d)")
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
    out["iters_cost"] = iters_cost(probe, a.rounds)
    out["position_cost"] = position_cost(probe, a.rounds)
    probe.trim(0)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
