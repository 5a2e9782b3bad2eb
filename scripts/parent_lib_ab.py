#!/usr/bin/env python3
"""The claim probe of this tree's libmi355x_probe.so against a build of the parent commit's: did a
change move the probe? Shared by the ``*_claim_probe_cost.py`` scripts, and a tool of its own.

Child processes load this tree's library or the one in ``--parent-lib DIR``, alternating,
``--rounds`` each; a child warms up and reports the p50 of 30 probes' ms and of their host-side
launch time (phases.launchMs). With ``--parent-lib-copy DIR2`` (a second copy of the parent's build)
the same procedure runs on the parent's library against itself: the difference of that null pair,
not the odd/even spread of one run, is what a difference must exceed. Without ``--parent-lib`` the
only pair is this tree's library against itself.

``--opts JSON`` adds keywords of gpupool.ops.probe.run to every child's probes, e.g.
'{"lds_check": true, "reg_check": true, "alu_check": true, "atom_check": true}'.

    python scripts/parent_lib_ab.py [--rounds 40] [--parent-lib DIR [--parent-lib-copy DIR2]] [--opts JSON]
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
med = statistics.median


def child(kw: dict = KW) -> None:
    from gpupool.ops import probe
    probe.init()
    for _ in range(5):
        assert probe.run(0, **kw)["passed"]
    runs = [probe.run(0, **kw) for _ in range(30)]
    print(json.dumps({"ms": med(r["ms"] for r in runs), "launchMs": med(r["phases"]["launchMs"] for r in runs)}))


def default_path(me: list[str], libs: dict[str, str], rounds: int) -> dict:
    """``me``: the command of a child (it ends in ``child()``); ``libs``: two names -> library
    directory ("" = this tree's). Alternating child processes."""
    a, b = list(libs)
    ms: dict[str, list[float]] = {a: [], b: []}
    launch: dict[str, list[float]] = {a: [], b: []}
    for r in range(rounds):
        for which in ((a, b) if r % 2 == 0 else (b, a)):
            env = dict(os.environ)
            if libs[which]:
                env["GPUPOOL_NATIVE_DIR"] = os.path.abspath(libs[which])
            # each child is one GPU step with its own limit; a failing child ends the script
            p = subprocess.run(me, env=env, capture_output=True, text=True, timeout=120, check=True)
            res = json.loads(p.stdout.strip().splitlines()[-1])
            ms[which].append(float(res["ms"]))
            launch[which].append(float(res["launchMs"]))
        if (r + 1) % 10 == 0:
            print(f"default path {a} vs {b}: round {r + 1}/{rounds}", file=sys.stderr, flush=True)
    return {"what": "p50 over child processes of each child's p50 probe ms (30 probes)",
            f"{a}_ms": round(med(ms[a]), 4), f"{b}_ms": round(med(ms[b]), 4),
            f"{b}_even_rounds_ms": round(med(ms[b][0::2]), 4),
            f"{b}_odd_rounds_ms": round(med(ms[b][1::2]), 4),
            "difference_ms": round(med(ms[a]) - med(ms[b]), 4),
            "odd_even_spread_ms": round(abs(med(ms[b][0::2]) - med(ms[b][1::2])), 4),
            f"{a}_launch_ms": round(med(launch[a]), 4), f"{b}_launch_ms": round(med(launch[b]), 4)}


def add_arguments(ap: argparse.ArgumentParser) -> None:
    ap.add_argument("--parent-lib", default="", help="a build of the parent commit's libmi355x_probe.so")
    ap.add_argument("--parent-lib-copy", default="", help="a second copy of the parent's build: the null pair")
    ap.add_argument("--child", action="store_true", help="(internal) one child process of the A/B")


def compare(me: list[str], a: argparse.Namespace) -> dict:
    """The A/B that ``add_arguments``' options ask for: {} without --parent-lib, else "default_path"
    and, with --parent-lib-copy, "default_path_null_pair". Run it before this process touches the GPU."""
    out: dict = {}
    if a.parent_lib:
        out["default_path"] = default_path(me, {"this": "", "parent": a.parent_lib}, a.rounds)
        if a.parent_lib_copy:
            out["default_path_null_pair"] = default_path(me, {"parent_copy": a.parent_lib_copy, "parent": a.parent_lib},
                                                         a.rounds)
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--opts", default="{}", help="JSON: more keywords of probe.run for every child's probes")
    add_arguments(ap)
    a = ap.parse_args()
    kw = {**KW, **json.loads(a.opts)}
    if a.child:
        return child(kw)
    me = [sys.executable, os.path.abspath(__file__), "--child", "--opts", a.opts]
    out: dict = {"rounds": a.rounds, "probe": kw}
    out.update(compare(me, a) if a.parent_lib else
               {"this_tree_null_pair": default_path(me, {"this_again": "", "this": ""}, a.rounds)})
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
