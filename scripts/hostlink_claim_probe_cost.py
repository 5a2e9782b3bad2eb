#!/usr/bin/env python3
"""What spec.probe.hostLinkCheck costs in the claim-time probe, and that the default probe did not
move.

(a) One process: probe.run(1 GiB, gemm_n=2048, overlap) without the check and with it at 1, 2, 4, 8,
    16 and 64 MiB, on a stream of its own and as the tail of the MFMA stream ("hostLinkStream":1),
    alternating for ``rounds`` rounds; p50 of the probe's own ms per option set, and the link's
    GB/s as measured beside the other phases.
(b) With ``--parent-lib DIR`` (a build of the parent commit's libmi355x_probe.so): child processes
    that load this tree's library or the parent's, alternating, ``rounds`` each; a child warms up
    and reports the p50 of 30 default probes. With ``--parent-lib-copy DIR2`` (a second copy of the
    same build) the same procedure runs on the parent's library against itself: the difference of
    that null pair is what a difference must exceed (scripts/parent_lib_ab.py).
(c) A fresh child process's PSS after default probes, after a host-link probe on the MFMA stream
    (the pinned buffer alone) and after one on its own stream (buffer + one more hardware queue),
    with the first-use allocMs of the pinned buffer.

    python scripts/hostlink_claim_probe_cost.py [--rounds 40] [--parent-lib DIR [--parent-lib-copy DIR2]] > profiles/hostlink_claim_probe_cost.json
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
import parent_lib_ab  # noqa: E402  (beside this script)
KW = dict(hbm_bytes=1 << 30, gemm_n=2048)
MIB = 1 << 20


def pss_mib() -> float:
    with open("/proc/self/smaps_rollup") as f:
        for line in f:
            if line.startswith("Pss:"):
                return round(int(line.split()[1]) / 1024, 1)
    return 0.0


def pss_child(nbytes: int) -> None:
    from gpupool.ops import probe
    probe.init()
    for _ in range(3):
        assert probe.run(0, **KW)["passed"]
    out = {"hostLinkBytes": nbytes, "pss_mib_default": pss_mib()}
    r = probe.run(0, host_link_bytes=nbytes, hostLinkStream=1, **KW)
    assert r["passed"], r
    out["first_use_alloc_ms"] = r["hostLink"]["allocMs"]
    out["pss_mib_buffer_on_mfma_stream"] = pss_mib()
    r = probe.run(0, host_link_bytes=nbytes, **KW)
    assert r["passed"], r
    out["pss_mib_buffer_and_own_stream"] = pss_mib()
    print(json.dumps(out))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40)
    parent_lib_ab.add_arguments(ap)
    ap.add_argument("--pss-child", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return parent_lib_ab.child()
    if a.pss_child:
        return pss_child(a.pss_child)
    out: dict = {"rounds": a.rounds, "probe": "hbmBytes 1 GiB x 2 patterns, gemmN 2048, two streams"}
    me = [sys.executable, os.path.abspath(__file__)]
    # children first: this process has not touched the GPU yet
    out.update(parent_lib_ab.compare([sys.executable, os.path.abspath(__file__), "--child"], a))
    out["footprint"] = []
    for nbytes in (4 * MIB, 64 * MIB):
        p = subprocess.run(me + ["--pss-child", str(nbytes)], capture_output=True, text=True, timeout=120, check=True)
        out["footprint"].append(json.loads(p.stdout.strip().splitlines()[-1]))
    from gpupool.ops import probe
    probe.init()
    sets = [("none", {})]
    for m in (1, 2, 4, 8, 16, 64):
        sets.append((f"{m}MiB own stream", {"host_link_bytes": m * MIB}))
        sets.append((f"{m}MiB mfma stream tail", {"host_link_bytes": m * MIB, "hostLinkStream": 1}))
    for _, kw in sets[::-1]:  # largest first: the pinned buffer is grown once
        for _ in range(3):
            assert probe.run(0, **kw, **KW)["passed"]
    t: dict[str, list[float]] = {k: [] for k, _ in sets}
    link: dict[str, list[float]] = {k: [] for k, _ in sets[1:]}
    for r in range(a.rounds):
        for k, kw in (sets if r % 2 == 0 else sets[::-1]):
            res = probe.run(0, **kw, **KW)
            assert res["passed"], res
            t[k].append(res["ms"])
            if kw:
                link[k].append(res["hostLink"]["GBps"])
    p50 = {k: round(statistics.median(v), 4) for k, v in t.items()}
    out["claim_probe_ms_p50"] = p50
    out["added_ms_p50"] = {k: round(v - p50["none"], 4) for k, v in p50.items() if k != "none"}
    out["none_even_odd_rounds_ms"] = [round(statistics.median(t["none"][0::2]), 4),
                                      round(statistics.median(t["none"][1::2]), 4)]
    out["link_gbps_beside_the_probe_p50"] = {k: round(statistics.median(v), 2) for k, v in link.items()}
    probe.trim(0)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
