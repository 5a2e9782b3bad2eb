#!/usr/bin/env python3
"""How accurate the MI355X's transcendental opcodes are on the operands the vector-ALU phase feeds them:
the figures the bounds of tests/gpu/test_probe_alu_trans_gpu.py are derived from.

Runs the phase alone with the trans trace (probe.alu(want_stage=3): workgroup 0's raw results of
v_exp/log/rcp/rsq/sqrt/sin/cos_f32, v_rcp_f64 and v_rsq_f64 at every step) at 64 steps for the eight
seeds SEED_BASE + 0..7, checks the trace's exact properties (four identical waves, the digest chain),
and compares every result with gpupool.ops.alu.trans_reference at the operands the trace's own digests
give. Per function: the sample count, the maximum error in the function's units (f32 ULP at the
reference; 2^-24 for sin and cos; f64 ULP for the f64 pair; a log2 result below 2^-10 in units of the
ULP at 2^-10), the operand and result bits of the worst case, the bound the tests take (maximum x 4,
rounded up to a power of two) and the cap it has to fit under (a quarter of a planted bit flip).

    python scripts/alu_trans_accuracy.py [--out profiles/alu_trans_accuracy.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEEDS = 8
STEPS = 64


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alu_trans_accuracy.json"))
    a = ap.parse_args()
    from gpupool.ops import alu, probe
    probe.init()
    per = {f: {"samples": 0, "max_error": 0.0, "worst": None, "not_finite": 0, "wrong_sign": 0} for f in alu.TRANS_FUNCS}
    small_log = 0
    for k in range(SEEDS):
        seed = alu.SEED_BASE + k
        r = probe.alu(0, iters=STEPS, want_stage=3, requireAllCUs=0, aluSeed=seed)
        assert r["passed"] and r["iters"] == STEPS, {x: v for x, v in r.items() if x != "data"}
        t = r["data"]
        assert (t[1:] == t[0]).all(), "the four waves' traces differ"
        chain = alu.trace_chain_errors(t[0], STEPS)
        assert not chain, chain
        assert alu.wave_value(alu.trace_fold(t[0], STEPS - 1)) == int(r["transDigest"], 16), "transDigest is not the trace's fold"
        for func, step, lane, ops, got, ref in alu.trace_samples(t[0], STEPS, seed):
            p = per[func]
            p["samples"] += 1
            small_log += func == "log2" and abs(ref) < alu.LOG_FLOOR
            err, why = alu.trans_error(func, got, ref)
            p["not_finite"] += err is None
            p["wrong_sign"] += why == "wrong sign"
            if err is not None and err > p["max_error"]:
                w = 16 if func.endswith("_f64") else 8
                p["max_error"] = err
                p["worst"] = {"seed": f"{seed:#x}", "step": step, "lane": lane, "a": f"{ops[0]:#010x}", "b": f"{ops[1]:#010x}",
                              "q": f"{ops[2]:#018x}", "got": f"{got:#0{w + 2}x}", "want": repr(float(ref))}
        print(f"seed {seed:#x}: done", file=sys.stderr, flush=True)
    arch = probe.identify(0).get("gcnArch")
    probe.trim(0)
    units = {**{f: "f32 ULP at the reference" for f in alu.TRANS_FUNCS[:5]},
             "log2": "f32 ULP at the reference, of 2^-10 where |reference| < 2^-10",
             "sin": "2^-24", "cos": "2^-24", "rcp_f64": "f64 ULP at the reference", "rsq_f64": "f64 ULP at the reference"}
    out = {"what": f"probe.alu(want_stage=3), {SEEDS} seeds from {alu.SEED_BASE:#x}, {STEPS} steps, 64 lanes, workgroup 0 "
                   "(its four waves identical), against gpupool.ops.alu.trans_reference",
           "device": arch,"log2_samples_below_2^-10": small_log, "functions": {}}
    for f, p in per.items():
        bound = alu.bound_from_measured(p["max_error"])
        out["functions"][f] = {"samples": p["samples"], "unit": units[f], "max_error_units": p["max_error"], "worst": p["worst"],
                               "not_finite": p["not_finite"], "wrong_sign": p["wrong_sign"], "bound_max_x4_pow2": bound,
                               "cap": alu.TRANS_CAPS[f], "fits_under_cap": bound <= alu.TRANS_CAPS[f]}
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
