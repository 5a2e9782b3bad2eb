"""The trans group of the probe's vector-ALU phase against a reference, on a real MI355X (run with ``-m gpu``).

The probe judges the transcendental group by consensus: every wave's digest must equal the first one
published, so a program that is wrong the same way in every wave (an opcode fed the wrong operand, a
dropped fabs, sin in radians, f64 halves folded in the wrong order, a stale-register hazard) passes it.
These tests read workgroup 0's raw-result trace (``probe.alu(want_stage=3)``: per wave, step and lane the
digest as the step began and the step's eleven result words as they were folded) and check

* exactly: the four waves agree, the digest starts at 0 and every stored digest is the fold of the step
  before, the fold of the last step is what dump stage 2 returns as row 5 and what the report's
  ``transDigest`` is the wave value of (of the production kernel's run too), and nothing is stored past
  the run's steps;
* within measured bounds: every result is finite, has the right sign and is within ``BOUNDS`` of
  ``gpupool.ops.alu.trans_reference`` at the operands the step's own stored digest gives, so every step
  is checked, not only step 0.

Then the suite sees what the probe cannot: a flip planted on every wave still passes the probe
(``test_a_trans_flip_on_every_wave_passes``) and is named here with its function, step and lane.
"""
from __future__ import annotations

import pytest

from gpupool.agent import simprobe
from gpupool.ops import alu

pytestmark = pytest.mark.gpu

SEEDS = tuple(alu.SEED_BASE + k for k in range(8))
ITERS = (1, 3, simprobe.SIM_ALU_ITERS)  # the first step, an odd count short of the trace, the library's default (64)
SEAMS = (0, 31, 32, 63)

# Error bounds per function, in gpupool.ops.alu.trans_unit's units (f32 ULP at the reference; 2^-24 for sin and
# cos; f64 ULP for the f64 pair; a log2 result below 2^-10 in ULPs of 2^-10). Nothing documents the accuracy of
# these opcodes, so each bound is the maximum measured on the MI355X over these seeds at 64 steps x 4, rounded up
# to a power of two: profiles/alu_trans_accuracy.json (scripts/alu_trans_accuracy.py), "max_error_units" and
# "bound_max_x4_pow2". tests/unit/test_alu_trans_reference.py holds the table to that file and to the caps (a
# quarter of a planted flip: 64 for the f32 words, 2^38 for the f64 results).
BOUNDS = {
    "exp2": 4,  # measured maximum 0.759 ULP
    "log2": 4,  # 0.993
    "rcp": 4,  # 0.855
    "rsq": 4,  # 0.810
    "sqrt": 4,  # 0.888
    "sin": 16,  # 2.02 units of 2^-24
    "cos": 16,  # 2.03
    "rcp_f64": 1 << 30,  # 2.43e8 f64 ULP: the opcode delivers about 24 bits, a seed for Newton steps
    "rsq_f64": 1 << 30,  # 2.44e8
}

_runs: dict = {}


@pytest.fixture(scope="module")
def hip(native_built):
    from gpupool.ops import probe
    n = probe.init()
    assert n >= 1, "no HIP device visible"
    return probe


def _trace(hip, seed: int, iters: int, **hooks) -> dict:
    """One stage-3 run, shared and read-only: the report with "data" uint32 [4][64][12][64]."""
    key = (seed, iters, tuple(sorted((k, tuple(v)) for k, v in hooks.items())))
    if key not in _runs:
        r = hip.alu(0, iters=iters, want_stage=3, requireAllCUs=0, aluSeed=seed, **hooks)
        assert "data" in r, r
        r["data"].setflags(write=False)
        _runs[key] = r
    return _runs[key]


@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("seed", SEEDS)
def test_trace_is_the_chain_the_verdict_folds(hip, seed, iters):
    r = _trace(hip, seed, iters)
    assert r["passed"] and r["iters"] == iters and r["splitWaves"] == 0, {k: v for k, v in r.items() if k != "data"}
    assert list(r)[-3:] == ["dumpCU", "dumpSimds", "data"], list(r)
    assert 0 <= r["dumpCU"] < 2048 and len(r["dumpSimds"]) == 4 and all(0 <= s < 4 for s in r["dumpSimds"]), r["dumpSimds"]
    t = r["data"]
    assert t.shape == (alu.WAVES, alu.TRACE_STEPS, alu.TRACE_WORDS, alu.LANES) and t.dtype == "uint32"
    assert (t[1:] == t[0]).all(), "the four waves' traces differ"
    # hs[0] == 0, hs[t + 1] is the fold of step t's eleven words from hs[t], steps iters..63 are zero
    assert alu.trace_chain_errors(t[0], iters) == []
    last = alu.trace_fold(t[0], iters - 1)
    # the fold of the last stored step is the digest the verdict compares: row 5 of a stage-2 dump ...
    d = hip.alu(0, iters=iters, want_stage=2, requireAllCUs=0, aluSeed=seed)
    assert d["passed"] and d["data"].shape == (4, 6, 64)
    assert (d["data"][:, 5] == last).all(), "the trace's last fold is not the group's final digest"
    # ... and the 64-bit consensus value is the wave value of those 64 digests: in this run, in the stage-2
    # run and in a run of the production kernel (no hook, no dump)
    want = f"{alu.wave_value(last):016x}"
    plain = hip.alu(0, iters=iters, requireAllCUs=0, aluSeed=seed)
    assert plain["passed"] and "dumpCU" not in plain
    assert r["transDigest"] == d["transDigest"] == plain["transDigest"] == want, (r["transDigest"], d["transDigest"],
                                                                                  plain["transDigest"], want)


@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("seed", SEEDS)
def test_every_result_is_within_its_bound_of_the_reference(hip, seed, iters):
    t = _trace(hip, seed, iters)["data"][0]
    worst = {f: 0.0 for f in alu.TRANS_FUNCS}
    for func, step, lane, ops, got, ref in alu.trace_samples(t, iters, seed):
        err, _ = alu.trans_error(func, got, ref)
        worst[func] = max(worst[func], err if err is not None else float("inf"))
    print(f"seed {seed:#x} x {iters} steps, max error in units: " + ", ".join(f"{f} {e:.4g}" for f, e in worst.items()))
    bad = alu.trace_accuracy(t, iters, seed, BOUNDS)
    assert not bad, f"{len(bad)} result(s) off the reference, first:\n" + "\n".join(bad[:8])


def test_log2_results_judged_in_the_absolute_unit_are_rare(hip):
    """log2|b| near b = +-1 loses relative accuracy; such results (below 2^-10) are not left out but judged
    in ULPs of 2^-10, and they are at most 0.1 % of the samples."""
    n = small = 0
    for seed in SEEDS:
        for func, step, lane, ops, got, ref in alu.trace_samples(_trace(hip, seed, ITERS[-1])["data"][0], ITERS[-1], seed):
            if func == "log2":
                n += 1
                small += abs(ref) < alu.LOG_FLOOR
    print(f"{small} of {n} log2 results below 2^-10")
    assert n == 8 * 64 * 64 and small <= n // 1000, (small, n)


def _only_failure(hip, flip, func):
    step, lane = flip[1], flip[2]
    r = _trace(hip, SEEDS[0], ITERS[-1], injectAluFlip=flip)
    # the probe cannot see it: every wave carries the same flip, the consensus holds
    assert r["passed"] and r["ok"] and r["splitWaves"] == 0 and r["badWaves"] == 0, {k: v for k, v in r.items() if k != "data"}
    assert r["transDigest"] != _trace(hip, SEEDS[0], ITERS[-1])["transDigest"]
    t = r["data"]
    assert (t[1:] == t[0]).all() and alu.trace_chain_errors(t[0], ITERS[-1]) == []  # the flipped word is what was folded
    # up to and including the flipped step the trace is the clean run's with that one bit changed in the last word
    want = _trace(hip, SEEDS[0], ITERS[-1])["data"][0, :step + 1].copy()
    want[step, alu.TRACE_WORDS - 1, lane] ^= 1 << flip[3]
    assert (t[0, :step + 1] == want).all()
    bad = alu.trace_accuracy(t[0], ITERS[-1], SEEDS[0], BOUNDS)
    assert len(bad) == 1 and bad[0].startswith(f"{func} seed {SEEDS[0]:#x} step {step} lane {lane}: "), bad
    return bad[0]


def test_the_flip_the_probe_passes_is_named(hip):
    """injectAluFlip=[5, 0, 0, 31] on every wave (test_a_trans_flip_on_every_wave_passes): the sign of rsq_f64."""
    assert "wrong sign" in _only_failure(hip, [5, 0, 0, 31], "rsq_f64")


@pytest.mark.parametrize("lane", SEAMS)
@pytest.mark.parametrize("step", (0, ITERS[-1] - 1))
def test_a_flipped_bit_40_of_an_f64_result_is_named(hip, step, lane):
    line = _only_failure(hip, [5, step, lane, 8], "rsq_f64")  # bit 8 of the high word
    assert "error" in line and "wrong sign" not in line, line
