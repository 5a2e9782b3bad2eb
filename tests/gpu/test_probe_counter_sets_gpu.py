"""The counter sets the four opt-in per-CU phases share (native/src/probe/ctx.h CounterSets) on a real
MI355X (run with ``-m gpu``).

A phase keeps two sets of device counters: a run counts into one and its workgroup 0 resets the other for
the next run. So a run that found faults leaves its set dirty for the run after next, and only the run in
between puts it right. Each phase alone: a run with the phase's flip hook fails with non-zero counts, and
the next two runs pass with every count zero; the second of them counts into the set the faulted run
used. Then the claim probe, which shares the sets with the stand-alone entry points: all four checks
pass, one phase's hook fails that block only, the same probe passes again, and so does each phase alone.

The plans are the smallest of each phase (4 KiB of LDS, one register pattern, one ALU step, one atomic
step): what alternates the sets is the run, not its size. The small plans finish too quickly for the
dispatcher to reach every CU every time, so the stand-alone runs do not require it; the counts are
what is asserted here.
"""
from __future__ import annotations

import pytest

pytestmark = pytest.mark.gpu

PROBE = dict(hbm_bytes=1 << 20, gemm_n=256)
CHECKS = dict(lds_check=True, reg_check=True, alu_check=True, atom_check=True)
# phase -> (the report block, the stand-alone call's smallest plan, a flip hook known to be decisive,
#           the count the hook must raise, every count a clean run leaves at zero)
PHASES = {
    "lds": ("lds", dict(nbytes=4096), dict(injectLdsFlipAtByte=100), "badBits", ("badBits", "badCUs")),
    "regs": ("regs", dict(patterns=1), dict(injectRegFlip=[259, 40, 1]), "badBits", ("badBits", "badCUs", "simdShort")),
    "alu": ("alu", dict(iters=1), dict(injectAluFlip=[1, 0, 9, 13]), "badWaves",
            ("badWaves", "badLanes", "badCUs", "splitWaves")),
    "atomics": ("atomics", dict(iters=1), dict(injectAtomFlip=[1, 12, 0, 63, 63]), "l2BadSlots",
                ("badCUs", "badWorkgroups", "ldsBadSlots", "l2BadSlots", "devBadSlots", "badReturns", "ticketFaults")),
}


@pytest.fixture(scope="module")
def hip(native_built):
    from gpupool.ops import probe
    n = probe.init()
    assert n >= 1, "no HIP device visible"
    return probe


def _alone(hip, phase: str, **hook) -> dict:
    _, plan, _, _, _ = PHASES[phase]
    return getattr(hip, phase)(0, **plan, requireAllCUs=0, **hook)


def _clean(block: dict, counts) -> bool:
    return block["ok"] and all(block[k] == 0 for k in counts)


@pytest.mark.parametrize("phase", list(PHASES))
def test_a_faulted_run_leaves_both_sets_clean_for_the_runs_after_it(hip, phase):
    _, _, hook, raised, counts = PHASES[phase]
    bad = _alone(hip, phase, **hook)
    assert not bad["passed"] and bad[raised] > 0, bad
    between = _alone(hip, phase)  # counts into the other set and resets the faulted run's
    assert between["passed"] and _clean(between, counts), between
    again = _alone(hip, phase)  # counts into the set the faulted run used
    assert again["passed"] and _clean(again, counts), again


def test_the_claim_probe_and_the_phases_alone_share_the_sets(hip):
    blocks = [PHASES[p][0] for p in PHASES]
    first = hip.run(0, **CHECKS, **PROBE)
    assert first["passed"] and all(_clean(first[PHASES[p][0]], PHASES[p][4]) for p in PHASES), first
    for phase, (block, _, hook, raised, counts) in PHASES.items():
        bad = hip.run(0, **CHECKS, **hook, **PROBE)
        assert not bad["passed"] and bad["hbm"]["ok"] and bad["mfma"]["ok"], bad
        assert not bad[block]["ok"] and bad[block][raised] > 0, bad[block]
        assert all(bad[b]["ok"] for b in blocks if b != block), {b: bad[b]["ok"] for b in blocks}
        again = hip.run(0, **CHECKS, **PROBE)
        assert again["passed"] and _clean(again[block], counts), again
    for phase in PHASES:
        r = _alone(hip, phase)
        assert r["passed"] and _clean(r, PHASES[phase][4]), r
