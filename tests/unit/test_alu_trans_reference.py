"""The reference the trans group of the probe's vector-ALU phase is tested against (gpupool/ops/alu.py:
trans_operands, trans_reference, wave_value, the trace comparer), on the CPU: the reference against mpmath
at 200 bits, the coverage of the operands the group feeds the opcodes, the comparer on synthetic traces
built from the reference alone (what must pass passes, every planted defect is found and named), the
bounds table of the GPU test against the measured figures it is derived from, and the constants that pin
the Python side and native/tests/test_alu_spec.cc to the same fold chain and wave value."""
from __future__ import annotations

import functools
import json
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from gpupool.ops import alu
from tests.gpu.test_probe_alu_trans_gpu import BOUNDS, ITERS, SEEDS

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEPS = 64
F32_WORDS = range(1, 8)  # the trace's words of the seven f32 results; 8..11 are the f64 halves

# (seed, steps) -> wave_value of the lanes' digests after a chain of synthetic steps whose eleven words are
# pattern_word(index(5, t, 16 + n, lane), seed) ^ hs; native/tests/test_alu_spec.cc quotes the same values
PINNED_WAVE = [(alu.SEED_BASE + 1, 1, 0xb0ce7828d128bfe8), (alu.SEED_BASE + 1, 3, 0x4ea75dfce15a94f1),
               (alu.SEED_BASE + 2, 64, 0xa2fb09cb03b5ff78)]


def _all_sets():
    """The issue's set: 8 seeds x 64 steps x 64 lanes at hs = 0 -> (seed, step, lane, a, b, q)."""
    for seed in SEEDS:
        for t in range(STEPS):
            for lane in range(alu.LANES):
                yield (seed, t, lane) + alu.trans_operands(0, t, lane, seed)


def test_reference_against_mpmath_at_200_bits():
    mp = pytest.importorskip("mpmath")
    mp.mp.prec = 200
    worst = {f: 0.0 for f in alu.TRANS_FUNCS}

    def turns(x):
        return 2 * mp.pi * (mp.mpf(x) - round(x))

    def frac(v):  # an mpf as an exact Fraction
        sign, man, exp, _ = v._mpf_
        return Fraction(-man if sign else man) * Fraction(2) ** exp

    for seed, t, lane, a, b, q in _all_sets():
        ma, mb, mq = mp.mpf(a), mp.mpf(b), mp.mpf(q)
        true = (mp.power(2, ma), mp.log(abs(mb), 2), 1 / ma, 1 / mp.sqrt(abs(mb)), mp.sqrt(abs(ma)), mp.sin(turns(a)),
                mp.cos(turns(b)), 1 / mq, 1 / mp.sqrt(abs(mq)))
        for func, ref, tv in zip(alu.TRANS_FUNCS, alu.trans_reference(a, b, q), true):
            tv = mp.mpf(tv)
            err = abs(frac(tv) - Fraction(ref)) / alu.trans_unit(func, frac(tv) if tv else 0.0)
            worst[func] = max(worst[func], float(err))
    print({f: f"{e:.3g}" for f, e in worst.items()})
    assert all(e <= 2.0 ** -20 for e in worst.values()), worst


def test_operand_coverage():
    classes, quadrants, small_log, n = set(), set(), 0, 0
    for seed, t, lane, a, b, q in _all_sets():
        n += 1
        for x in (a, b, q):
            assert math.isfinite(x) and x != 0.0 and 2.0 ** -4 <= abs(x) < 2.0 ** 4, (seed, t, lane, x)
        classes.add((math.frexp(a)[1], a < 0))
        r = a - round(a)  # the reduced sin argument, in [-1/2, 1/2] revolutions
        quadrants.add(int(math.floor(4 * (r % 1.0))))
        small_log += abs(math.log2(abs(b))) < alu.LOG_FLOOR
    assert n == 8 * 64 * 64
    assert len(classes) == 16 and {e for e, _ in classes} == set(range(-3, 5)), sorted(classes)
    assert quadrants == {0, 1, 2, 3}
    assert small_log <= n // 1000, small_log  # the log2 results judged in the absolute unit: at most 0.1 %
    # a digest other than 0 moves the operands and keeps them in the window
    ops = {alu.trans_operand_bits(h, 5, 9, SEEDS[0]) for h in (0, 1, 0xFFFFFFFF, 0x12345678)}
    assert len(ops) == 4
    for ab, bb, qb in ops:
        assert 123 <= (ab >> 23) & 0xFF <= 130 and 123 <= (bb >> 23) & 0xFF <= 130 and 1019 <= (qb >> 52) & 0x7FF <= 1026
    # the operands are words 0..3 of group 5: a and b through the f32 window, q from (high, low)
    w = [alu.pattern_word(alu.index(5, 7, o, 33), SEEDS[1]) ^ 0xABCD for o in range(4)]
    assert alu.trans_operand_bits(0xABCD, 7, 33, SEEDS[1]) == (alu.f32_bits(w[0]), alu.f32_bits(w[1]), alu.f64_bits(w[2], w[3]))


def test_reference_at_hand_values():
    e, l, r, rs, s, sn, cs, r64, rs64 = alu.trans_reference(3.0, -0.25, -4.0)
    assert (e, l, r, rs, s) == (8.0, -2.0, 1.0 / 3.0, 2.0, math.sqrt(3.0))
    assert sn == 0.0 and cs == math.cos(2 * math.pi * -0.25) and abs(cs) < 1e-16  # revolutions: sin(3 turns), cos(-1/4 turn)
    assert r64 == Fraction(-1, 4) and abs(rs64 - Fraction(1, 2)) < Fraction(1, 1 << 100)
    assert alu.trans_reference(0.25, 0.5, 2.0)[5:7] == (1.0, -1.0)  # sin(1/4 turn), cos(1/2 turn)
    assert abs(alu.rsqrt_fraction(Fraction(2)) ** 2 * 2 - 1) < Fraction(1, 1 << 100)
    # units: the f32 ULP at the reference, the floor for a small log2, 2^-24 for sin and cos, the f64 ULP
    assert alu.trans_unit("exp2", 1.5) == Fraction(1, 1 << 23) and alu.trans_unit("rcp", -0.75) == Fraction(1, 1 << 24)
    assert alu.trans_unit("log2", 2.0 ** -10) == Fraction(1, 1 << 33) == alu.trans_unit("log2", 1e-7) == alu.trans_unit("log2", 0.0)
    assert alu.trans_unit("sin", 1e-9) == alu.trans_unit("cos", 1.0) == Fraction(1, 1 << 24)
    assert alu.trans_unit("rcp_f64", Fraction(1, 3)) == Fraction(1, 1 << 54)
    assert [alu.bound_from_measured(x) for x in (0.0, 0.2, 0.25, 0.26, 1.0, 1.01, 3e6)] == [1, 1, 1, 2, 4, 8, 1 << 24]


# ------------------------------------------------------------------ synthetic traces from the reference alone
def _round(func: str, ref) -> int:
    return alu.round_to(Fraction(ref), alu.F64 if func.endswith("_f64") else alu.F32)


def _words(bits: list[int]) -> list[int]:
    """Nine result encodings -> the step's eleven words."""
    return bits[:7] + [bits[7] & alu.M32, bits[7] >> 32, bits[8] & alu.M32, bits[8] >> 32]


@functools.lru_cache(maxsize=None)
def _synthetic(seed: int, steps: int) -> np.ndarray:
    """One wave's trace as a device with correctly rounded opcodes would store it. Read-only."""
    t = np.zeros((alu.TRACE_STEPS, alu.TRACE_WORDS, alu.LANES), dtype=np.uint32)
    for lane in range(alu.LANES):
        h = 0
        for s in range(steps):
            refs = alu.trans_reference(*alu.trans_operands(h, s, lane, seed))
            words = _words([_round(f, r) for f, r in zip(alu.TRANS_FUNCS, refs)])
            t[s, 0, lane] = h
            t[s, 1:, lane] = words
            for w in words:
                h = alu.fold(h, w)
    t.setflags(write=False)
    return t


def _relink(t: np.ndarray, seed: int, steps: int, step: int, lane: int) -> None:
    """After a change to the words of (step, lane): what a device that computed them would have stored in
    the steps that follow: the changed digest, and correct results at the operands it gives."""
    for s in range(step + 1, min(steps, alu.TRACE_STEPS)):
        h = alu._fold_all(int(t[s - 1, 0, lane]), [int(x) for x in t[s - 1, 1:, lane]])
        refs = alu.trans_reference(*alu.trans_operands(h, s, lane, seed))
        t[s, 0, lane] = h
        t[s, 1:, lane] = _words([_round(f, r) for f, r in zip(alu.TRANS_FUNCS, refs)])


def test_correctly_rounded_results_pass():
    for seed, steps in ((SEEDS[0], 64), (SEEDS[3], 3), (SEEDS[7], 1)):
        t = _synthetic(seed, steps)
        assert alu.trace_chain_errors(t, steps) == []
        assert alu.trace_accuracy(t, steps, seed, {f: 1 for f in alu.TRANS_FUNCS}) == []  # half a unit, in fact
        assert alu.trace_accuracy(t, steps, seed, BOUNDS) == []
    assert not _synthetic(SEEDS[3], 3)[3:].any()


def _perturbed(func: str, got: int, ref, units: int) -> int:
    """The encoding ``units`` units (trans_unit at ``ref``) nearer to zero than ``got``: exact in the format
    while it does not cross zero, so the error against ``ref`` grows by ``units`` less the half unit of
    the rounding at most."""
    fmt = alu.F64 if func.endswith("_f64") else alu.F32
    v = alu.decode(got, fmt)
    return alu.round_to(v - (1 if v > 0 else -1) * units * alu.trans_unit(func, ref), fmt)


@pytest.mark.parametrize("word", range(1, alu.TRACE_WORDS))
def test_a_word_off_by_more_than_its_bound_is_named(word):
    seed, steps = SEEDS[2], 4
    name = alu.TRANS_WORDS[word - 1]
    func, half = name.split(".")[0], name.partition(".")[2]
    fi = alu.TRANS_FUNCS.index(func)
    for step, lane in ((0, 0), (1, 31), (3, 32), (2, 63)):
        t = _synthetic(seed, steps).copy()
        ref = alu.trans_reference(*alu.trans_operands(int(t[step, 0, lane]), step, lane, seed))[fi]
        got = alu.trans_results(t[step, 1:, lane])[fi]
        if half == "hi":  # the high word alone: a step of it is 2^32 ULP, or 2^31 where it crosses into the binade below
            t[step, word, lane] = int(t[step, word, lane]) - (BOUNDS[func] >> 31) - 1
        else:
            new = _words([0] * fi + [_perturbed(func, got, ref, BOUNDS[func] + 1)] + [0] * (8 - fi))
            t[step, word, lane] = new[word - 1]
            if half == "lo":  # with its borrow from the high word, if any
                t[step, word + 1, lane] = new[word]
        _relink(t, seed, steps, step, lane)
        assert alu.trace_chain_errors(t, steps) == []  # a wrong result folds like a right one
        bad = alu.trace_accuracy(t, steps, seed, BOUNDS)
        assert len(bad) == 1 and bad[0].startswith(f"{func} seed {seed:#x} step {step} lane {lane}: "), bad
        assert "error" in bad[0] and f"bound {BOUNDS[func]}" in bad[0], bad
        # one unit inside the bound passes: the comparer is no tighter than the table says
        if not half:
            t = _synthetic(seed, steps).copy()
            t[step, word, lane] = _perturbed(func, got, ref, BOUNDS[func] - 1)
            assert alu.trace_accuracy(t, steps, seed, BOUNDS) == []


@pytest.mark.parametrize("word,bit", [(w, 8) for w in F32_WORDS] + [(9, 8), (11, 8), (11, 31)])
def test_a_planted_flip_is_found(word, bit):
    """Bit 8 of an f32 result word and bit 40 of an f64 result (bit 8 of its high word), and the probe's
    documented blind spot, injectAluFlip=[5, 0, 0, 31]: the sign of the last word."""
    seed, steps = SEEDS[5], 64
    func = alu.TRANS_WORDS[word - 1].split(".")[0]
    for step, lane in ((0, 0), (63, 63)) + (((0, 31), (63, 32)) if word >= 8 else ()):
        t = _synthetic(seed, steps).copy()
        if func in ("sin", "cos"):  # judged where the flip is worth 256 units: results of magnitude >= 0.5
            big = [(s, l) for f, s, l, _, _, ref in alu.trace_samples(t, steps, seed) if f == func and abs(ref) >= 0.5]
            step, lane = next((c for c in big if c >= (step, lane)), big[-1])
        t[step, word, lane] ^= 1 << bit
        _relink(t, seed, steps, step, lane)
        assert alu.trace_chain_errors(t, steps) == []
        bad = alu.trace_accuracy(t, steps, seed, BOUNDS)
        assert len(bad) == 1 and bad[0].startswith(f"{func} seed {seed:#x} step {step} lane {lane}: "), bad
        assert "wrong sign" in bad[0] if bit == 31 else "error" in bad[0], bad


def test_a_broken_link_fails_the_chain_check():
    seed, steps = SEEDS[1], 3
    good = _synthetic(seed, steps)
    t = good.copy()
    t[2, 0, 17] ^= 1
    assert alu.trace_chain_errors(t, steps) == ["hs[2] is not the fold of step 1 in lane 17"]
    t = good.copy()
    t[0, 0, 5] = 1
    assert alu.trace_chain_errors(t, steps)[0] == "hs[0] is not zero in lane(s) [5]"
    t = good.copy()
    t[1, 4, 40] ^= 0x100  # a result changed after it was folded: the next digest no longer follows
    assert alu.trace_chain_errors(t, steps) == ["hs[2] is not the fold of step 1 in lane 40"]
    t = good.copy()
    t[3, 7, 0] = 1  # something stored past the run's steps
    assert alu.trace_chain_errors(t, steps) == ["steps 3..63 are not zero"]
    assert alu.trace_chain_errors(good, steps) == [] and alu.trace_chain_errors(_synthetic(SEEDS[0], 64), 64) == []


@pytest.mark.parametrize("lo", (8, 10))
def test_swapped_f64_halves_fail(lo):
    seed, steps = SEEDS[6], 2
    func = alu.TRANS_WORDS[lo - 1].split(".")[0]
    for step, lane in ((0, 0), (1, 63)):
        t = _synthetic(seed, steps).copy()
        t[step, lo, lane], t[step, lo + 1, lane] = t[step, lo + 1, lane], t[step, lo, lane]
        _relink(t, seed, steps, step, lane)
        bad = alu.trace_accuracy(t, steps, seed, BOUNDS)
        assert len(bad) == 1 and bad[0].startswith(f"{func} seed {seed:#x} step {step} lane {lane}: "), bad


def test_bounds_table_is_derived_from_the_measurement_and_fits_the_caps():
    """Each bound is the measured maximum x 4 rounded up to a power of two (profiles/alu_trans_accuracy.json,
    scripts/alu_trans_accuracy.py) and at most a quarter of the planted flip's error."""
    prof = json.load(open(os.path.join(ROOT, "profiles", "alu_trans_accuracy.json")))
    assert set(BOUNDS) == set(alu.TRANS_FUNCS) == set(prof["functions"])
    for f, p in prof["functions"].items():
        assert p["samples"] == 8 * 64 * 64 and p["not_finite"] == 0 and p["wrong_sign"] == 0, (f, p)
        assert BOUNDS[f] == alu.bound_from_measured(p["max_error_units"]) == p["bound_max_x4_pow2"], (f, p)
        assert BOUNDS[f] <= alu.TRANS_CAPS[f], (f, BOUNDS[f])
    assert alu.TRANS_CAPS == {**{f: 256 // 4 for f in alu.TRANS_FUNCS[:7]}, "rcp_f64": 2 ** 40 // 4, "rsq_f64": 2 ** 40 // 4}
    assert prof["log2_samples_below_2^-10"] <= 8 * 64 * 64 // 1000
    assert list(SEEDS) == [alu.SEED_BASE + k for k in range(8)] and tuple(ITERS) == (1, 3, 64)


# ------------------------------------------------------------------ the constants both sides are pinned to
def _chain_value(seed: int, steps: int) -> int:
    h = [0] * alu.LANES
    for t in range(steps):
        for lane in range(alu.LANES):
            hs = h[lane]
            for n in range(11):
                h[lane] = alu.fold(h[lane], alu.pattern_word(alu.index(5, t, 16 + n, lane), seed) ^ hs)
    return alu.wave_value(h)


def test_wave_value_and_fold_chain_are_pinned_on_both_sides():
    assert alu.wave_value([0] * 64) == 1  # 0 is the consensus slot's empty value
    assert alu.wave_value([1] + [0] * 63) == 0x9E3779B97F4A7C15
    assert alu.wave_value([0] * 63 + [1]) == 0x9E3779B97F4A7C15 + 126
    assert alu.wave_value([0xFFFFFFFF] * 64) == sum(0xFFFFFFFF * (0x9E3779B97F4A7C15 + 2 * l) for l in range(64)) % 2 ** 64
    assert (alu.TRACE_STEPS, alu.TRACE_WORDS, alu.TRACE_BYTES) == (64, 12, 786432)
    assert len(alu.TRANS_WORDS) == 11 and len(alu.TRANS_FUNCS) == 9
    cc = open(os.path.join(ROOT, "native", "tests", "test_alu_spec.cc")).read()
    for seed, steps, value in PINNED_WAVE:
        assert _chain_value(seed, steps) == value, (hex(seed), steps, hex(_chain_value(seed, steps)))
        assert "{0x%08xu, %d, 0x%016xull}" % (seed, steps, value) in cc, (hex(seed), steps)


def test_binding_asks_for_the_trace_and_shapes_it(monkeypatch):
    import ctypes

    from gpupool.ops import probe as hp
    seen = []

    class Lib:
        def mi355x_probe_alu(self, dev, opts, buf, n):
            seen.append((json.loads(opts), n))
            ctypes.memmove(buf, np.arange(n // 4, dtype="<u4").tobytes(), n)
            return 1

    monkeypatch.setattr(hp, "lib", lambda: Lib())
    monkeypatch.setattr(hp, "_take", lambda p: {"passed": True, "dumpCU": 5})
    r = hp.alu(0, iters=3, want_stage=3, aluSeed=7)
    assert seen == [({"aluIters": 3, "aluSeed": 7, "aluDumpStage": 3}, 786432)]
    assert r["data"].shape == (4, 64, 12, 64) and r["data"].dtype == np.uint32
    assert int(r["data"][1, 2, 3, 4]) == ((1 * 64 + 2) * 12 + 3) * 64 + 4  # wave, step, word, lane


def test_native_side(native_built):
    """native/tests/test_alu_spec.cc trans_*: wave_value and the fold chain at the same constants, the
    options and sizes of dump stage 3."""
    r = subprocess.run([os.path.join(native_built, "gpupool_tests"), "trans_"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "2 passed, 0 failed" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]
