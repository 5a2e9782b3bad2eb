"""The exact twin of the probe's vector-ALU phase (gpupool/ops/alu.py): its one rounder against numpy's and
torch's conversions on every f16 and bf16 code and on sampled f32 / f64 values (ties and subnormals
included), its FMA against the definition of a correctly rounded result, the operand windows, the lane
maps against each instruction's map written out in plain integers, and the table of digests that pins
the twin and the C++ host reference (native/src/probe/alu_ref.h, native/tests/test_alu_spec.cc) to the
same words."""
from __future__ import annotations

import os
import re
import struct
from fractions import Fraction

import numpy as np
import pytest
import torch

from gpupool.agent import simprobe
from gpupool.ops import alu

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SEED = alu.SEED_BASE + 1
SEAMS = (0, 31, 32, 63)

# (iters, group, lane, digest) at seed SEED_BASE + 1: alu.expected(SEED, iters)[group][lane];
# native/tests/test_alu_spec.cc quotes the same table against alu_ref.h
PINNED = [
    (1, 0, 0, 0x5e126bed), (1, 0, 31, 0xd6b16a73), (1, 0, 32, 0xf85258a7), (1, 0, 63, 0x6a33ec2a), (1, 1, 0, 0x7d86bc5d),
    (1, 1, 31, 0xf00e1a27), (1, 1, 32, 0x9848006b), (1, 1, 63, 0x5673358f), (1, 2, 0, 0x9e78f11a), (1, 2, 31, 0xe557af65),
    (1, 2, 32, 0xe54b04ed), (1, 2, 63, 0x3e1b419c), (1, 3, 0, 0x872e801e), (1, 3, 31, 0xefe28f2c), (1, 3, 32, 0xfe44caa7),
    (1, 3, 63, 0xfdaa3434), (1, 4, 0, 0x8722c077), (1, 4, 31, 0x4a946b7e), (1, 4, 32, 0x7f9ff23c), (1, 4, 63, 0xe2955ff9),
    (3, 0, 0, 0x96819c53), (3, 0, 31, 0xd3d309c2), (3, 0, 32, 0x56e643aa), (3, 0, 63, 0x0e853592), (3, 1, 0, 0xaa242be8),
    (3, 1, 31, 0x53ed99a5), (3, 1, 32, 0x0190999b), (3, 1, 63, 0x4ef07782), (3, 2, 0, 0x9aef41b7), (3, 2, 31, 0xf2148c0c),
    (3, 2, 32, 0x63633485), (3, 2, 63, 0x40c0bbd7), (3, 3, 0, 0xfa5f3d2e), (3, 3, 31, 0x5f0f409c), (3, 3, 32, 0x4e9f1bbf),
    (3, 3, 63, 0x0fa52211), (3, 4, 0, 0x6dcaec06), (3, 4, 31, 0x122a7564), (3, 4, 32, 0x87f090a9), (3, 4, 63, 0x862d3145),
]


def test_constants():
    assert alu.GROUPS == ("int", "f32", "f64", "f16", "lane", "trans") and alu.EXACT_GROUPS == 5
    assert [alu.group_name(g) for g in range(6)] == list(alu.GROUPS)
    assert alu.SEED_BASE == 0x414C5500 and alu.FOLD_MUL == 0x9E3779B1
    assert (alu.WAVES, alu.LANES, alu.DUMP_BYTES) == (4, 64, 4 * 6 * 64 * 4)
    assert alu.fold(0, 1) == 0x9E3779B1 and alu.fold(0x80000000, 0) == 16 * 0x9E3779B1 & 0xFFFFFFFF
    assert alu.index(4, 3, 2, 63) == (4 << 32) | (3 << 12) | (2 << 6) | 63
    # the library's defaults, as the simulated probe mirrors them, sit in options.h
    text = open(os.path.join(ROOT, "native", "src", "probe", "options.h")).read()
    ns = text[text.index("namespace alu {"):]
    assert int(re.search(r"constexpr int kIters = (\d+);", ns).group(1)) == simprobe.SIM_ALU_ITERS
    assert int(re.search(r"constexpr int kBlocksPerCU = (\d+);", ns).group(1)) == simprobe.SIM_ALU_BLOCKS_PER_CU


def test_pattern_word_is_the_hbm_tests():
    # (index, seed, value) of hbm.h's pattern_word compiled for the CPU: tests/unit/test_probe_abft_cases.py
    for idx, seed, want in ((0x0, 0x0, 0x00000000), (0x1, 0x0, 0xc80d83e3), (0x7ffff, 0x0, 0xe15030b4),
                            (0x100000000, 0x0, 0xf63a927f), (0x123456789, 0x51, 0xfebfb623), (0x2, 0x1234, 0xbcb73fe0),
                            (0xffffffff, 0x1234, 0x14970fc6), (0x100000000, 0xbeef, 0xcfe482b1)):
        assert alu.pattern_word(idx, seed) == want, (hex(idx), hex(seed))


def test_rounder_on_every_f16_code():
    """Each finite code's value rounds to the code; the midpoint to the next code and a point a quarter
    of the way round as numpy's float64 -> float16 conversion (one correct rounding) says."""
    codes = np.arange(0, 0x7C00, dtype=np.uint16)
    vals = codes.view(np.float16).astype(np.float64)
    nxt = (codes + 1).astype(np.uint16).view(np.float16).astype(np.float64)
    nxt[-1] = 65536.0  # above the largest finite value: the rounder is only asked below the overflow threshold
    mids, quarters = (vals + nxt) / 2, vals + (nxt - vals) / 4
    want_mid = mids[:-1].astype(np.float16).view(np.uint16)
    want_q = quarters[:-1].astype(np.float16).view(np.uint16)
    for c in range(0x7C00):
        v = Fraction(float(vals[c]))
        assert alu.decode(c, alu.F16) == v and alu.round_to(v, alu.F16) == c
        if c and c % 7 == 0:
            assert alu.round_to(-v, alu.F16) == c | 0x8000
        if c < 0x7BFF:
            assert alu.round_to(Fraction(float(mids[c])), alu.F16) == int(want_mid[c]), c
            assert alu.round_to(Fraction(float(quarters[c])), alu.F16) == int(want_q[c]), c
    assert alu.round_to(Fraction(0), alu.F16) == 0
    assert alu.round_to(Fraction(-1, 1 << 26), alu.F16) == 0x8000  # a negative value that rounds to zero keeps its sign


def test_rounder_on_every_bf16_code():
    """The same against torch's float32 -> bfloat16 conversion; a midpoint of two bf16 codes is a float32."""
    codes = np.arange(0, 0x7F80, dtype=np.uint32)
    vals = (codes << 16).view(np.float32)
    mids = ((codes << 16) | 0x8000).view(np.float32)  # exactly half way to the next code
    above = ((codes << 16) | 0x8001).view(np.float32)
    to_bf16 = lambda x: (torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().astype(np.uint16))  # noqa: E731
    want_mid, want_above = to_bf16(mids), to_bf16(above)
    for c in range(0x7F80):
        v = Fraction(float(vals[c]))
        assert alu.decode(c, alu.BF16) == v and alu.round_to(v, alu.BF16) == c
        if c < 0x7F7F:
            assert alu.round_to(Fraction(float(mids[c])), alu.BF16) == int(want_mid[c]), c
            assert alu.round_to(Fraction(float(above[c])), alu.BF16) == int(want_above[c]), c


def _f32(x: float) -> int:
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _f64(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_rounder_on_sampled_f32_and_f64():
    rng = np.random.default_rng(7)
    # f32: float64 samples over the whole range, subnormals and exact ties between neighbours included
    xs = list(rng.standard_normal(300) * 10.0 ** rng.integers(-44, 38, 300))
    xs += [1e-45, 7e-46, 1.4e-45, 3e-39, 1.17549435e-38, 1.1754942e-38, 3.4028234e38, 0.1, -0.1, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24]
    for bits in rng.integers(0, 0x7F7FFFFF, 200):  # ties: half way between two adjacent floats, exact in float64
        a, b = np.uint32(bits).view(np.float32), np.uint32(bits + 1).view(np.float32)
        xs.append((float(a) + float(b)) / 2)
    for x in xs:
        want = int(np.float64(x).astype(np.float32).view(np.uint32))
        assert alu.round_to(Fraction(float(x)), alu.F32) == want, x
        assert alu.decode(want, alu.F32) == Fraction(float(np.uint32(want).view(np.float32)))
    # f64: Python's float(Fraction) is one correct rounding
    for _ in range(300):
        n, d = int(rng.integers(1, 1 << 62)), int(rng.integers(1, 1 << 62))
        fr = Fraction(n, d) * Fraction(2) ** int(rng.integers(-1060, 1000))
        assert alu.round_to(fr, alu.F64) == _f64(float(fr)), fr
        assert alu.round_to(-fr, alu.F64) == _f64(-float(fr))
    for x in (5e-324, 2.5e-324, 7.4e-324, 2.2250738585072014e-308, 2.225073858507201e-308, 1.7976931348623157e308):
        assert alu.round_to(Fraction(x), alu.F64) == _f64(x)
    tie = (Fraction(1.0) + Fraction(1.0 + 2.0 ** -52)) / 2
    assert alu.round_to(tie, alu.F64) == _f64(1.0)  # to even
    assert alu.round_to(tie + Fraction(2) ** -52, alu.F64) == _f64(1.0 + 2.0 ** -51)
    assert alu.round_to(Fraction(5e-324) / 2, alu.F64) == 0 and alu.round_to(Fraction(5e-324) * 3 / 2, alu.F64) == 2


def test_fma_is_one_correct_rounding():
    """The twin's f32 FMA against the definition: no float is nearer to the exact a*b+c than the result,
    and of two equally near ones the result has the even mantissa."""
    rng = np.random.default_rng(11)
    words = [int(w) for w in rng.integers(0, 1 << 32, 3 * 400)]
    for i in range(0, len(words), 3):
        ab, bb, cb = (alu.f32_bits(w) for w in words[i:i + 3])
        a, b, c = (alu.decode(x, alu.F32) for x in (ab, bb, cb))
        if i % 9 == 0:  # force a cancellation: c = -(a*b rounded)
            cb = alu.round_to(-(a * b), alu.F32)
            c = alu.decode(cb, alu.F32)
        exact = a * b + c
        r = alu.fma(a, b, c, alu.F32)
        rv = alu.decode(r, alu.F32)
        if exact == 0:
            assert r == 0
            continue
        assert (r >> 31) == (1 if exact < 0 else 0)
        mag = r & 0x7FFFFFFF
        for other in (mag - 1, mag + 1):
            ov = alu.decode((r & 0x80000000) | other, alu.F32) if other >= 0 else -rv
            d_r, d_o = abs(exact - rv), abs(exact - ov)
            assert d_r < d_o or (d_r == d_o and mag % 2 == 0), (hex(ab), hex(bb), hex(cb))


def _trajectory(group: int, lane: int, steps: int):
    """(step, h at its start) of one lane of one non-lane group."""
    h = 0
    for t in range(steps):
        yield t, h
        for r in alu._RESULTS[group](h, t, lane, SEED):
            h = alu.fold(h, r)


@pytest.mark.parametrize("steps", (3, simprobe.SIM_ALU_ITERS))
def test_operands_stay_inside_the_window(steps):
    lanes = range(alu.LANES) if steps <= 3 else SEAMS
    for lane in lanes:
        for t, h in _trajectory(1, lane, steps):
            for b in alu.operands_f32(h, t, lane, SEED):
                assert 123 <= (b >> 23) & 0xFF <= 130  # finite, normal, 2^-4 <= |x| < 2^4
                assert Fraction(1, 16) <= abs(alu.decode(b, alu.F32)) < 16
        for t, h in _trajectory(2, lane, steps):
            for b in alu.operands_f64(h, t, lane, SEED):
                assert 1019 <= (b >> 52) & 0x7FF <= 1026
                assert Fraction(1, 16) <= abs(alu.decode(b, alu.F64)) < 16
        for t, h in _trajectory(3, lane, steps):
            for b in alu.operands_f16(h, t, lane, SEED):
                assert 13 <= (b >> 10) & 0x1F <= 16
                assert Fraction(1, 4) <= abs(alu.decode(b, alu.F16)) < 4
    # whatever the word, the window holds: sign and mantissa kept, exponent confined
    for w in (0, 0xFFFFFFFF, 0x7F800000, 0xFF800000, 0x00000001, 0x80000000, 0x7FC00000):
        b = alu.f32_bits(w)
        assert b & 0x807FFFFF == w & 0x807FFFFF and 123 <= (b >> 23) & 0xFF <= 130
        d = alu.f64_bits(w, w ^ 0x55555555)
        assert (d >> 63) == w >> 31 and d & 0xFFFFFFFF == w ^ 0x55555555 and 1019 <= (d >> 52) & 0x7FF <= 1026
        hb = alu.f16_bits(w & 0xFFFF)
        assert hb & 0x83FF == w & 0x83FF and 13 <= (hb >> 10) & 0x1F <= 16


def test_results_are_finite_and_only_f16_goes_subnormal():
    sub16 = 0
    for lane in SEAMS:
        for t, h in _trajectory(1, lane, 8):
            for r in alu.results_f32(h, t, lane, SEED)[:11]:  # the float results (the rest are integers or moved bits)
                assert 0 < (r >> 23) & 0xFF < 255 or r & 0x7FFFFFFF == 0, hex(r)
        for t, h in _trajectory(2, lane, 8):
            rs = alu.results_f64(h, t, lane, SEED)
            for lo, hi in ((rs[0], rs[1]), (rs[2], rs[3]), (rs[4], rs[5])):
                e = (hi >> 20) & 0x7FF
                assert 0 < e < 2047 or (hi & 0x7FFFFFFF) | lo == 0
        for t, h in _trajectory(3, lane, 8):
            for r in alu.results_f16(h, t, lane, SEED)[:3]:
                for half in (r & 0xFFFF, r >> 16):
                    assert (half >> 10) & 0x1F < 31
                    sub16 += (half >> 10) & 0x1F == 0 and half & 0x3FF != 0
    assert sub16 >= 0  # counted, not required: a cancelling v_pk_fma_f16 is the only way there


def test_lane_maps_against_each_instructions_map_in_plain_integers():
    rows = [list(range(16 * r, 16 * r + 16)) for r in range(4)]
    # row_shr:1 — every row moves up by one lane, its lane 0 has no source
    assert [alu.row_shr1(l) for l in range(64)] == sum(([None] + row[:-1] for row in rows), [])
    # row_ror:3 — every row rotates by three lanes towards the higher lane numbers
    assert [alu.row_ror3(l) for l in range(64)] == sum((row[-3:] + row[:-3] for row in rows), [])
    # row_bcast:15 row_mask:0xa — rows 1 and 3 take the last lane of the row below
    assert [alu.row_bcast15(l) for l in range(64)] == [None] * 16 + [15] * 16 + [None] * 16 + [47] * 16
    # v_permlane32_swap (x, y): x's upper half changes places with y's lower half
    first = [("x", l) for l in range(32)] + [("y", l) for l in range(32)]
    second = [("x", l) for l in range(32, 64)] + [("y", l) for l in range(32, 64)]
    assert [alu.permlane32_swap(l) for l in range(64)] == list(zip(first, second))
    # v_permlane16_swap (x, z): x's rows 1 and 3 change places with z's rows 0 and 2
    first = [("x", l) for l in rows[0]] + [("z", l) for l in rows[0]] + [("x", l) for l in rows[2]] + [("z", l) for l in rows[2]]
    second = [("x", l) for l in rows[1]] + [("z", l) for l in rows[1]] + [("x", l) for l in rows[3]] + [("z", l) for l in rows[3]]
    assert [alu.permlane16_swap(l) for l in range(64)] == list(zip(first, second))
    # ds_swizzle bit mode, xor 0x15 inside each half
    assert [alu.swizzle(l) for l in range(64)] == [l ^ 21 for l in range(64)] and all(alu.swizzle(l) // 32 == l // 32 for l in range(64))
    assert [alu.read_lane(t) for t in (0, 1, 2, 9)] == [37, 44, 51, 36]
    # a step of the group moves exactly these words: h = 0, so the operands are the pattern words
    h = [0] * 64
    x = [alu.pattern_word(alu.index(4, 0, 0, l), SEED) for l in range(64)]
    y = [alu.pattern_word(alu.index(4, 0, 1, l), SEED) for l in range(64)]
    z = [alu.pattern_word(alu.index(4, 0, 2, l), SEED) for l in range(64)]
    rs = alu.results_lane(h, 0, SEED)
    assert len(rs) == 64 and all(len(r) == 12 for r in rs)
    assert rs[0][0] == y[0] and rs[1][0] == x[0] and rs[16][0] == y[16] and rs[63][0] == x[62]
    assert rs[0][1] == x[13] and rs[3][1] == x[0] and rs[31][1] == x[28]
    assert rs[16][2] == x[15] and rs[15][2] == y[15] and rs[40][2] == y[40] and rs[63][2] == x[47]
    assert rs[31][3] == x[31] and rs[32][3] == y[0] and rs[0][4] == x[32] and rs[63][4] == y[63]
    assert rs[16][5] == z[0] and rs[0][5] == x[0] and rs[0][6] == x[16] and rs[48][6] == z[48]
    assert rs[9][7] == x[z[9] & 63] and rs[9][8] == y[9 ^ 21]
    assert rs[5][9] == x[37] and rs[6][9] == x[6] and all(r[10] == x[37] and r[11] == y[0] for r in rs)


def test_pinned_table():
    groups, lanes = set(), set()
    for iters, g, lane, word in PINNED:
        assert int(alu.expected(SEED, iters)[g][lane]) == word, (iters, g, lane)
        groups.add(g)
        lanes.add(lane)
    assert groups == set(range(alu.EXACT_GROUPS)) and lanes == set(SEAMS) and len(PINNED) >= 36
    e = alu.expected(SEED, 3)
    assert e.shape == (6, 64) and e.dtype == np.uint32 and not e[5].any()  # trans has no expectation
    assert (alu.expected(SEED, 1) != alu.expected(SEED, 2))[:5].all()  # the digest feeds the next step
    assert (alu.expected(SEED, 2) != alu.expected(SEED ^ 1, 2))[:5].all()
    # the C++ test quotes the same words
    cc = open(os.path.join(ROOT, "native", "tests", "test_alu_spec.cc")).read()
    for iters, g, lane, word in PINNED:
        assert "{%d, %d, %d, 0x%08x}" % (iters, g, lane, word) in cc, (iters, g, lane)
