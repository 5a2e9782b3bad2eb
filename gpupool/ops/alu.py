"""Exact twin of the probe's vector-ALU phase (native/src/probe/alu.h, alu_ref.h), for tests and scripts
that check the digests ``probe.alu(..., want_stage=...)`` returns.

Independent of the C++ reference on purpose: no float arithmetic at all. Every floating-point value is
a ``fractions.Fraction``, every result is computed exactly and rounded once by ``round_to``, one generic
round-to-nearest-even for any (exponent bits, mantissa bits), subnormals included; integers are Python
integers masked to 32 bits; the cross-lane instructions are lane maps in plain integers.

A lane keeps a 32-bit digest ``h`` per group (``GROUPS``). Step ``t`` of group ``g`` builds operand ``o``
as ``pattern_word(index(g, t, o, lane), seed) ^ h`` with ``h`` as it stood when the step began, and folds
every result ``r``, as bits: ``h = (rotl(h, 5) ^ r) * 0x9E3779B1``. Floating-point operands take sign and
mantissa from the word and a biased exponent in a window at the bias (f32 and f64 2^-4..2^4, f16
2^-2..2^2), so every result is finite and only f16 results reach the subnormal range. The ``trans`` group
has no expected digest (the device compares it with its own consensus, ``wave_value``): hardware
approximations are not bit-defined. For it the module holds a reference of the nine functions instead
(``trans_operands``, ``trans_reference``) and the comparer of a raw-result trace (``probe.alu(...,
want_stage=3)``) against it within per-function error bounds (``trace_chain_errors``,
``trace_accuracy``); that part uses float64 (``math``), ``Fraction`` and ``math.isqrt``.
"""
from __future__ import annotations

import functools
import math
import struct
from fractions import Fraction

import numpy as np

GROUPS = ("int", "f32", "f64", "f16", "lane", "trans")
EXACT_GROUPS = 5  # the first five have a host expectation
LANES = 64
WAVES = 4  # of a workgroup
SEED_BASE = 0x414C5500  # the phase's seed is SEED_BASE + HIP device ordinal
FOLD_MUL = 0x9E3779B1
DUMP_BYTES = WAVES * len(GROUPS) * LANES * 4
TRACE_STEPS, TRACE_WORDS = 64, 12  # dump stage 3: uint32 [wave][step][word][lane], word 0 the digest as the step began
TRACE_BYTES = WAVES * TRACE_STEPS * TRACE_WORDS * LANES * 4
WAVE_MUL = 0x9E3779B97F4A7C15
M64 = 0xFFFFFFFFFFFFFFFF
WRITE_LANE = 5
SWIZZLE_XOR = 0x15
M32 = 0xFFFFFFFF
F16, BF16, F32, F64 = (5, 10), (8, 7), (8, 23), (11, 52)


def group_name(g: int) -> str:
    return GROUPS[g]


def pattern_word(idx: int, seed: int) -> int:
    """hbm.h ``pattern_word`` in plain integers."""
    x = ((idx & M32) * 0x9E3779B1 & M32) ^ ((idx >> 32) * 0x85EBCA77 & M32)
    x ^= seed & M32
    x ^= x >> 15
    x = x * 0x2C1B3C6D & M32
    x ^= x >> 12
    return x


def index(group: int, step: int, operand: int, lane: int) -> int:
    return (group << 32) | (step << 12) | (operand << 6) | lane


def fold(h: int, r: int) -> int:
    return ((((h << 5) | (h >> 27)) & M32) ^ (r & M32)) * FOLD_MUL & M32


# ------------------------------------------------------------------ formats
def round_to(x: Fraction, fmt: tuple[int, int]) -> int:
    """The encoding of ``x`` rounded once to nearest-even in the binary format ``fmt`` = (exponent bits,
    mantissa bits), subnormals included. Finite results only. A negative ``x`` that rounds to zero keeps
    its sign; an exact zero is +0."""
    eb, mb = fmt
    sign = (1 << (eb + mb)) if x < 0 else 0
    a = -x if x < 0 else x
    if a == 0:
        return sign
    bias = (1 << (eb - 1)) - 1
    e = a.numerator.bit_length() - a.denominator.bit_length()  # floor(log2 a), or one above it
    if Fraction(2) ** e > a:
        e -= 1
    q = max(e, 1 - bias) - mb  # the exponent of one unit in the last place
    scaled = a / Fraction(2) ** q
    m = scaled.numerator // scaled.denominator
    rem = scaled - m
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and m & 1):
        m += 1
    # a normal m carries its hidden bit into the exponent field; so does a mantissa that rounded up
    return sign | (((q + mb + bias - 1) << mb) + m)


def decode(bits: int, fmt: tuple[int, int]) -> Fraction:
    """The value of a finite encoding."""
    eb, mb = fmt
    bias = (1 << (eb - 1)) - 1
    e = (bits >> mb) & ((1 << eb) - 1)
    m = bits & ((1 << mb) - 1)
    assert e != (1 << eb) - 1, "infinity or NaN"
    v = Fraction((1 << mb) + m) * Fraction(2) ** (e - bias - mb) if e else Fraction(m) * Fraction(2) ** (1 - bias - mb)
    return -v if (bits >> (eb + mb)) & 1 else v


def f32_bits(w: int) -> int:
    return (w & 0x807FFFFF) | ((123 + ((w >> 23) & 7)) << 23)


def f64_bits(hi: int, lo: int) -> int:
    return (((hi & 0x800FFFFF) | ((1019 + ((hi >> 20) & 7)) << 20)) << 32) | lo


def f16_bits(w16: int) -> int:
    return (w16 & 0x83FF) | ((13 + ((w16 >> 10) & 3)) << 10)


def fma(a: Fraction, b: Fraction, c: Fraction, fmt) -> int:
    """a * b + c, exact, rounded once."""
    return round_to(a * b + c, fmt)


# ------------------------------------------------------------------ the steps: results in fold order
def _words(g: int, t: int, n: int, lane: int, seed: int, h: int) -> list[int]:
    return [pattern_word(index(g, t, o, lane), seed) ^ h for o in range(n)]


def _s8(x: int) -> int:
    x &= 0xFF
    return x - 256 if x & 0x80 else x


def _s32(x: int) -> int:
    return x - (1 << 32) if x & 0x80000000 else x


def results_int(h: int, t: int, lane: int, seed: int) -> list[int]:
    a, b, c, d = _words(0, t, 4, lane, seed, h)
    ab, cd = (a << 32) | b, (c << 32) | d
    mad = (a * b + cd) & 0xFFFFFFFFFFFFFFFF
    perm = 0
    for i in range(4):  # bytes of {a, b}: 0..3 are b's, 4..7 are a's
        perm |= ((ab >> (8 * ((d >> (8 * i)) & 7))) & 0xFF) << (8 * i)
    s = (ab + cd) & 0xFFFFFFFFFFFFFFFF
    dot = (c & 0xFFFFFF) + sum(_s8(a >> (8 * i)) * _s8(b >> (8 * i)) for i in range(4))
    return [mad & M32, mad >> 32, a * c & M32, (b * d) >> 32, (a + b + c) & M32, ((a << (d & 7)) + c) & M32,
            (ab >> (c & 31)) & M32, perm, (a >> (b & 31)) & ((1 << (c & 31)) - 1), (bin(a).count("1") + b) & M32,
            32 - a.bit_length() if a else M32, s & M32, s >> 32, dot & M32]


def operands_f32(h: int, t: int, lane: int, seed: int) -> list[int]:
    """The f32 group's four operand encodings (for the window test)."""
    return [f32_bits(w) for w in _words(1, t, 4, lane, seed, h)]


def results_f32(h: int, t: int, lane: int, seed: int) -> list[int]:
    w = _words(1, t, 5, lane, seed, h)
    ab, bb, cb, db = (f32_bits(x) for x in w[:4])
    a, b, c, d = (decode(x, F32) for x in (ab, bb, cb, db))
    e = w[4]
    r = lambda x: round_to(x, F32)  # noqa: E731
    return [r(a * b + c), r(a + d), r(b * c), r(a * c + b), r(b * d + a), r(a * d), r(b * d), r(a + b), r(c + d),
            ab if a <= b else bb, cb if c >= d else db,
            int(a * 1024) & M32,  # int() truncates toward zero
            r(Fraction(_s32(e))), r(b * Fraction(2) ** ((e & 15) - 8)), cb if a < b else db]


def operands_f64(h: int, t: int, lane: int, seed: int) -> list[int]:
    w = _words(2, t, 6, lane, seed, h)
    return [f64_bits(w[0], w[1]), f64_bits(w[2], w[3]), f64_bits(w[4], w[5])]


def results_f64(h: int, t: int, lane: int, seed: int) -> list[int]:
    w = _words(2, t, 7, lane, seed, h)
    ab, bb, cb = f64_bits(w[0], w[1]), f64_bits(w[2], w[3]), f64_bits(w[4], w[5])
    a, b, c = (decode(x, F64) for x in (ab, bb, cb))
    g = decode(f32_bits(w[6]), F32)
    out: list[int] = []
    for x in (round_to(a * b + c, F64), round_to(a + c, F64), round_to(b * c, F64), round_to(g, F64)):
        out += [x & M32, x >> 32]
    out.append(round_to(a, F32))
    for x in (ab if a <= b else bb, bb if b >= c else cb):
        out += [x & M32, x >> 32]
    return out


def operands_f16(h: int, t: int, lane: int, seed: int) -> list[int]:
    w = _words(3, t, 3, lane, seed, h)
    return [f16_bits(x & 0xFFFF) for x in w] + [f16_bits(x >> 16) for x in w]


def results_f16(h: int, t: int, lane: int, seed: int) -> list[int]:
    w = _words(3, t, 6, lane, seed, h)
    lo = [decode(f16_bits(x & 0xFFFF), F16) for x in w[:3]]
    hi = [decode(f16_bits(x >> 16), F16) for x in w[:3]]
    g0, g1 = decode(f32_bits(w[3]), F32), decode(f32_bits(w[4]), F32)
    s = w[5]
    i = [((s >> (4 * k)) & 15) - 8 for k in range(4)]
    dot = 256 + ((s >> 16) & 255) + i[0] * i[2] + i[1] * i[3]
    pk = lambda f: round_to(f(*lo), F16) | (round_to(f(*hi), F16) << 16)  # noqa: E731
    return [pk(lambda a, b, c: a * b + c), pk(lambda a, b, c: a + c), pk(lambda a, b, c: b * c),
            round_to(g0, F16), round_to(g0, BF16) | (round_to(g1, BF16) << 16),
            round_to(Fraction(dot), F32), round_to(Fraction(dot), F32)]


# ---- the lane maps: for destination lane l, the source lane (None: the lane keeps ``old``)
def row_shr1(lane: int):
    return lane - 1 if lane & 15 else None


def row_ror3(lane: int) -> int:
    return (lane & ~15) | (((lane & 15) - 3) % 16)


def row_bcast15(lane: int):
    """row_bcast:15 under row_mask 0xa: rows 1 and 3 take lane 15 of the row below them."""
    return (lane & ~15) - 1 if (lane >> 4) & 1 else None


def permlane32_swap(lane: int):
    """(first, second) results of the swap of (x, y): each is ("x" | "y", source lane)."""
    return (("x", lane) if lane < 32 else ("y", lane - 32)), (("x", lane + 32) if lane < 32 else ("y", lane))


def permlane16_swap(lane: int):
    """... of (x, z): x's odd rows change places with z's even rows."""
    odd = (lane >> 4) & 1
    return (("z", lane - 16) if odd else ("x", lane)), (("z", lane) if odd else ("x", lane + 16))


def swizzle(lane: int) -> int:
    return lane ^ SWIZZLE_XOR


def read_lane(step: int) -> int:
    return (7 * step + 37) & 63


def results_lane(h: list[int], t: int, seed: int) -> list[list[int]]:
    """Per lane, the results of the lane group's step ``t`` on a wave whose digests are ``h``."""
    v = {"x": [pattern_word(index(4, t, 0, l), seed) ^ h[l] for l in range(LANES)],
         "y": [pattern_word(index(4, t, 1, l), seed) ^ h[l] for l in range(LANES)],
         "z": [pattern_word(index(4, t, 2, l), seed) ^ h[l] for l in range(LANES)]}
    x, y, z = v["x"], v["y"], v["z"]
    s = x[read_lane(t)]
    out = []
    for l in range(LANES):
        p32, p16 = permlane32_swap(l), permlane16_swap(l)
        out.append([y[l] if row_shr1(l) is None else x[row_shr1(l)], x[row_ror3(l)],
                    y[l] if row_bcast15(l) is None else x[row_bcast15(l)],
                    v[p32[0][0]][p32[0][1]], v[p32[1][0]][p32[1][1]], v[p16[0][0]][p16[0][1]], v[p16[1][0]][p16[1][1]],
                    x[z[l] & 63], y[swizzle(l)], s if l == WRITE_LANE else x[l], s, y[0]])
    return out


_RESULTS = (results_int, results_f32, results_f64, results_f16)


def _fold_all(h: int, rs: list[int]) -> int:
    for r in rs:
        h = fold(h, r)
    return h


@functools.lru_cache(maxsize=32)
def _expected(seed: int, steps: int) -> tuple:
    rows = []
    for g in range(4):
        row = []
        for l in range(LANES):
            h = 0
            for t in range(steps):
                h = _fold_all(h, _RESULTS[g](h, t, l, seed))
            row.append(h)
        rows.append(tuple(row))
    h = [0] * LANES
    for t in range(steps):
        rs = results_lane(h, t, seed)
        h = [_fold_all(h[l], rs[l]) for l in range(LANES)]
    rows.append(tuple(h))
    rows.append((0,) * LANES)
    return tuple(rows)


def expected(seed: int, steps: int) -> np.ndarray:
    """uint32 [6][64] (group, lane): every lane's digests after ``steps`` steps — the kernel's dump stage 1
    is ``steps`` = 1, stage 2 and the verdict ``steps`` = iters. Row 5 (``trans``) is zero: its digest
    hashes hardware approximations and has no expected value; what the group computes is checked from
    the stage-3 trace against ``trans_reference`` below. Computed once per (seed, steps)."""
    return np.array(_expected(int(seed) & M32, int(steps)), dtype=np.uint32)


# ------------------------------------------------------------------ trans: the reference of the nine functions
# The trace's result words 1..11 in step_trans's order, and the function each belongs to.
TRANS_FUNCS = ("exp2", "log2", "rcp", "rsq", "sqrt", "sin", "cos", "rcp_f64", "rsq_f64")
TRANS_WORDS = ("exp2", "log2", "rcp", "rsq", "sqrt", "sin", "cos", "rcp_f64.lo", "rcp_f64.hi", "rsq_f64.lo", "rsq_f64.hi")
LOG_FLOOR = 2.0 ** -10  # a log2 result below this is judged in units of ulp32(LOG_FLOOR), not of its own ULP
TRIG_UNIT = 2.0 ** -24  # sin and cos are judged in absolute units: their accuracy is absolute near the zeros


# A test bound may hide no planted defect: it is at most a quarter of the error of a flipped bit 8 of an f32
# result word (256 units; for sin and cos on results of magnitude >= 0.5) and of bit 40 of an f64 result.
TRANS_CAPS = {**{f: 64 for f in TRANS_FUNCS[:7]}, "rcp_f64": 2 ** 38, "rsq_f64": 2 ** 38}


def bound_from_measured(max_error: float) -> int:
    """A test bound from a measured maximum error, in the function's units: the maximum x 4 (a sample of
    operands does not reach an approximation's worst case), rounded up to a power of two."""
    return 1 << max(0, math.ceil(math.log2(4.0 * max_error))) if max_error > 0 else 1


def f32_value(bits: int) -> float:
    """The f32 of this encoding, as a Python float (exact)."""
    return struct.unpack("<f", struct.pack("<I", bits & M32))[0]


def f64_value(bits: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", bits & M64))[0]


def wave_value(digests) -> int:
    """The 64-bit value a wave publishes for the consensus, from its 64 lanes' trans digests: the sum over
    lanes of h * (0x9E3779B97F4A7C15 + 2 * lane) mod 2^64, with 0 (the empty slot) mapped to 1."""
    assert len(digests) == LANES
    v = sum(int(h) * (WAVE_MUL + 2 * lane) for lane, h in enumerate(digests)) & M64
    return v or 1


def trans_operand_bits(hs: int, step: int, lane: int, seed: int) -> tuple[int, int, int]:
    """The encodings of step_trans's operands: f32 a, f32 b, f64 q."""
    w = _words(5, step, 4, lane, seed, hs)
    return f32_bits(w[0]), f32_bits(w[1]), f64_bits(w[2], w[3])


def trans_operands(hs: int, step: int, lane: int, seed: int) -> tuple[float, float, float]:
    """(a, b, q) of step ``step`` of the trans group in ``lane``, ``hs`` the lane's digest as the step began.
    Python floats hold an f32 and an f64 exactly."""
    ab, bb, qb = trans_operand_bits(hs, step, lane, seed)
    return f32_value(ab), f32_value(bb), f64_value(qb)


def _turns(x: float) -> float:
    """x revolutions as radians of the reduced argument: r = x - round(x) is exact for an f32 x."""
    return 2.0 * math.pi * (x - round(x))


def rsqrt_fraction(q: Fraction, bits: int = 128) -> Fraction:
    """1 / sqrt(q) for q > 0 with at least ``bits`` - 8 > 100 correct bits, from one integer square root:
    isqrt(2^(2 bits) / q) / 2^bits, for q in the operand window [2^-4, 2^4)."""
    n = (q.denominator << (2 * bits)) // q.numerator
    return Fraction(math.isqrt(n), 1 << bits)


def trans_reference(a: float, b: float, q: float) -> tuple:
    """The true values of what step_trans computes, in its order: exp2(a), log2|b|, 1/a, 1/sqrt|b|, sqrt|a|,
    sin(2 pi a), cos(2 pi b) as float64 (v_sin_f32 and v_cos_f32 take revolutions; the argument is reduced
    exactly first), then 1/q as the exact Fraction and 1/sqrt|q| as a Fraction good to > 100 bits."""
    fb = abs(b)
    qf = Fraction(q)
    return (2.0 ** a, math.log2(fb), 1.0 / a, 1.0 / math.sqrt(fb), math.sqrt(abs(a)), math.sin(_turns(a)),
            math.cos(_turns(b)), 1 / qf, rsqrt_fraction(abs(qf)))


def _floor_log2(x) -> int:
    """floor(log2 |x|) of a non-zero float or Fraction, exactly."""
    f = Fraction(x)
    f = -f if f < 0 else f
    e = f.numerator.bit_length() - f.denominator.bit_length()
    return e - 1 if Fraction(2) ** e > f else e


def trans_unit(func: str, ref) -> Fraction:
    """The unit the error of ``func`` is counted in at the reference value ``ref``: the f32 ULP at ``ref`` for
    exp2, log2 (never below the ULP at LOG_FLOOR), rcp, rsq and sqrt; 2^-24 for sin and cos; the f64 ULP
    at ``ref`` for the two f64 functions."""
    if func in ("sin", "cos"):
        return Fraction(TRIG_UNIT)
    if func in ("rcp_f64", "rsq_f64"):
        return Fraction(2) ** (_floor_log2(ref) - 52)
    if func == "log2" and abs(ref) < LOG_FLOOR:
        return Fraction(2) ** (_floor_log2(LOG_FLOOR) - 23)
    return Fraction(2) ** (_floor_log2(ref) - 23)


def trans_results(words) -> list[int]:
    """A step's eleven result words -> the nine results' encodings (the f64 halves joined, low word first)."""
    w = [int(x) for x in words]
    return w[:7] + [w[7] | (w[8] << 32), w[9] | (w[10] << 32)]


def trans_error(func: str, got_bits: int, ref) -> tuple[float | None, str]:
    """(error in ``trans_unit`` units, what else is wrong) of a result encoding against its reference:
    the error is None and the text non-empty for a result that is not finite; the text also names a wrong
    sign (judged where the reference is at least one unit away from zero)."""
    f64 = func.endswith("_f64")
    exp_all_ones = (got_bits >> 52) & 0x7FF == 0x7FF if f64 else (got_bits >> 23) & 0xFF == 0xFF
    if exp_all_ones:
        return None, "not finite"
    got = Fraction(f64_value(got_bits) if f64 else f32_value(got_bits))
    r = Fraction(ref)
    unit = trans_unit(func, ref)
    err = float(abs(got - r) / unit)
    negative = bool(got_bits >> (63 if f64 else 31))
    wrong_sign = abs(r) >= unit and negative != (r < 0)
    return err, "wrong sign" if wrong_sign else ""


def trace_chain_errors(trace, steps: int) -> list[str]:
    """The exact properties of one wave's trace uint32 [TRACE_STEPS][12][64]: the digest starts at 0, each
    step's stored digest is the fold of the step before, and the steps past ``steps`` are zero. -> what
    does not hold ([] when all does)."""
    t = np.asarray(trace, dtype=np.uint32)
    assert t.shape == (TRACE_STEPS, TRACE_WORDS, LANES), t.shape
    n = min(int(steps), TRACE_STEPS)
    out = []
    if t[0, 0].any():
        out.append(f"hs[0] is not zero in lane(s) {np.flatnonzero(t[0, 0])[:4].tolist()}")
    for s in range(n - 1):
        for lane in np.flatnonzero(trace_fold(t, s) != t[s + 1, 0])[:4].tolist():
            out.append(f"hs[{s + 1}] is not the fold of step {s} in lane {lane}")
    if t[n:].any():
        out.append(f"steps {n}..{TRACE_STEPS - 1} are not zero")
    return out


def trace_fold(trace, step: int) -> np.ndarray:
    """uint32 [64]: every lane's digest after ``step``: the fold of its eleven words from its stored hs."""
    t = np.asarray(trace, dtype=np.uint32)
    return np.array([_fold_all(int(t[step, 0, lane]), [int(x) for x in t[step, 1:, lane]]) for lane in range(LANES)],
                    dtype=np.uint32)


def trace_samples(trace, steps: int, seed: int):
    """Every result of one wave's trace with its reference: yields (func, step, lane, operand encodings
    (a, b, q), got encoding, reference value). The operands come from the stored digest of each step."""
    t = np.asarray(trace, dtype=np.uint32)
    for s in range(min(int(steps), TRACE_STEPS)):
        for lane in range(LANES):
            ops = trans_operand_bits(int(t[s, 0, lane]), s, lane, seed)
            refs = trans_reference(f32_value(ops[0]), f32_value(ops[1]), f64_value(ops[2]))
            for func, got, ref in zip(TRANS_FUNCS, trans_results(t[s, 1:, lane]), refs):
                yield func, s, lane, ops, got, ref


def trace_accuracy(trace, steps: int, seed: int, bounds: dict) -> list[str]:
    """Every result of one wave's trace against ``trans_reference`` at the operands its stored digests give:
    finite, the right sign, and within ``bounds[func]`` units (``trans_unit``). -> one line per failure,
    naming function, seed, step, lane, operand bits, got, want and the error in units."""
    out = []
    for func, s, lane, ops, got, ref in trace_samples(trace, steps, seed):
        err, why = trans_error(func, got, ref)
        if err is None or why or err > bounds[func]:
            width = 16 if func.endswith("_f64") else 8
            out.append(f"{func} seed {seed:#x} step {s} lane {lane}: a {ops[0]:#010x} b {ops[1]:#010x} q {ops[2]:#018x} "
                       f"got {got:#0{width + 2}x} want {float(ref)!r}: "
                       + (why if err is None else f"{why + ', ' if why else ''}error {err:.4g} units, bound {bounds[func]}"))
    return out
