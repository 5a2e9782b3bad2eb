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
has no expectation (the device compares it with its own consensus).
"""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np

GROUPS = ("int", "f32", "f64", "f16", "lane", "trans")
EXACT_GROUPS = 5  # the first five have a host expectation
LANES = 64
WAVES = 4  # of a workgroup
SEED_BASE = 0x414C5500  # the phase's seed is SEED_BASE + HIP device ordinal
FOLD_MUL = 0x9E3779B1
DUMP_BYTES = WAVES * len(GROUPS) * LANES * 4
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
    is ``steps`` = 1, stage 2 and the verdict ``steps`` = iters. Row 5 (``trans``) is zero: it has no
    expectation. Computed once per (seed, steps)."""
    return np.array(_expected(int(seed) & M32, int(steps)), dtype=np.uint32)
