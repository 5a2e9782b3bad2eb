"""Host references of the probe's checker kernels (native/src/probe/abft.h, lowp.h). Needs no GPU
and no torch: ``test_probe_checkers_gpu.py`` compares the kernels with them on an MI355X,
``tests/unit/test_probe_abft_cases.py`` checks on the CPU that the references agree with each other.

Everything here is integer arithmetic: the in-probe operands are small integers, C = A x Bt^T is an
integer matrix with |C| <= 576 K < 2^53 (exact in a float64 matmul), and the six checksum vectors
are sums of those integers modulo 2^32.

    acol[k] = sum_m A[m][k]      bcol[k] = sum_n Bt[n][k]
    col_c[n] = sum_m C[m][n]     exp_col[n] = sum_k Bt[n][k] acol[k]
    row_c[m] = sum_n C[m][n]     exp_row[m] = sum_k A[m][k] bcol[k]

A checker run counts three things (``predict_counts``): elements of C that are no integer, not
finite or beyond the bound (``odd``), columns with col_c != exp_col, rows with row_c != exp_row.
For a corrupted C the expected vectors are those of the clean C (they are computed from the
operands alone), and the sums of C take each element as the kernels do: clamped to +-2e9, rounded
down to an integer, wrapped to 32 bits.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from gpupool.ops import lowp

from . import gemm_cases

MASK = 0xFFFFFFFF
BF16 = "bf16"
DTYPES = (BF16,) + lowp.DTYPES
GEN_GRID = 2048 * 256            # threads of the generator's production grid

# (seed, span) of the probe's bf16 operands: the 256^3 element check's A and B, the N^3 GEMM's A and B
BF16_SEEDS = ((0x1234, 3), (0xBEEF, 3), (0x51, 2), (0x77, 2))
SCALE_LO = {"fp8": 0, "mxfp8": 0, "mxfp4": 1}
# largest magnitude of a decoded, scaled operand
SPAN = {BF16: 2, "fp8": 8, "mxfp8": 16, "mxfp4": 24}

# (m, n, k) at the loop splits of colsum_partial (64-row blocks of 4 interleaved waves x 4 loads in
# flight; 256 fp32 / 512 bf16 columns per block) and rowdot (4 rows per block; 1024 fp32 / 2048 bf16
# columns per unrolled iteration)
BF16_SHAPES = (
    (1, 4, 8),            # one lane, one row
    (5, 260, 520),        # idle waves in the 4-row interleave, a partial first unroll; a second
                          # column block of one lane, fp32 (256 + 4) and bf16 (512 + 8)
    (65, 1028, 2056),     # a second row block of one row; rowdot fp32 1024 + 4, bf16 2048 + 8
    (100, 252, 504),      # 64 + 36 rows: a partial unroll in the second row block; one lane short of a block
    (64, 2052, 4104),     # exactly one row block; rowdot two full iterations + 4 / + 8, 9 column blocks
    (256, 256, 256),      # the element check's shape
    (512, 512, 512),      # the probe's own (tests)
)
# lowp colsum<T>: 256 32-bit words per block (k 1024 at 8 bits, 2048 at 4), 64-row slabs; rowdot<T>:
# 64 words per iteration (k 256 / 512)
LOWP_SHAPES = (
    (1, 4, 32),           # one word (8 bit: 8 words of one row), one row
    (65, 260, 1056),      # 8 bit: 264 words = a block + 8, 4 iterations + 8 words; 4 bit: 132 words =
                          # 2 iterations + 4; a second slab of one row (A), of four (Bt)
    (100, 1028, 2080),    # 8 bit: 520 words = 2 blocks + 8; 4 bit: 260 words = a block + 4; 64 + 36 rows
    (64, 516, 4128),      # 8 bit: 1032 words = 4 blocks + 8; 4 bit: 516 = 2 blocks + 4; exactly one slab
    (256, 256, 256),      # the element check's shape
)
FAULT_SHAPE = (512, 512, 512)


def shapes(dtype: str) -> tuple:
    return BF16_SHAPES if dtype == BF16 else LOWP_SHAPES


# ------------------------------------------------------------------ the generators' replicas
def pattern_word(idx, seed: int) -> np.ndarray:
    """hbm.h's pattern_word: uint32 arithmetic on a 64-bit word index."""
    idx = np.asarray(idx, dtype=np.uint64)
    lo, hi = idx & np.uint64(MASK), idx >> np.uint64(32)
    x = ((lo * np.uint64(0x9E3779B1)) & np.uint64(MASK)) ^ ((hi * np.uint64(0x85EBCA77)) & np.uint64(MASK))
    x ^= np.uint64(seed & MASK)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x2C1B3C6D)) & np.uint64(MASK)
    x ^= x >> np.uint64(12)
    return x.astype(np.uint32)


def small_int(h, span: int) -> np.ndarray:
    """The integer small_int_bf16 encodes: h mod (2 span + 1) - span."""
    return (np.asarray(h, dtype=np.uint32).astype(np.int64) % (2 * span + 1)) - span


def small_int_bf16(h, span: int) -> np.ndarray:
    """abft.h's small_int_bf16: that integer as bf16 bits (exact)."""
    return gemm_cases.bf16_bits(small_int(h, span).astype(np.float32))


def gen_bf16(count: int, seed: int, span: int) -> np.ndarray:
    """What gen_operand writes: ``count`` bf16 bit patterns."""
    return small_int_bf16(pattern_word(np.arange(count, dtype=np.uint64), seed), span)


def lowp_seeds(dtype: str) -> tuple:
    """The seeds of lowp::launch_phase_t: the 256^3 A and B, the N^3 A and B."""
    s = 0x10F0 + 0x101 * lowp.dtype_index(dtype)
    return (s, s ^ 0xBEEF, s ^ 0x51, s ^ 0x77)


def gen_lowp(dtype: str, count: int, seed: int, scale_lo: int):
    """What lowp::gen_operand<T> writes for ``count`` elements (whole 32-bit words): the operand
    bytes and the count // 32 scale bytes (None for fp8)."""
    bits = lowp.BITS[dtype]
    assert count % (32 // bits) == 0
    if bits == 8:
        v = pattern_word(np.arange(count, dtype=np.uint64), seed).astype(np.int64) % 17 - 8
        data = lowp.e4m3_encode(v)
    else:
        data = pattern_word(np.arange(count // 8, dtype=np.uint64), seed).astype("<u4").view(np.uint8)
    scales = None
    if lowp.SCALED[dtype]:
        bit = (pattern_word(np.arange(count // 32, dtype=np.uint64), seed ^ 0x5CA1E) >> np.uint32(7)) & np.uint32(1)
        scales = lowp.e8m0_encode(scale_lo + bit.astype(np.int64))
    return np.ascontiguousarray(data), scales


# ------------------------------------------------------------------ operands of a checker case
@dataclasses.dataclass(frozen=True)
class Operands:
    dtype: str
    shape: tuple
    kind: str                    # "probe": the generator's values; "max": every operand at +max
    a: np.ndarray                # as the entry points take them: bf16 bits [m][k], or bytes
    bt: np.ndarray
    scale_a: np.ndarray | None
    scale_bt: np.ndarray | None
    a_int: np.ndarray            # int64 [m][k]: the decoded, scaled values
    bt_int: np.ndarray
    c_int: np.ndarray            # int64 [m][n] = A x Bt^T
    bound: float                 # K * span^2

    @property
    def c(self) -> np.ndarray:
        """A fresh, writable fp32 C (every value is exact: |C| < 2^24 at these shapes)."""
        return self.c_int.astype(np.float32)


def _as_int(x: np.ndarray) -> np.ndarray:
    i = np.rint(x).astype(np.int64)
    assert (i == x).all(), "operands must decode to integers"
    return i


@functools.lru_cache(maxsize=None)
def operands(dtype: str, shape: tuple, kind: str = "probe") -> Operands:
    """Computed once per (dtype, shape, kind), shared, read-only."""
    m, n, k = shape
    sa = sb = None
    if dtype == BF16:
        if kind == "probe":
            a, bt = gen_bf16(m * k, 0x51, 2).reshape(m, k), gen_bf16(n * k, 0x77, 2).reshape(n, k)
        else:
            a, bt = (gemm_cases.bf16_bits(np.full(s, 2, dtype=np.float32)) for s in ((m, k), (n, k)))
        a_int, bt_int = _as_int(gemm_cases.bf16_value(a)), _as_int(gemm_cases.bf16_value(bt))
    else:
        row = k * lowp.BITS[dtype] // 8
        if kind == "probe":
            sd = lowp_seeds(dtype)
            a, sa = gen_lowp(dtype, m * k, sd[2], SCALE_LO[dtype])
            bt, sb = gen_lowp(dtype, n * k, sd[3], SCALE_LO[dtype])
        else:  # +8, or +6 in both nibbles, under the larger scale
            byte = int(lowp.e4m3_encode(np.array([8.0]))[0]) if lowp.BITS[dtype] == 8 else 0x77
            a, bt = np.full(m * row, byte, dtype=np.uint8), np.full(n * row, byte, dtype=np.uint8)
            if lowp.SCALED[dtype]:
                sa = lowp.e8m0_encode(np.full(m * k // 32, SCALE_LO[dtype] + 1))
                sb = lowp.e8m0_encode(np.full(n * k // 32, SCALE_LO[dtype] + 1))
        a, bt = a.reshape(m, row), bt.reshape(n, row)
        if sa is not None:
            sa, sb = sa.reshape(m, k // 32), sb.reshape(n, k // 32)
        a_int, bt_int = _as_int(lowp.decode_operand(dtype, a, sa)), _as_int(lowp.decode_operand(dtype, bt, sb))
    span = SPAN[dtype]
    assert np.abs(a_int).max() <= span and np.abs(bt_int).max() <= span
    c = a_int.astype(np.float64) @ bt_int.astype(np.float64).T   # exact: |C| <= 576 K < 2^53
    c_int = c.astype(np.int64)
    assert (c_int == c).all() and np.abs(c_int).max() < 1 << 24
    for x in (a, bt, sa, sb, a_int, bt_int, c_int):
        if x is not None:
            x.setflags(write=False)
    return Operands(dtype, shape, kind, a, bt, sa, sb, a_int, bt_int, c_int, float(k * span * span))


# ------------------------------------------------------------------ the six vectors and the counts
@dataclasses.dataclass(frozen=True)
class Vectors:
    acol: np.ndarray
    bcol: np.ndarray
    col_c: np.ndarray
    exp_col: np.ndarray
    row_c: np.ndarray
    exp_row: np.ndarray

    def packed(self) -> np.ndarray:
        return np.concatenate([self.acol, self.bcol, self.col_c, self.exp_col, self.row_c, self.exp_row])


def _u32(x: np.ndarray) -> np.ndarray:
    """int64 -> its value modulo 2^32 (two's complement wrap)."""
    return (np.asarray(x, dtype=np.int64) & MASK).astype(np.uint32)


def kernel_int(c: np.ndarray) -> np.ndarray:
    """An fp32 C element as the sums take it: clamped to +-2e9 (NaN -> -2e9, as fmaxf drops it),
    rounded down, as int64. Its low 32 bits are what the kernels add."""
    x = np.asarray(c, dtype=np.float32).astype(np.float64)
    x = np.where(np.isnan(x), -2.0e9, np.clip(x, -2.0e9, 2.0e9))
    return np.floor(x).astype(np.int64)


def vectors(a_int: np.ndarray, bt_int: np.ndarray, c_vals: np.ndarray) -> Vectors:
    """The six vectors from integer operands and an integer C (int64), modulo 2^32. The weights of
    the expected sums are the wrapped column sums, as in the kernels; products and sums in wrapped
    64-bit arithmetic, whose low 32 bits are exact."""
    acol, bcol = _u32(a_int.sum(axis=0)), _u32(bt_int.sum(axis=0))
    with np.errstate(over="ignore"):
        exp_col = (_u32(bt_int).astype(np.uint64) * acol.astype(np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
        exp_row = (_u32(a_int).astype(np.uint64) * bcol.astype(np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
    return Vectors(acol, bcol, _u32(c_vals.sum(axis=0)), (exp_col & np.uint64(MASK)).astype(np.uint32),
                   _u32(c_vals.sum(axis=1)), (exp_row & np.uint64(MASK)).astype(np.uint32))


def clean_vectors(o: Operands) -> Vectors:
    return vectors(o.a_int, o.bt_int, o.c_int)


def predict_counts(o: Operands, c: np.ndarray) -> tuple:
    """(odd, column mismatches, row mismatches) of a checker run over the fp32 ``c`` in place of the
    clean C of ``o``: from the corruption alone."""
    c = np.asarray(c, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        fine = (c == np.rint(c)) & (np.abs(c) <= np.float32(o.bound))   # NaN fails both
    got = kernel_int(c)
    cols = _u32(got.sum(axis=0)) != _u32(o.c_int.sum(axis=0))
    rows = _u32(got.sum(axis=1)) != _u32(o.c_int.sum(axis=1))
    return int((~fine).sum()), int(cols.sum()), int(rows.sum())


# ------------------------------------------------------------------ fault positions
def fault_positions(m: int, n: int) -> list:
    """(row, col) of every position class of the single-fault sweep: every row residue mod 64 at a
    few columns; every column residue mod 16 on both sides of each 256-column block edge (the
    matrix edges included) at a few rows; the four corners."""
    pos = []
    cols = sorted({0, n // 5, n - 1})
    for res in range(64):
        r = res if res < m else None
        if r is None:
            continue
        r2 = (m - 1) // 64 * 64 + res        # the same residue in the last row block, if it exists
        for c in cols:
            pos.append((r, c))
            if r2 < m and r2 != r:
                pos.append((r2, c))
    rows = sorted({0, m // 3, m - 1})
    edges = list(range(0, n + 1, 256))
    if edges[-1] != n:
        edges.append(n)
    for e in edges:
        for c in range(e - 16, e + 16):
            if 0 <= c < n:
                pos += [(r, c) for r in rows]
    pos += [(0, 0), (0, n - 1), (m - 1, 0), (m - 1, n - 1)]
    return sorted(set(pos))


# ------------------------------------------------------------------ calling the entry points
def _ptr(x):
    return None if x is None else x.ctypes.data


def run_check(hip, o: Operands, c: np.ndarray, faults=None):
    """mi355x_probe_abft_check on ``o`` and the fp32 ``c`` -> (packed vectors, (odd, col, row),
    per-fault counts [nfaults][3]). ``faults``: (flat indices int64, values float32). Outputs start
    as 0xFF bytes, so a call that wrote nothing cannot pass."""
    m, n, k = o.shape
    c = np.ascontiguousarray(c, dtype=np.float32)
    assert c.shape == (m, n)
    vec = np.full(2 * (m + n + k), MASK, dtype=np.uint32)
    counts = np.full(3, 2 ** 64 - 1, dtype=np.uint64)
    nf, idx, val, fc = 0, None, None, None
    if faults is not None:
        idx = np.ascontiguousarray(faults[0], dtype=np.int64)
        val = np.ascontiguousarray(faults[1], dtype=np.float32)
        nf = len(idx)
        assert len(val) == nf
        fc = np.full((nf, 3), 2 ** 64 - 1, dtype=np.uint64)
    hip.abft_check(0, o.dtype, _ptr(o.a), _ptr(o.bt), _ptr(o.scale_a), _ptr(o.scale_bt), _ptr(c), m, n, k,
                   o.bound, _ptr(vec), _ptr(counts), nf, _ptr(idx), _ptr(val), _ptr(fc))
    return vec, tuple(int(x) for x in counts), fc


def run_ref(hip, o: Operands) -> np.ndarray:
    m, n, k = o.shape
    r = gemm_cases.poisoned_c(m, n)
    hip.gemm_ref(0, o.dtype, _ptr(o.a), _ptr(o.bt), _ptr(o.scale_a), _ptr(o.scale_bt), _ptr(r), m, n, k)
    return r
