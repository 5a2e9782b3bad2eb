"""Cases, operands and references of the low-precision probe GEMM tests (fp8, mxfp8, mxfp4). Needs
no GPU and no torch: ``test_probe_lowp_gpu.py`` runs the cases on an MI355X, ``tests/unit/
test_lowp_formats.py`` checks on the CPU that the operand sets are exact and that the comparer
(``gemm_cases.check``) flags the ways a low-precision tiled kernel goes wrong.

C[m][n] (fp32) = A[m][k] x Bt[n][k]^T, operands as ``gpupool.ops.probe.gemm_lowp`` takes them: one
e4m3 byte per element (fp8, mxfp8) or two e2m1 nibbles per byte (mxfp4), E8M0 scale bytes
[rows][k/32] for the scaled dtypes. The kernel's block tile is 128x128 with BK = 128 elements.

Every expectation is exact: how the hardware orders and widens the sum inside one low-precision
MFMA is not documented, so the operands are chosen such that every partial sum is exactly
representable in fp32 (in any order for fp8 and mxfp4; see mxfp8 below) and C must equal the float64 reference bit for bit (``==``: a zero
of either sign equals zero).

``encodings``  one block tile, one K-step (128, 128, 128). A holds every finite encoding of the
               dtype, cycling over rows and K positions; Bt[n] is +-1 at k = perm(n), an asymmetric
               permutation, else 0: C[m][n] = +-A[m][perm(n)], so the OCP bias, the subnormals, 448
               and the operand lane / nibble map are each pinned by single products. Scaled dtypes
               also run with per-block A scales spread over 2^-60 .. 2^60 (``encodings-scaled``).
``exact``      the shapes below. fp8 / mxfp8 draw from the 80 e4m3 encodings that are multiples of
               1/8 with |v| <= 15, mxfp4 from all 16 e2m1 encodings; scaled dtypes take scales from
               {2^-1 .. 2^2}, random per row and block.
                 fp8    products are multiples of 2^-6 and <= 225: exact for 225 K 2^6 < 2^24, K <= 1165
                 mxfp4  products are multiples of 2^-4 and <= 576: exact for 576 K 2^4 < 2^24, K <= 1820
                 mxfp8  products are multiples of 2^-8 and <= 3600: the worst case over any order
                        does not fit 2^24 quanta beyond K = 18, so what is checked for the drawn
                        data (tests/unit/test_lowp_formats.py) is that every result, every
                        partial sum in K order and a shuffled-order fp32 sum are exact. A kernel
                        result that differs here is a finding about the order in which the
                        instruction adds, to be recorded in probe.h, not a reason for a tolerance.
                        On the MI355X all six shapes come back exact.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from gpupool.ops import lowp

from . import gemm_cases

TILE = 128
DTYPES = lowp.DTYPES
ENCODING_SHAPE = (128, 128, 128)
# 1, 2, 3, 5 and 7 K-tiles, non-square grids, 15 workgroups (no multiple of the 8 XCDs)
SHAPES = ((128, 128, 128), (128, 128, 256), (128, 256, 384), (384, 128, 640), (256, 768, 896),
          (640, 384, 384))
SCALE_EXPONENTS = (-1, 0, 1, 2)

FINITE_E4M3 = np.array([b for b in range(256) if (b & 0x7F) != 0x7F], dtype=np.uint8)     # 254
WINDOW_E4M3 = np.array([b for b in FINITE_E4M3
                        if abs(float(lowp.E4M3[b])) <= 15 and float(lowp.E4M3[b]) * 8 % 1 == 0],
                       dtype=np.uint8)                                                     # 80
QUANTUM = {"fp8": 2.0 ** -6, "mxfp8": 2.0 ** -8, "mxfp4": 2.0 ** -4}  # of one product, ``exact``
PRODUCT_MAX = {"fp8": 225.0, "mxfp8": 225.0 * 16, "mxfp4": 36.0 * 16}


@dataclasses.dataclass(frozen=True)
class Operands:
    dtype: str
    shape: tuple
    a: np.ndarray            # [m][k] bytes, or [m][k/2] packed nibbles
    bt: np.ndarray
    scale_a: np.ndarray | None   # [m][k/32] E8M0
    scale_bt: np.ndarray | None
    data: gemm_cases.Data    # what ``gemm_cases.check`` compares against (bound None: exact)


def _finish(dtype, kind, shape, a, bt, sa, sb) -> Operands:
    ref = lowp.reference(dtype, a, bt, sa, sb)
    for x in (a, bt, sa, sb, ref):
        if x is not None:
            x.setflags(write=False)
    return Operands(dtype, shape, a, bt, sa, sb, gemm_cases.Data(f"{dtype}-{kind}", shape, a, bt, ref, None))


def _codes(dtype: str, codes: np.ndarray) -> np.ndarray:
    return lowp.pack_fp4(codes) if lowp.BITS[dtype] == 4 else np.ascontiguousarray(codes, dtype=np.uint8)


def perm(n: np.ndarray) -> np.ndarray:
    """The K position of Bt row n's single +-1: a permutation of 0..127 that is not its own inverse."""
    return (37 * n + 11) % 128


@functools.lru_cache(maxsize=None)
def encodings(dtype: str, scaled_run: bool = False) -> Operands:
    m, n, k = ENCODING_SHAPE
    rows, ks = np.arange(m)[:, None], np.arange(k)[None, :]
    if lowp.BITS[dtype] == 4:
        a = ((5 * rows + ks + 3 * (ks // 32)) % 16).astype(np.uint8)  # no period of a K-block
        one, minus_one = 2, 10
    else:
        a = FINITE_E4M3[(3 * rows + ks) % len(FINITE_E4M3)]
        one, minus_one = 0x38, 0xB8
    bt = np.zeros((n, k), dtype=np.uint8)
    cols = np.arange(n)
    bt[cols, perm(cols)] = np.where(cols % 3 == 0, minus_one, one)
    sa = sb = None
    if lowp.SCALED[dtype]:
        blocks = k // lowp.BLOCK
        e = np.zeros((m, blocks), dtype=np.int64)
        if scaled_run:
            e = (np.arange(m * blocks).reshape(m, blocks) * 7) % 121 - 60
        sa, sb = lowp.e8m0_encode(e), lowp.e8m0_encode(np.zeros((n, blocks), dtype=np.int64))
    elif scaled_run:
        raise ValueError("fp8 takes no scales")
    return _finish(dtype, "encodings-scaled" if scaled_run else "encodings", ENCODING_SHAPE,
                   _codes(dtype, a), _codes(dtype, bt), sa, sb)


@functools.lru_cache(maxsize=None)
def exact(dtype: str, shape: tuple) -> Operands:
    """Operands and reference of one dtype and shape: computed once, shared, read-only."""
    m, n, k = shape
    rng = np.random.default_rng([m, n, k, DTYPES.index(dtype)])
    if lowp.BITS[dtype] == 4:
        a, bt = rng.integers(0, 16, (m, k), dtype=np.uint8), rng.integers(0, 16, (n, k), dtype=np.uint8)
    else:
        a, bt = WINDOW_E4M3[rng.integers(0, len(WINDOW_E4M3), (m, k))], WINDOW_E4M3[rng.integers(0, len(WINDOW_E4M3), (n, k))]
    sa = sb = None
    if lowp.SCALED[dtype]:
        sa = lowp.e8m0_encode(rng.choice(SCALE_EXPONENTS, (m, k // lowp.BLOCK)))
        sb = lowp.e8m0_encode(rng.choice(SCALE_EXPONENTS, (n, k // lowp.BLOCK)))
    return _finish(dtype, "exact", shape, _codes(dtype, a), _codes(dtype, bt), sa, sb)


def abs_sum_max(o: Operands) -> float:
    """max over (m, n) of sum_k |a||b|: no partial sum of any element, in any order, exceeds it."""
    a = np.abs(lowp.decode_operand(o.dtype, o.a, o.scale_a))
    b = np.abs(lowp.decode_operand(o.dtype, o.bt, o.scale_bt))
    return float((a @ b.T).max())


def run(hip, o: Operands, poison_c: int = 1) -> np.ndarray:
    """The kernel's C for these operands; C is poisoned on the host (and with ``poison_c`` on the
    device), so a tile that is never written, or a copy-back that never happened, cannot pass."""
    m, n, k = o.shape
    c = gemm_cases.poisoned_c(m, n)
    hip.gemm_lowp(0, o.dtype, o.a.ctypes.data, o.bt.ctypes.data,
                  None if o.scale_a is None else o.scale_a.ctypes.data,
                  None if o.scale_bt is None else o.scale_bt.ctypes.data, c.ctypes.data, m, n, k,
                  poison_c=poison_c)
    return c
