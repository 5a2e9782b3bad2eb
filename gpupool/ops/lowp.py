"""The low-precision number formats of the probe's FP8 / MX matrix-core checks, on the host.

numpy only (no torch, no GPU): the tests, the measuring scripts and the simulated probe share it.

``fp8``    OCP e4m3fn bytes on the unscaled MFMA.
``mxfp8``  e4m3 bytes, one E8M0 scale byte per 32 K-elements.
``mxfp4``  e2m1 nibbles, two per byte with the even k in the low nibble, E8M0 scales as above.

e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits; no infinities, S.1111.111 is NaN, the largest
finite value is 448 and the subnormals are multiples of 2^-9. e2m1: 1 sign, 2 exponent (bias 1),
1 mantissa bit: 0, 0.5, 1, 1.5, 2, 3, 4, 6. E8M0: 2^(b - 127), 255 is NaN.
"""
from __future__ import annotations

import numpy as np

DTYPES = ("fp8", "mxfp8", "mxfp4")      # the order is the C ABI's dtype index and mask bit
SCALED = {"fp8": False, "mxfp8": True, "mxfp4": True}
BITS = {"fp8": 8, "mxfp8": 8, "mxfp4": 4}
BLOCK = 32                              # K-elements per E8M0 scale


def dtype_index(name: str) -> int:
    if name not in DTYPES:
        raise ValueError(f"unknown low-precision dtype {name!r}: one of {DTYPES}")
    return DTYPES.index(name)


def dtype_mask(names) -> int:
    """Names -> the bit mask of the probe option "mfmaLowPrecision". Duplicates are refused."""
    names = list(names)
    if len(set(names)) != len(names):
        raise ValueError(f"duplicate low-precision dtype in {names}")
    mask = 0
    for n in names:
        mask |= 1 << dtype_index(n)
    return mask


def mask_names(mask: int) -> list[str]:
    return [n for i, n in enumerate(DTYPES) if mask >> i & 1]


def _e4m3_table() -> np.ndarray:
    b = np.arange(256)
    e, m = (b >> 3) & 15, b & 7
    mag = np.where(e == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (e.astype(np.float64) - 10))
    mag[(e == 15) & (m == 7)] = np.nan
    return np.where(b & 0x80, -mag, mag).astype(np.float32)


E4M3 = _e4m3_table()                    # byte -> float32
E4M3.setflags(write=False)
E2M1 = np.array([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6], dtype=np.float32)
E2M1.setflags(write=False)


def e4m3_decode(b: np.ndarray) -> np.ndarray:
    return E4M3[np.asarray(b, dtype=np.uint8)]


def e2m1_decode(nibbles: np.ndarray) -> np.ndarray:
    return E2M1[np.asarray(nibbles, dtype=np.uint8) & 15]


def _encode(x: np.ndarray, mags: np.ndarray, sign_bit: int) -> np.ndarray:
    """Round to nearest, ties to the even code, saturating; ``mags`` are the magnitudes of codes
    0 .. len-1 in increasing order."""
    x = np.asarray(x, dtype=np.float64)
    if not np.isfinite(x).all():
        raise ValueError("only finite values encode")
    mag = np.abs(x)
    hi = np.clip(np.searchsorted(mags, mag), 1, len(mags) - 1)
    lo = hi - 1
    dlo, dhi = mag - mags[lo], mags[hi] - mag
    code = np.where((dlo < dhi) | ((dlo == dhi) & (lo % 2 == 0)), lo, hi)
    return (code | np.where(np.signbit(x), sign_bit, 0)).astype(np.uint8)


def e4m3_encode(x: np.ndarray) -> np.ndarray:
    return _encode(x, E4M3[:0x7F].astype(np.float64), 0x80)


def e2m1_encode(x: np.ndarray) -> np.ndarray:
    return _encode(x, E2M1[:8].astype(np.float64), 8)


def e8m0_decode(b: np.ndarray) -> np.ndarray:
    """E8M0 bytes -> float64 powers of two (255 -> NaN)."""
    b = np.asarray(b, dtype=np.uint8)
    return np.where(b == 255, np.nan, np.ldexp(1.0, b.astype(np.int32) - 127))


def e8m0_encode(exponent: np.ndarray) -> np.ndarray:
    """Integer exponents e in [-127, 127] -> the E8M0 byte of 2^e."""
    e = np.asarray(exponent, dtype=np.int64)
    if ((e < -127) | (e > 127)).any():
        raise ValueError("E8M0 holds 2^-127 .. 2^127")
    return (e + 127).astype(np.uint8)


def pack_fp4(nibbles: np.ndarray) -> np.ndarray:
    """[..., k] e2m1 codes -> [..., k/2] bytes, element 2i in the low nibble of byte i."""
    n = np.asarray(nibbles, dtype=np.uint8)
    if n.shape[-1] % 2:
        raise ValueError("an even number of elements packs into bytes")
    return np.ascontiguousarray((n[..., 0::2] & 15) | ((n[..., 1::2] & 15) << 4))


def unpack_fp4(packed: np.ndarray) -> np.ndarray:
    p = np.asarray(packed, dtype=np.uint8)
    out = np.empty(p.shape[:-1] + (p.shape[-1] * 2,), dtype=np.uint8)
    out[..., 0::2] = p & 15
    out[..., 1::2] = p >> 4
    return out


def decode_operand(dtype: str, data: np.ndarray, scales: np.ndarray | None = None) -> np.ndarray:
    """An operand as the GEMM entry point takes it ([rows][k] e4m3 bytes, or [rows][k/2] packed
    e2m1; ``scales`` [rows][k/32] E8M0 for the scaled dtypes) -> float64 [rows][k]."""
    dtype_index(dtype)
    if SCALED[dtype] != (scales is not None):
        raise ValueError(f"{dtype}: scales are {'needed' if SCALED[dtype] else 'not taken'}")
    v = (e2m1_decode(unpack_fp4(data)) if BITS[dtype] == 4 else e4m3_decode(data)).astype(np.float64)
    if scales is not None:
        v = v * np.repeat(e8m0_decode(scales), BLOCK, axis=-1)
    return v


def reference(dtype: str, a, bt, scale_a=None, scale_bt=None) -> np.ndarray:
    """float64 A @ Bt^T of the decoded, scaled operands."""
    return decode_operand(dtype, a, scale_a) @ decode_operand(dtype, bt, scale_bt).T
