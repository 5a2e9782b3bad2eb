"""numpy reference of what the probe's register-file phase (native/src/probe/regfile.h) holds in the
vector registers of one workgroup, for tests and scripts that check the images
``probe.regs(..., want_stage=...)`` returns.

Registers are numbered ``u`` = 0..511: ``v0..v255`` are 0..255, ``a0..a255`` are 256..511. Register
``u`` of lane ``l`` of wave ``w`` of workgroup ``b`` holds ``(base + u * MULTIPLIER) ^ flip`` with
``base`` the first word of the HBM test's ``pattern16<1>`` of index ``(b << 32) | (64 w + l)``
(``hostlink.pattern_words``): the multiplier is odd, so no two registers of a lane share a value,
and the base differs per lane, wave, workgroup and seed.
"""
from __future__ import annotations

import numpy as np

from . import hostlink

SEED_BASE = 0x52454700  # the phase's seed is (SEED_BASE + HIP device ordinal) ^ salt
MULTIPLIER = 0x9E3779B1
REGISTERS = 512  # per lane: v0..v255, a0..a255
LANES = 64
WAVES = 4  # of a workgroup, one per SIMD
IMAGE_BYTES = WAVES * REGISTERS * LANES * 4


def base_words(workgroup: int, seed: int) -> np.ndarray:
    """uint32 [4][64]: the per-lane base of every wave of ``workgroup``."""
    return hostlink.pattern_words(int(workgroup) << 32, WAVES * LANES, seed)[:, 0].reshape(WAVES, LANES).copy()


def expected(workgroup: int, seed: int, flip: int = 0) -> np.ndarray:
    """uint32 [4][512][64] (wave, register, lane): the registers of ``workgroup`` after a march write
    of polarity ``flip`` (0, or 0xFFFFFFFF for the complement)."""
    base = base_words(workgroup, seed).astype(np.uint64)[:, None, :]
    u = np.arange(REGISTERS, dtype=np.uint64)[None, :, None]
    e = (base + u * np.uint64(MULTIPLIER)) & np.uint64(0xFFFFFFFF)
    return (e ^ np.uint64(flip & 0xFFFFFFFF)).astype(np.uint32)


def register_name(u: int) -> str:
    """``v17`` / ``a3`` for the unified index ``u``."""
    return f"v{u}" if u < 256 else f"a{u - 256}"
