"""numpy reference of what the probe's LDS phase (native/src/probe/lds.h) holds in a CU's Local Data
Share, for tests and scripts that check the images ``probe.lds(..., want_stage=...)`` returns.

Workgroup ``b`` writes 16-byte chunk ``j`` as the HBM test's ``pattern16<1>`` of index
``(b << 32) | j`` (``hostlink.pattern_words``), so no two workgroups and no two chunks share a value;
the address pass gives dword ``d`` the first word of ``pattern16<1>((b << 32) | d, seed + 1)``, written
in the order ``d = (i * stride(N)) % N``.
"""
from __future__ import annotations

import math

import numpy as np

from . import hostlink

SEED_BASE = 0x4C445300  # the phase's seed is (SEED_BASE + HIP device ordinal) ^ salt
BYTES_PER_CU = 163840
CHUNK = 16


def march_bytes(workgroup: int, chunks: int, seed: int, flip: int = 0) -> np.ndarray:
    """uint8 [chunks * 16]: the LDS of ``workgroup`` after a march write of polarity ``flip``
    (0, or 0xFFFFFFFF for the complement)."""
    return hostlink.pattern_bytes(int(workgroup) << 32, chunks, seed, flip)


def address_words(workgroup: int, dwords: int, seed: int) -> np.ndarray:
    """uint32 [dwords]: the LDS of ``workgroup`` after the address pass (``seed`` is the march's; the
    pass uses seed + 1)."""
    return hostlink.pattern_words(int(workgroup) << 32, dwords, (seed + 1) & 0xFFFFFFFF)[:, 0].copy()


def stride(dwords: int) -> int:
    """The address pass's stride: the smallest odd value >= 33 coprime to ``dwords``."""
    s = 33
    while math.gcd(s, dwords) != 1:
        s += 2
    return s
