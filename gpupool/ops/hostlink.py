"""numpy reference of the probe's address-dependent pattern (``pattern16<1>`` in probe.hip), as the
host-link phase (native/src/probe/hostlink.h) writes it into pinned host memory: for tests and
scripts that check what ``probe.host_link`` returns or preload a buffer for it.

One 16-byte chunk ``i`` holds four little-endian 32-bit words: a bijective mix ``h`` of the chunk
index and the seed, then byte rotations of ``h`` XOR fixed masks, every word XOR ``flip`` (0, or
0xFFFFFFFF on the complementary passes).
"""
from __future__ import annotations

import numpy as np

SEED_BASE = 0x4C4B0000  # the phase's seed is SEED_BASE + HIP device ordinal
CHUNK = 16
_MASKS = (0x00000000, 0xA5A5A5A5, 0x3C96C396, 0x5A0FF05A)


def _rotl(x: np.ndarray, r: int) -> np.ndarray:
    x = x.astype(np.uint64) & 0xFFFFFFFF
    return ((x << np.uint64(r)) | (x >> np.uint64(32 - r))) & np.uint64(0xFFFFFFFF) if r else x


def pattern_words(first_chunk: int, chunks: int, seed: int, flip: int = 0) -> np.ndarray:
    """uint32 [chunks, 4]: the words of chunks first_chunk .. first_chunk + chunks - 1."""
    i = np.uint64(first_chunk) + np.arange(chunks, dtype=np.uint64)
    lo, hi = i & np.uint64(0xFFFFFFFF), i >> np.uint64(32)
    h = ((lo ^ np.uint64(seed & 0xFFFFFFFF)) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    h ^= _rotl(hi, 7)
    h ^= h >> np.uint64(15)
    out = np.empty((chunks, 4), dtype=np.uint32)
    for w, (rot, mask) in enumerate(zip((0, 8, 16, 24), _MASKS)):
        out[:, w] = (_rotl(h, rot) ^ np.uint64(mask) ^ np.uint64(flip & 0xFFFFFFFF)).astype(np.uint32)
    return out


def pattern_bytes(first_chunk: int, chunks: int, seed: int, flip: int = 0) -> np.ndarray:
    """uint8 [chunks * 16]: the same as the bytes the GPU stores (little-endian words)."""
    return pattern_words(first_chunk, chunks, seed, flip).astype("<u4").reshape(-1).view(np.uint8)
