"""The numpy twin (gpupool/ops/hostlink.py) of the probe's kPat 1 chunk pattern, which the host-link
phase writes into pinned host memory: known answers computed by the host-compiled ``pattern16<1>``,
distinctness and the complementary polarity."""
from __future__ import annotations

import numpy as np

from gpupool.ops import hostlink


def _hex(words) -> str:
    return " ".join(f"{int(w):08x}" for w in words)


def test_known_answers():
    assert _hex(hostlink.pattern_words(5, 1, 0x4C4B0000, 0)[0]) == "49f0f395 555630ec cf038a66 cf4600a9"
    # an index past 2^32 (the high half enters the mix), a device seed, the complementary polarity
    assert _hex(hostlink.pattern_words(2**32 + 7, 1, 0x4C4B0003, 0xFFFFFFFF)[0]) == \
        "54464eca e3eb6ff1 725c97d0 905bb614"
    assert hostlink.SEED_BASE == 0x4C4B0000


def test_bytes_are_the_little_endian_words():
    b = hostlink.pattern_bytes(5, 2, 0x4C4B0000, 0)
    assert b.dtype == np.uint8 and b.shape == (32,)
    assert bytes(b[:8]).hex() == "95f3f049" "ec305655"
    assert np.array_equal(b[16:], hostlink.pattern_bytes(6, 1, 0x4C4B0000, 0))  # a range is its chunks


def test_chunks_are_pairwise_distinct_over_1_mib():
    w = hostlink.pattern_words(0, (1 << 20) // 16, 0x4C4B0000, 0)
    assert len(np.unique(w, axis=0)) == len(w)
    assert len(np.unique(w[:, 0])) == len(w)  # already in the first word: the mix is a bijection
    far = hostlink.pattern_words(2**32, (1 << 20) // 16, 0x4C4B0000, 0)  # the same low halves
    assert not np.any(np.all(far == w, axis=1))


def test_polarity_1_is_the_bitwise_complement():
    a = hostlink.pattern_bytes(123, 4096, 0x4C4B0001, 0)
    b = hostlink.pattern_bytes(123, 4096, 0x4C4B0001, 0xFFFFFFFF)
    assert np.array_equal(a ^ b, np.full_like(a, 0xFF))
    ones = np.unpackbits(a).mean()
    assert 0.45 < ones < 0.55  # both bit values dense
