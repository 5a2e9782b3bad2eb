"""The numpy twin (gpupool/ops/lds.py) of what the probe's LDS phase holds in a CU's LDS: known
answers computed by the host-compiled ``pattern16<1>`` at the indices the kernel uses, no value shared
between two workgroups over the whole 160 KiB, the complementary polarity, distinct address-pass
dwords, and the stride of the address pass."""
from __future__ import annotations

import math

import numpy as np

from gpupool.ops import hostlink, lds

SEED = lds.SEED_BASE
CHUNKS = lds.BYTES_PER_CU // 16


def _hex(words) -> str:
    return " ".join(f"{int(w):08x}" for w in words)


def _chunk(b: np.ndarray, j: int) -> str:
    return _hex(b[16 * j:16 * j + 16].view("<u4"))


def test_known_answers():
    assert lds.SEED_BASE == 0x4C445300 and lds.BYTES_PER_CU == 163840 == 16 * CHUNKS
    # workgroup 3, chunk 5: pattern16<1>((3 << 32) | 5, seed, 0)
    assert _chunk(lds.march_bytes(3, 8, SEED, 0), 5) == "f28c27ee 29824b57 1b78311a b4fd7c7d"
    # the last workgroup of the largest grid's first 2048, the last chunk, device 7, salted, complemented
    assert _chunk(lds.march_bytes(2047, CHUNKS, (SEED + 7) ^ 0x5A17, 0xFFFFFFFF), CHUNKS - 1) == \
        "7351731f f4d6bad6 4f89b0c7 457ca129"
    # the address pass: dword d holds the FIRST word of pattern16<1>((b << 32) | d, seed + 1, 0)
    assert f"{int(lds.address_words(3, 8, SEED)[7]):08x}" == "90c41d2c"
    assert f"{int(lds.address_words(0, 4 * CHUNKS, SEED ^ 0x5A17)[-1]):08x}" == "2460cc76"


def test_march_bytes_is_the_shared_pattern_at_the_workgroups_index():
    a = lds.march_bytes(9, 300, SEED, 0)
    assert a.dtype == np.uint8 and a.shape == (4800,)
    assert np.array_equal(a, hostlink.pattern_bytes((9 << 32), 300, SEED, 0))
    w = lds.address_words(9, 1200, SEED)
    assert w.dtype == np.uint32 and w.shape == (1200,)
    assert np.array_equal(w, hostlink.pattern_words(9 << 32, 1200, SEED + 1, 0)[:, 0])


def test_two_workgroups_never_share_a_chunk_value_over_160_kib():
    """At the same LDS address: what another workgroup left in a chunk is never what this one expects
    there (the workgroup enters the mix by XOR, so equal indices differ exactly when the workgroups
    do), and inside a workgroup every chunk is distinct (an aliased address reads another value)."""
    ids = (0, 1, 2, 255, 2047, 4095, 16383)
    w = {b: lds.march_bytes(b, CHUNKS, SEED, 0).view("<u4").reshape(CHUNKS, 4) for b in ids}
    for b in ids:
        assert len(np.unique(w[b], axis=0)) == CHUNKS
        assert len(np.unique(w[b][:, 0])) == CHUNKS  # already in the first word
        for c in ids:
            if c > b:
                assert not np.any(np.all(w[b] == w[c], axis=1)), (b, c)
    # the same workgroup under the next run's salt: what a CU still holds is never what is expected
    nxt = lds.march_bytes(0, CHUNKS, SEED ^ 1, 0).view("<u4").reshape(CHUNKS, 4)
    assert not np.any(np.all(nxt == w[0], axis=1))


def test_polarity_1_is_the_bitwise_complement():
    a = lds.march_bytes(5, CHUNKS, SEED, 0)
    b = lds.march_bytes(5, CHUNKS, SEED, 0xFFFFFFFF)
    assert np.array_equal(a ^ b, np.full_like(a, 0xFF))
    assert 0.45 < np.unpackbits(a).mean() < 0.55  # both bit values dense


def test_address_words_are_distinct_over_40960_dwords():
    w = lds.address_words(0, 4 * CHUNKS, SEED)
    assert w.size == 40960 and len(np.unique(w)) == w.size
    other = lds.address_words(1, 4 * CHUNKS, SEED)
    assert not np.any(other == w)  # nor what the workgroup before left at the same dword


def test_stride():
    for n in (4, 400, 660, 1028, 16388, 40956, 40960):
        s = lds.stride(n)
        assert s >= 33 and s % 2 == 1 and math.gcd(s, n) == 1
        assert all(math.gcd(c, n) > 1 for c in range(33, s, 2))  # the smallest such
        assert np.array_equal(np.sort(np.arange(n, dtype=np.int64) * s % n), np.arange(n))
    assert lds.stride(660) == 37 and lds.stride(40960) == 33
