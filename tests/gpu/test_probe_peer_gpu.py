"""The xGMI peer checks (``probe.peer``, ``probe.peer_ring``) with planted faults and an independent
reference, on a real MI355X (run with ``-m gpu``).

What arrived on the destination is compared byte for byte with the numpy twin of the pattern
(``gpupool.ops.hostlink``, seeded with the seed the report names); a bit flipped in the receiving
window between the copy and the verify is counted once and found at its offset, at the first and
the last chunk and spread over the window; a copy that is left out (``skipCopy``) fails every link
at offset 0 with exactly the bits in which this call's pattern differs from what the window still
held; and counters and windows are clean again afterwards. All comparisons are exact counts and
offsets. Sizes are the smallest that still split the fill / verify loops on a 256-CU part (the
entry points clamp to 1 MiB). One visible GPU runs every case as local copies (``peer(0, 0)``,
rings ``[0, 0]`` and ``[0, 0, 0]``); the cases over real links skip there.
"""
from __future__ import annotations

import numpy as np
import pytest

from gpupool.ops import hostlink

pytestmark = pytest.mark.gpu

MIB = 1 << 20
SIZES = [
    MIB,             # 65536 chunks = 256 workgroups of work: the tail loops only
    MIB + 16 * 77,   # a ragged tail
    4 * MIB + 16,    # the fill's unrolled main loop once on 256 CUs, plus one tail chunk
    4 * MIB + 8,     # no multiple of 16: "bytes" is rounded down, the last 8 bytes are not tested
]
PAIRS = ["local", "xgmi"]
RINGS = ["local2", "local3", "xgmi"]
_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint64)


@pytest.fixture(scope="module")
def hip(native_built):
    from gpupool.ops import probe
    n = probe.init()
    assert n >= 1, "no HIP device visible"
    return probe


def _pair(hip, kind):
    if kind == "local":
        return 0, 0
    if hip.init() < 2:
        pytest.skip("one GPU visible")
    return 0, 1


def _ring(hip, kind):
    if kind == "local2":
        return [0, 0]
    if kind == "local3":
        return [0, 0, 0]
    if hip.init() < 2:
        pytest.skip("one GPU visible")
    return list(range(min(hip.init(), 4)))


def _hook_links(kind, ring):
    """The links the flip hooks are aimed at: every link of a local ring, the last of a real one."""
    return [len(ring) - 1] if kind == "xgmi" else list(range(len(ring)))


def first_flip_offset(nbytes: int, k: int) -> int:
    """Byte offset of the lowest chunk ``injectBitFlips=k`` corrupts (the formula of
    test_probe_hbm_edges_gpu.py): one bit in each of the words stride, 2 * stride, .. k * stride,
    stride = words // (k + 1)."""
    n16 = nbytes // 16
    return 16 * ((n16 * 4 // (k + 1)) // 4)


def differing_bits(n16: int, seed_a: int, seed_b: int) -> int:
    """In how many bits the patterns of two seeds differ over chunks [0, n16), by the twin."""
    x = hostlink.pattern_words(0, n16, seed_a) ^ hostlink.pattern_words(0, n16, seed_b)
    return int(_POP8[np.ascontiguousarray(x).view(np.uint8)].sum())


def _assert_clean_link(link, nbytes):
    assert link["passed"] is True and link["canAccessPeer"] is True, link
    assert link["badBits"] == 0 and link["firstBadOffset"] is None, link
    assert link["bytes"] == nbytes // 16 * 16, link


def _assert_clean_ring(r, ring, nbytes):
    assert r["passed"] is True and r["bytes"] == nbytes // 16 * 16 and len(r["links"]) == len(ring), r
    for i, link in enumerate(r["links"]):
        assert (link["src"], link["dst"]) == (ring[i], ring[(i + 1) % len(ring)]), link
        _assert_clean_link(link, nbytes)


def _struck(ring, j):
    """The links that see a flip planted ahead of link j's verify: link j, and every link verified
    after it on the same receive window (a repeated device; none when the devices are distinct)."""
    dst = [ring[(i + 1) % len(ring)] for i in range(len(ring))]
    return {i for i in range(j, len(ring)) if dst[i] == dst[j]}


# ---------------------------------------------------------------- the pair check
@pytest.mark.parametrize("nbytes", SIZES)
@pytest.mark.parametrize("kind", PAIRS)
def test_pair_arrived_bytes_equal_the_twin(hip, kind, nbytes):
    src, dst = _pair(hip, kind)
    n16 = nbytes // 16
    seeds = []
    for _ in range(2):
        r = hip.peer(src, dst, nbytes, want_bytes=nbytes)
        assert (r["src"], r["dst"]) == (src, dst), r
        _assert_clean_link(r, nbytes)
        assert len(r["data"]) == n16 * 16, (len(r["data"]), n16)
        got = np.frombuffer(r["data"], dtype=np.uint8)
        ref = hostlink.pattern_bytes(0, n16, r["seed"])
        bad = np.flatnonzero(got != ref)
        assert bad.size == 0, (bad.size, int(bad[0]), r)
        seeds.append(r["seed"])
    assert seeds[0] != seeds[1], seeds  # a call's verify is not satisfiable by an earlier call's data
    # a shorter image: only that much comes back
    r = hip.peer(src, dst, nbytes, want_bytes=48)
    assert r["data"] == hostlink.pattern_bytes(0, 3, r["seed"]).tobytes(), r


@pytest.mark.parametrize("nbytes", SIZES)
@pytest.mark.parametrize("kind", PAIRS)
def test_pair_flip_at_first_and_last_chunk_is_found_there(hip, kind, nbytes):
    src, dst = _pair(hip, kind)
    n16 = nbytes // 16
    for chunk in (0, n16 - 1):
        r = hip.peer(src, dst, nbytes, want_bytes=nbytes, injectFlipAtChunk=chunk)
        assert r["passed"] is False and r["canAccessPeer"] is True, r
        assert r["badBits"] == 1 and r["firstBadOffset"] == 16 * chunk, (chunk, r)
        # what the destination held: the twin, but for bit 0 of that chunk's first byte
        diff = np.frombuffer(r["data"], dtype=np.uint8) ^ hostlink.pattern_bytes(0, n16, r["seed"])
        at = np.flatnonzero(diff)
        assert at.tolist() == [16 * chunk] and int(diff[16 * chunk]) == 1, (chunk, at[:8], r)
    _assert_clean_link(hip.peer(src, dst, nbytes, injectFlipAtChunk=n16), nbytes)  # past the end: no flip


@pytest.mark.parametrize("nbytes", SIZES)
@pytest.mark.parametrize("kind", PAIRS)
def test_pair_spread_flips_counted_and_first_located(hip, kind, nbytes):
    src, dst = _pair(hip, kind)
    for k in (1, 6, 37):
        r = hip.peer(src, dst, nbytes, injectBitFlips=k, injectLink=5)  # a pair check ignores injectLink
        assert r["passed"] is False, r
        assert r["badBits"] == k and r["firstBadOffset"] == first_flip_offset(nbytes, k), (k, r)
    _assert_clean_link(hip.peer(src, dst, nbytes), nbytes)


@pytest.mark.parametrize("nbytes", SIZES)
@pytest.mark.parametrize("kind", PAIRS)
def test_pair_without_its_copy_fails(hip, kind, nbytes):
    """The destination is a fresh allocation of the size the clean call just freed: whatever it
    holds, the last call's pattern included, must not verify as this call's."""
    src, dst = _pair(hip, kind)
    _assert_clean_link(hip.peer(src, dst, nbytes), nbytes)
    r = hip.peer(src, dst, nbytes, skipCopy=1)
    assert r["passed"] is False and r["canAccessPeer"] is True, r
    assert r["badBits"] > 0 and r["firstBadOffset"] == 0, r
    assert r["bytes"] == nbytes // 16 * 16, r
    _assert_clean_link(hip.peer(src, dst, nbytes), nbytes)


# ---------------------------------------------------------------- the ring
@pytest.mark.parametrize("nbytes", SIZES)
@pytest.mark.parametrize("kind", RINGS)
def test_ring_clean_and_seeded_per_source_and_call(hip, kind, nbytes):
    ring = _ring(hip, kind)
    a = hip.peer_ring(ring, nbytes)
    b = hip.peer_ring(ring, nbytes)
    for r in (a, b):
        _assert_clean_ring(r, ring, nbytes)
        by_src = {}
        for link in r["links"]:
            assert by_src.setdefault(link["src"], link["seed"]) == link["seed"], r  # one pattern per source
        assert len(set(by_src.values())) == len(by_src), r  # and no two sources share one
    for la, lb in zip(a["links"], b["links"]):
        assert la["seed"] != lb["seed"], (la, lb)


@pytest.mark.parametrize("nbytes", SIZES)
@pytest.mark.parametrize("kind", RINGS)
def test_ring_flip_at_first_and_last_chunk_is_found_on_its_link(hip, kind, nbytes):
    ring = _ring(hip, kind)
    n16 = nbytes // 16
    for j in _hook_links(kind, ring):
        for chunk in (0, n16 - 1):
            r = hip.peer_ring(ring, nbytes, injectFlipAtChunk=chunk, injectLink=j)
            assert r["passed"] is False and len(r["links"]) == len(ring), r
            for i, link in enumerate(r["links"]):
                if i in _struck(ring, j):
                    assert link["passed"] is False and link["badBits"] == 1, (j, chunk, i, r)
                    assert link["firstBadOffset"] == 16 * chunk, (j, chunk, i, r)
                else:  # every other link stays clean
                    _assert_clean_link(link, nbytes)
        _assert_clean_ring(hip.peer_ring(ring, nbytes, injectFlipAtChunk=n16, injectLink=j), ring, nbytes)
    if kind == "xgmi":  # distinct devices: the fault of one link is that link's alone
        assert _struck(ring, len(ring) - 1) == {len(ring) - 1}


@pytest.mark.parametrize("nbytes", SIZES)
@pytest.mark.parametrize("kind", RINGS)
def test_ring_spread_flips_counted_and_first_located(hip, kind, nbytes):
    ring = _ring(hip, kind)
    for j in _hook_links(kind, ring):
        for k in (1, 6, 37):
            r = hip.peer_ring(ring, nbytes, injectBitFlips=k, injectLink=j)
            assert r["passed"] is False, r
            for i, link in enumerate(r["links"]):
                if i in _struck(ring, j):
                    assert link["passed"] is False and link["badBits"] == k, (j, k, i, r)
                    assert link["firstBadOffset"] == first_flip_offset(nbytes, k), (j, k, i, r)
                else:
                    _assert_clean_link(link, nbytes)
    # a link the ring does not have: no flip
    _assert_clean_ring(hip.peer_ring(ring, nbytes, injectBitFlips=6, injectLink=len(ring)), ring, nbytes)
    _assert_clean_ring(hip.peer_ring(ring, nbytes), ring, nbytes)


@pytest.mark.parametrize("nbytes", SIZES)
@pytest.mark.parametrize("kind", RINGS)
def test_ring_without_its_copies_fails_with_exact_counts(hip, kind, nbytes):
    """The receive windows are kept between rings of one size, so after a clean ring each still
    holds that ring's pattern. A ring whose copies are left out verifies this call's pattern
    against it: every link fails from chunk 0 on, in exactly the bits in which the two patterns
    differ — the twin computes them from the two reported seeds. A link that goes dead after its
    first good check looks like this."""
    ring = _ring(hip, kind)
    n16 = nbytes // 16
    clean = hip.peer_ring(ring, nbytes)
    _assert_clean_ring(clean, ring, nbytes)
    held = {}  # receiving device -> the seed of the last pattern copied into its window
    for link in clean["links"]:
        held[link["dst"]] = link["seed"]
    r = hip.peer_ring(ring, nbytes, skipCopy=1)
    assert r["passed"] is False and r["bytes"] == n16 * 16 and len(r["links"]) == len(ring), r
    for link in r["links"]:
        assert link["passed"] is False and link["canAccessPeer"] is True, r
        assert link["seed"] != held[link["dst"]], (link, held)
        assert link["firstBadOffset"] == 0, r
        assert link["badBits"] == differing_bits(n16, held[link["dst"]], link["seed"]), (link, held)
    _assert_clean_ring(hip.peer_ring(ring, nbytes), ring, nbytes)


@pytest.mark.parametrize("kind", RINGS)
def test_counters_are_left_clean_after_a_faulty_ring(hip, kind):
    """The ring's device counters are kept between calls and the pinned result slots are the claim
    probe's: a clean ring and a clean claim probe right after a faulty ring report nothing, and a
    clean ring right after a faulty claim probe neither."""
    ring = _ring(hip, kind)
    small = dict(hbm_bytes=MIB, gemm_n=256)
    last = len(ring) - 1
    bad = hip.peer_ring(ring, MIB, injectBitFlips=5, injectLink=last)
    assert bad["passed"] is False and bad["links"][last]["badBits"] == 5, bad
    _assert_clean_ring(hip.peer_ring(ring, MIB), ring, MIB)
    bad = hip.peer_ring(ring, MIB, injectFlipAtChunk=3, injectLink=last)
    assert bad["passed"] is False and bad["links"][last]["firstBadOffset"] == 48, bad
    for dev in sorted(set(ring)):
        p = hip.run(dev, **small)
        assert p["passed"] is True, p
        assert p["hbm"]["badBits"] == 0 and p["hbm"]["firstBadOffset"] is None, p["hbm"]
        assert p["mfma"]["abftMismatches"] == 0 and p["mfma"]["elementMismatches"] == 0, p["mfma"]
    p = hip.run(ring[0], injectBitFlips=7, **small)
    assert p["passed"] is False and p["hbm"]["badBits"] == 7, p
    _assert_clean_ring(hip.peer_ring(ring, MIB), ring, MIB)
    src, dst = ring[0], ring[1]
    bad = hip.peer(src, dst, MIB, injectBitFlips=3)
    assert bad["badBits"] == 3, bad
    _assert_clean_link(hip.peer(src, dst, MIB), MIB)
    _assert_clean_ring(hip.peer_ring(ring, MIB), ring, MIB)


@pytest.mark.parametrize("kind", RINGS)
def test_ring_windows_allocated_again_after_a_trim(hip, kind):
    ring = _ring(hip, kind)
    _assert_clean_ring(hip.peer_ring(ring, MIB), ring, MIB)
    hip.trim(0)  # frees the ring windows; the next ring allocates them again
    r = hip.peer_ring(ring, MIB, skipCopy=1)
    assert r["passed"] is False, r
    for link in r["links"]:
        assert link["passed"] is False and link["badBits"] > 0 and link["firstBadOffset"] is not None, r
    _assert_clean_ring(hip.peer_ring(ring, MIB), ring, MIB)
    hip.trim(0)
    _assert_clean_ring(hip.peer_ring(ring, MIB), ring, MIB)
