"""The probe's PCIe host-link phase on a real MI355X (run with ``-m gpu``).

The GPU writes the address-dependent pattern into pinned host memory over the link, reads it back
and verifies every bit; the tests compare what landed in host memory byte for byte with the numpy
twin of the pattern (``gpupool.ops.hostlink``), let the GPU verify buffers the host made (clean,
one flipped bit at either end, 37 spread flips), and flip a bit from the host between a write and
its verify. Sizes sit where the kernels' loops can go wrong: one partial workgroup, exactly one
main-loop pass of the whole grid plus one tail chunk (from the geometry the library exports), a
large size with a ragged tail, and a size that is no multiple of 16. Every size runs after a larger
run has left the other polarity in the buffer, so a chunk the kernel never wrote cannot pass.
The bandwidth case asserts only the ceiling: above the link's 63 GB/s the traffic did not cross it.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from gpupool.agent.prober import Prober
from gpupool.ops import hostlink

pytestmark = pytest.mark.gpu

MIB = 1 << 20
SEED = hostlink.SEED_BASE  # + device ordinal 0
BIG = 64 * MIB + 16 * 4096  # larger than every tested size: leaves foreign data behind them all
PROBE = dict(hbm_bytes=64 * MIB, gemm_n=512)
DEFAULT_KEYS = {"device", "hipUUID", "gcnArch", "passed", "hbm", "mfma", "cus", "ms", "phases", "reportMs"}
PHASE_KEYS = {"arenaReused", "setupMs", "allocMs", "launchMs", "hbmFirst", "hbmWallMs", "mfmaWallMs", "freeMs"}
BLOCK_KEYS = {"ok", "bytes", "patterns", "seed", "badBits", "firstBadOffset", "hostSamples",
              "hostSampleMismatches", "writeGBps", "readGBps", "GBps", "ms", "allocMs"}
SIZES = ("partial_workgroup", "one_grid_pass_plus_one", "large_ragged", "not_multiple_of_16")


@pytest.fixture(scope="module")
def hip(native_built):
    from gpupool.ops import probe
    n = probe.init()
    assert n >= 1, "no HIP device visible"
    return probe


def _size(hip, name: str) -> int:
    g = hip.host_link_geometry()
    return {"partial_workgroup": 16 * 100,
            "one_grid_pass_plus_one": 16 * (g["grid"] * g["threads"] * g["unroll"] + 1),
            "large_ragged": 64 * MIB + 16 * 77,
            "not_multiple_of_16": 64 * MIB + 8}[name]


@functools.lru_cache(maxsize=None)
def _ref(chunks: int, flip: int) -> np.ndarray:
    """The reference bytes of chunks [0, chunks), computed once per size and polarity, read-only."""
    a = hostlink.pattern_bytes(0, chunks, SEED, flip)
    a.setflags(write=False)
    return a


def _clean(r, nbytes):
    assert set(r) == BLOCK_KEYS | {"device", "passed"} or set(r) == BLOCK_KEYS | {"device", "passed", "data"}, sorted(r)
    assert r["passed"] and r["ok"], r
    assert r["bytes"] == nbytes // 16 * 16 and r["seed"] == SEED
    assert r["badBits"] == 0 and r["firstBadOffset"] is None and r["hostSampleMismatches"] == 0, r
    assert r["hostSamples"] == min(nbytes // 16, 1026)


def _dirty(hip, patterns):
    """A larger run that leaves polarity (patterns - 1) & 1 over everything a test then touches."""
    assert hip.host_link(0, BIG, patterns=patterns)["passed"]


@pytest.mark.parametrize("name", SIZES)
def test_written_bytes_match_the_reference(hip, name):
    nbytes = _size(hip, name)
    chunks = nbytes // 16
    _dirty(hip, 2)  # leaves polarity 1; one pass must leave polarity 0 in every tested chunk
    r = hip.host_link(0, nbytes, patterns=1, want_bytes=nbytes)
    data = r.pop("data")
    _clean(r, nbytes)
    assert r["patterns"] == 1 and len(data) == chunks * 16
    got = np.frombuffer(data, dtype=np.uint8)
    diff = np.flatnonzero(got != _ref(chunks, 0))
    assert diff.size == 0, f"{diff.size} bytes differ, first at {diff[0]}"
    # now polarity 0 is behind it: two passes must leave polarity 1
    r = hip.host_link(0, nbytes, want_bytes=nbytes)
    data = r.pop("data")
    _clean(r, nbytes)
    assert r["patterns"] == 2
    diff = np.flatnonzero(np.frombuffer(data, dtype=np.uint8) != _ref(chunks, 0xFFFFFFFF))
    assert diff.size == 0, f"{diff.size} bytes differ, first at {diff[0]}"
    assert 0 < r["GBps"] == min(r["writeGBps"], r["readGBps"])


@pytest.mark.parametrize("name", SIZES)
def test_gpu_verifies_what_the_host_made(hip, name):
    nbytes = _size(hip, name)
    chunks = nbytes // 16
    _dirty(hip, 2)
    good = np.zeros(nbytes, dtype=np.uint8)  # a trailing partial chunk stays zero: it is not tested
    good[:chunks * 16] = _ref(chunks, 0)
    r = hip.host_link(0, 0, preload=good)
    assert r["passed"] and r["badBits"] == 0 and r["firstBadOffset"] is None, r
    assert r["bytes"] == chunks * 16 and r["patterns"] == 1 and r["hostSamples"] == 0
    assert r["writeGBps"] == 0 and r["GBps"] == r["readGBps"] > 0
    for chunk in (0, chunks - 1):
        bad = good.copy()
        bad[16 * chunk] ^= 1
        r = hip.host_link(0, 0, preload=bad)
        assert not r["passed"] and not r["ok"], r
        assert r["badBits"] == 1 and r["firstBadOffset"] == 16 * chunk, r
    # 37 single-bit flips spread over the buffer, in different words and bit positions
    rng = np.random.default_rng(37)
    where = np.sort(rng.choice(chunks, size=min(37, chunks), replace=False))
    assert where.size == 37
    bad = good.copy()
    for k, c in enumerate(where):
        bad[16 * int(c) + (k % 16)] ^= np.uint8(1 << (k % 8))
    r = hip.host_link(0, 0, preload=bad)
    assert not r["passed"] and r["badBits"] == 37 and r["firstBadOffset"] == 16 * int(where[0]), r


@pytest.mark.parametrize("name", SIZES)
def test_host_flip_between_write_and_verify_is_found(hip, name):
    nbytes = _size(hip, name)
    chunks = nbytes // 16
    for chunk in (0, chunks - 1):
        r = hip.run(0, host_link_bytes=nbytes, injectHostLinkFlipAtChunk=chunk, **PROBE)
        assert not r["passed"] and r["hbm"]["ok"] and r["mfma"]["ok"], r
        h = r["hostLink"]
        assert not h["ok"] and h["badBits"] == 1 and h["firstBadOffset"] == 16 * chunk, h
        assert "HostLinkMismatch: 1 flipped bit(s), first at offset %d" % (16 * chunk) in Prober.explain(r)["error"]
    r = hip.run(0, host_link_bytes=nbytes, injectHostLinkFlipAtChunk=chunks, **PROBE)  # past the end
    assert r["passed"] and r["hostLink"]["ok"] and r["hostLink"]["badBits"] == 0, r


def test_clean_run_at_default_hbm_and_mfma_settings(hip):
    r = hip.run(0, host_link_bytes=8 * MIB)
    assert r["passed"], r
    assert set(r) == DEFAULT_KEYS | {"hostLink"}
    assert r["hbm"]["ok"] and r["mfma"]["ok"] and r["cus"]["ok"]
    h = r["hostLink"]
    assert set(h) == BLOCK_KEYS
    assert h["ok"] and h["bytes"] == 8 * MIB and h["patterns"] == 2 and h["seed"] == SEED
    assert h["badBits"] == 0 and h["firstBadOffset"] is None
    assert h["hostSamples"] == 1026 and h["hostSampleMismatches"] == 0
    assert h["GBps"] == min(h["writeGBps"], h["readGBps"]) > 0


def test_phase_switched_off_reports_what_it_always_did(hip):
    hip.run(0, host_link_bytes=MIB, **PROBE)  # the buffer and the stream exist by now
    for r in (hip.run(0, **PROBE), hip.run(0, host_link_bytes=0, **PROBE), hip.run(0)):
        assert r["passed"] and set(r) == DEFAULT_KEYS, sorted(r)
        assert set(r["phases"]) == PHASE_KEYS, sorted(r["phases"])


def test_stale_pattern_of_another_size_never_verifies_as_the_new_one(hip):
    assert hip.run(0, host_link_bytes=8 * MIB, **PROBE)["passed"]       # leaves polarity 1 over 8 MiB
    r = hip.host_link(0, 4 * MIB + 16, patterns=1, want_bytes=4 * MIB + 16)  # polarity 0 over the front
    assert r["passed"] and r["hostSampleMismatches"] == 0
    assert np.array_equal(np.frombuffer(r["data"], dtype=np.uint8), _ref((4 * MIB + 16) // 16, 0))
    r = hip.run(0, host_link_bytes=8 * MIB, hostLinkPatterns=3, **PROBE)  # mixed polarities behind it
    assert r["passed"] and r["hostLink"]["patterns"] == 3 and r["hostLink"]["hostSampleMismatches"] == 0
    tail = hip.host_link(0, 8 * MIB, patterns=1, preload=_ref(8 * MIB // 16, 0))
    assert tail["passed"], tail  # the host's pattern, verified by the GPU over the whole 8 MiB
    stale = hip.host_link(0, 0, preload=_ref(8 * MIB // 16, 0xFFFFFFFF))  # the other polarity must not pass
    assert not stale["passed"] and stale["badBits"] == 8 * MIB * 8 and stale["firstBadOffset"] == 0


def test_rates_stay_under_the_links_ceiling(hip):
    """63 GB/s is the spec rate of PCIe Gen5 x16 per direction: a figure above 64 means the data
    came from a cache and never crossed the link. No lower bound here (the floor is the pool's)."""
    r = hip.run(0, overlap=0, host_link_bytes=64 * MIB, **PROBE)
    assert r["passed"], r
    h = r["hostLink"]
    print(f"host link 64 MiB alone: write {h['writeGBps']:.2f} read {h['readGBps']:.2f} GB/s, {h['ms']:.3f} ms")
    assert 0 < h["writeGBps"] <= 64, h
    assert 0 < h["readGBps"] <= 64, h


def test_floor_through_the_prober_on_a_real_result(hip):
    opts = {"hostLinkCheck": True, "hostLinkBytes": 8 * MIB}
    r = hip.run(0, overlap=0, host_link_bytes=8 * MIB, **PROBE)
    assert r["passed"]
    low = Prober.apply_floors(dict(r), {}, {**opts, "minHostLinkGBps": 1e6})
    assert not low["passed"] and low["error"].startswith("PerformanceBelowFloor: host link ")
    assert Prober.apply_floors(dict(r), {}, {**opts, "minHostLinkGBps": 0})["passed"]


def test_bad_arguments_are_reports_not_crashes(hip):
    assert "error" in hip.host_link(99, MIB) and not hip.host_link(99, MIB)["passed"]
    assert not hip.host_link(0, 8)["passed"]  # fewer than one chunk
    import ctypes
    import json
    p = hip.lib().mi355x_probe_host_link(0, json.dumps({"preload": 1}).encode(), None, 0)
    r = json.loads(ctypes.string_at(p).decode())
    hip.lib().mi355x_probe_free(p)
    assert not r["passed"] and "error" in r
