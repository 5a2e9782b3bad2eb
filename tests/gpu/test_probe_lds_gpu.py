"""The probe's LDS phase on a real MI355X (run with ``-m gpu``).

Every workgroup of the phase's kernel owns its CU's whole Local Data Share, marches the tested part
in both polarities and address-tests it at dword granularity. The tests compare workgroup 0's LDS
byte for byte with the numpy twin (``gpupool.ops.lds``) at the three points the kernel can dump it,
and prove on the hardware that a flipped bit, a flip on one XCD only and a chunk the write skipped
are found where they are, per CU. Sizes sit where the loops can go wrong: fewer chunks than threads,
one pass of all threads plus one tail chunk, 660 dwords (the stride search passes 33 and 35), just
past 64 KiB, a size that rounds down, and the full 160 KiB.

Coverage (every CU reached by a workgroup) is asserted at the full size with the defaults, the claim
probe's configuration. Below it a workgroup lives for well under a microsecond of LDS work and the
dispatcher's placement is not the subject: those runs pass ``requireAllCUs=0`` and print what they
covered.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from gpupool.agent.prober import Prober
from gpupool.ops import lds

pytestmark = pytest.mark.gpu

FULL = lds.BYTES_PER_CU
SIZES = (1600, 16 * 257, 2640, 65552, 163832, FULL)
SALT = 0x5A17
SEED = lds.SEED_BASE ^ SALT  # device ordinal 0
MIB = 1 << 20
PROBE = dict(hbm_bytes=64 * MIB, gemm_n=512)
DEFAULT_KEYS = {"device", "hipUUID", "gcnArch", "passed", "hbm", "mfma", "cus", "ms", "phases", "reportMs"}
PHASE_KEYS = {"arenaReused", "setupMs", "allocMs", "launchMs", "hbmFirst", "hbmWallMs", "mfmaWallMs", "freeMs"}
BLOCK_KEYS = {"ok", "bytesPerCU", "patterns", "salt", "workgroups", "cusTested", "cusVerified", "perXcd",
              "badCUs", "badBits", "firstBadCU", "firstBadOffset", "ms"}


@pytest.fixture(scope="module")
def hip(native_built):
    from gpupool.ops import probe
    n = probe.init()
    assert n >= 1, "no HIP device visible"
    return probe


@pytest.fixture(scope="module")
def cus(hip):
    return int(hip.identify(0)["computeUnits"])


def _relaxed(nbytes: int) -> dict:
    return {} if nbytes == FULL else {"requireAllCUs": 0}


@functools.lru_cache(maxsize=None)
def _ref(chunks: int, stage: int) -> bytes:
    """Workgroup 0's LDS at a dump stage, computed once per size and stage."""
    if stage == 3:
        return lds.address_words(0, 4 * chunks, SEED).astype("<u4").tobytes()
    return lds.march_bytes(0, chunks, SEED, 0 if stage == 1 else 0xFFFFFFFF).tobytes()


@pytest.mark.parametrize("stage", (1, 2, 3))
@pytest.mark.parametrize("nbytes", SIZES)
def test_dump_of_workgroup_0_equals_the_twin(hip, nbytes, stage):
    r = hip.lds(0, nbytes, want_stage=stage, ldsSalt=SALT, requireAllCUs=0)
    assert set(r) == BLOCK_KEYS | {"device", "passed", "dumpCU", "data"}, sorted(r)
    chunks = nbytes // 16
    assert r["passed"] and r["bytesPerCU"] == 16 * chunks and r["salt"] == SALT, r
    assert 0 <= r["dumpCU"] < 2048
    got, want = np.frombuffer(r["data"], np.uint8), np.frombuffer(_ref(chunks, stage), np.uint8)
    assert got.size == want.size == 16 * chunks
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, f"{diff.size} byte(s) differ, first at {diff[0]}"


@pytest.mark.parametrize("nbytes", SIZES)
def test_clean_run(hip, cus, nbytes):
    r = hip.lds(0, nbytes, **_relaxed(nbytes))
    print(f"lds {nbytes} B: {r['cusTested']}/{cus} CUs by {r['workgroups']} workgroups in {r['ms']:.3f} ms")
    assert set(r) == BLOCK_KEYS | {"device", "passed"}, sorted(r)
    assert r["passed"] and r["ok"], r
    assert r["bytesPerCU"] == nbytes // 16 * 16 and r["patterns"] == 2
    assert r["badBits"] == 0 and r["badCUs"] == 0 and r["firstBadCU"] is None and r["firstBadOffset"] is None, r
    assert r["workgroups"] % cus == 0 and r["workgroups"] >= cus, r  # ldsBlocksPerCU x CUs, all of them ran
    assert r["cusVerified"] == r["cusTested"] == sum(r["perXcd"]), r
    if nbytes == FULL:
        assert r["cusVerified"] == cus, r


def test_workgroups_follow_the_grid_factor(hip, cus):
    for factor in (1, 3):
        r = hip.lds(0, 1600, ldsBlocksPerCU=factor, requireAllCUs=0)
        assert r["passed"] and r["workgroups"] == factor * cus, r
    salts = [hip.lds(0, 1600, requireAllCUs=0)["salt"] for _ in range(2)]
    assert salts[1] == salts[0] + 1  # the default salt is the device's run counter


@pytest.mark.parametrize("nbytes", SIZES)
def test_a_flip_in_every_workgroup(hip, nbytes):
    tested = nbytes // 16 * 16
    for o in (0, tested - 1, tested // 32 * 16 + 5):
        r = hip.lds(0, nbytes, injectLdsFlipAtByte=o, **_relaxed(nbytes))
        assert not r["passed"] and not r["ok"], r
        assert r["badBits"] == r["workgroups"], r  # one bit per workgroup, found once
        assert r["firstBadOffset"] == o, r
        assert r["badCUs"] == r["cusTested"] > 0 and r["cusVerified"] == 0 and sum(r["perXcd"]) == 0, r
        assert 0 <= r["firstBadCU"] < 2048
    r = hip.lds(0, nbytes, injectLdsFlipAtByte=tested, **_relaxed(nbytes))  # past the tested range
    assert r["passed"] and r["badBits"] == 0, r


def test_a_flip_on_one_xcd(hip, cus):
    clean = hip.lds(0, FULL)
    assert clean["passed"], clean
    r = hip.lds(0, FULL, injectLdsFlipAtByte=4097, injectLdsFaultXcc=3)
    assert not r["passed"] and r["cusTested"] == cus, r
    assert r["badCUs"] == clean["perXcd"][3] > 0, r  # the tested CUs of XCD 3, no other
    assert r["firstBadCU"] >> 8 == 3 and r["firstBadOffset"] == 4097, r
    assert r["perXcd"] == [0 if x == 3 else n for x, n in enumerate(clean["perXcd"])], r
    assert r["cusVerified"] == cus - r["badCUs"]
    assert r["badCUs"] <= r["badBits"] < r["workgroups"], r


@pytest.mark.parametrize("nbytes", SIZES)
def test_a_chunk_the_write_skipped(hip, nbytes):
    """What the chunk still holds is another workgroup's or another run's value, so the verify fails
    there. The reported offset is the chunk's first byte unless, on the lowest-keyed CU, the stale
    first byte equals the expected one in every workgroup that ran there (1 in 256 each): 16
    workgroups per CU put that out of reach."""
    for j in (0, nbytes // 16 - 1):
        r = hip.lds(0, nbytes, injectLdsSkipChunk=j, ldsBlocksPerCU=16, **_relaxed(nbytes))
        assert not r["passed"] and r["badBits"] > 0, r  # stale bytes never verify
        assert r["firstBadOffset"] == 16 * j, r
        assert r["badCUs"] == r["cusTested"] and r["cusVerified"] == 0, r
    r = hip.lds(0, nbytes, injectLdsSkipChunk=nbytes // 16, **_relaxed(nbytes))  # no such chunk
    assert r["passed"], r


def test_inside_the_claim_probe(hip, cus):
    r = hip.run(0, lds_check=True, **PROBE)
    assert set(r) == DEFAULT_KEYS | {"lds"}, sorted(r)
    assert list(r).index("lds") == list(r).index("ms") - 1
    assert set(r["lds"]) == BLOCK_KEYS and set(r["phases"]) == PHASE_KEYS
    print(f"lds inside the probe: {r['lds']['cusTested']}/{cus} CUs in {r['lds']['ms']:.3f} ms")
    assert r["hbm"]["ok"] and r["mfma"]["ok"] and r["cus"]["ok"], r
    assert r["lds"]["badBits"] == 0 and r["lds"]["cusVerified"] == r["lds"]["cusTested"], r["lds"]
    assert r["lds"]["bytesPerCU"] == FULL and r["lds"]["cusVerified"] == cus, r["lds"]
    assert r["passed"] and r["lds"]["ok"], r
    for extra in ({}, {"ldsFirst": 0}, {"ldsFirst": 1}, {"overlap": 0}, {"mfma": False}):
        f = hip.run(0, lds_check=True, injectLdsFlipAtByte=100, **{**PROBE, **extra})
        assert not f["passed"] and not f["lds"]["ok"], f
        assert f["hbm"]["ok"] and f["mfma"]["ok"] and f.get("cus", {"ok": True})["ok"], f
        assert f["lds"]["badBits"] == f["lds"]["workgroups"] and f["lds"]["firstBadOffset"] == 100, f["lds"]
        err = Prober.explain(f)["error"]
        assert err.startswith(f"LDSPatternMismatch: {f['lds']['badBits']} flipped bit(s) on {f['lds']['badCUs']} CU(s), "
                              f"first on CU ") and err.endswith(" at LDS offset 100"), err
    # with the option off after runs with it on: exactly the default report
    for off in (hip.run(0, **PROBE), hip.run(0, lds_check=False, **PROBE)):
        assert set(off) == DEFAULT_KEYS and set(off["phases"]) == PHASE_KEYS and off["passed"], off


def test_bad_arguments_are_reports(hip):
    for r in (hip.lds(99), hip.lds(0, 8), hip.lds(0, 200000), hip.lds(0, 0), hip.lds(0, -16)):
        assert r["passed"] is False and r["error"], r
        assert "lds" not in r and "bytesPerCU" not in r
    r = hip.run(0, lds_check=True, ldsBytes=200000, **PROBE)
    assert r["passed"] is False and "ldsBytes" in r["error"], r
    assert hip.run(0, **PROBE)["passed"]
