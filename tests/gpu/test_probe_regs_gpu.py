"""The probe's register-file phase on a real MI355X (run with ``-m gpu``).

Every workgroup of the phase's kernel owns its CU: the kernel asks for all 512 vector registers per
lane (v0..v255, a0..a255), so one wave sits on each of the CU's four SIMDs and marches that SIMD's
whole file in both polarities. The tests compare workgroup 0's registers word for word with the
numpy twin (``gpupool.ops.regfile``) at the two points the kernel can dump them, which proves that
every register is written with the value the verify expects, and prove on the hardware that a
flipped bit (in every wave, on one SIMD, on one XCD) and a register the write skipped are found
where they are. The registers sit at the seams: u = 0, 15, 16 (between the two asm statements), 255,
256 (between the arch and the acc half) and 511.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from gpupool.agent import simprobe
from gpupool.agent.prober import Prober
from gpupool.ops import regfile

pytestmark = pytest.mark.gpu

SALT = 0x5A17
SEED = regfile.SEED_BASE ^ SALT  # device ordinal 0
SEAMS = (0, 15, 16, 255, 256, 511)
MIB = 1 << 20
PROBE = dict(hbm_bytes=64 * MIB, gemm_n=512)
DEFAULT_KEYS = {"device", "hipUUID", "gcnArch", "passed", "hbm", "mfma", "cus", "ms", "phases", "reportMs"}
PHASE_KEYS = {"arenaReused", "setupMs", "allocMs", "launchMs", "hbmFirst", "hbmWallMs", "mfmaWallMs", "freeMs"}
BLOCK_KEYS = ["ok", "registersPerLane", "workgroupsPerCU", "patterns", "salt", "workgroups", "cusTested",
              "cusVerified", "simdsTested", "simdShort", "perXcd", "badCUs", "badBits", "firstBadCU",
              "firstBadSimd", "firstBadRegister", "firstBadLane", "ms"]


@pytest.fixture(scope="module")
def hip(native_built):
    from gpupool.ops import probe
    n = probe.init()
    assert n >= 1, "no HIP device visible"
    return probe


@pytest.fixture(scope="module")
def cus(hip):
    return int(hip.identify(0)["computeUnits"])


@pytest.fixture(scope="module")
def clean(hip):
    """One clean run at the defaults, shared."""
    return hip.regs(0)


@functools.lru_cache(maxsize=None)
def _ref(stage: int) -> np.ndarray:
    """Workgroup 0's registers at a dump stage, computed once."""
    return regfile.expected(0, SEED, 0 if stage == 1 else 0xFFFFFFFF)


@pytest.mark.parametrize("stage", (1, 2))
def test_dump_of_workgroup_0_equals_the_twin(hip, stage):
    r = hip.regs(0, want_stage=stage, regsSalt=SALT, requireAllCUs=0)
    assert list(r) == ["device", "passed"] + BLOCK_KEYS + ["dumpCU", "dumpSimds", "data"], list(r)
    assert r["passed"] and r["salt"] == SALT and r["badBits"] == 0, {k: v for k, v in r.items() if k != "data"}
    assert r["registersPerLane"] == 512 and r["workgroupsPerCU"] == 1  # the test instantiation owns its CU too
    assert 0 <= r["dumpCU"] < 2048
    assert sorted(r["dumpSimds"]) == [0, 1, 2, 3], r["dumpSimds"]  # HW_ID[5:4]: one wave per SIMD
    got, want = r["data"], _ref(stage)
    assert got.shape == want.shape == (4, 512, 64) and got.dtype == want.dtype == np.uint32
    diff = np.argwhere(got != want)
    assert diff.size == 0, f"{len(diff)} word(s) differ, first at (wave, register, lane) {tuple(diff[0])}"
    for u in SEAMS:  # spelled out: the seams between the statements and between the halves
        assert (got[:, u, :] == want[:, u, :]).all(), u


def test_clean_run_at_the_defaults(hip, cus, clean):
    r = clean
    print(f"regs: {r['cusTested']}/{cus} CUs by {r['workgroups']} workgroups in {r['ms']:.3f} ms")
    assert list(r) == ["device", "passed"] + BLOCK_KEYS, list(r)
    assert r["passed"] and r["ok"], r
    assert r["registersPerLane"] == 512 and r["workgroupsPerCU"] == 1, r
    assert r["patterns"] == 2 and r["simdShort"] == 0, r
    assert r["badBits"] == 0 and r["badCUs"] == 0, r
    assert r["firstBadCU"] is None and r["firstBadSimd"] is None and r["firstBadRegister"] is None \
        and r["firstBadLane"] is None, r
    assert r["simdsTested"] == 4 * r["cusTested"], r
    assert r["cusVerified"] == r["cusTested"] == sum(r["perXcd"]) == cus, r
    for factor in (1, 3):  # workgroups == regsBlocksPerCU x CUs: all of them ran
        f = hip.regs(0, regsBlocksPerCU=factor, requireAllCUs=0)
        assert f["passed"] and f["workgroups"] == factor * cus, f
    assert r["workgroups"] == simprobe.SIM_REGS_BLOCKS_PER_CU * cus, r  # the default factor (options.h)
    salts = [hip.regs(0, requireAllCUs=0)["salt"] for _ in range(2)]
    assert salts[1] == salts[0] + 1  # the default salt is the device's run counter


@pytest.mark.parametrize("u", SEAMS)
def test_one_flip(hip, u):
    for lane in (0, 31, 32, 63):
        for bit in (0, 31):
            r = hip.regs(0, injectRegFlip=[u, lane, bit], requireAllCUs=0)
            assert not r["passed"] and not r["ok"], r
            assert r["registersPerLane"] == 512 and r["workgroupsPerCU"] == 1, r
            assert r["badBits"] == 4 * r["workgroups"], r  # one bit per wave, found once
            assert r["firstBadRegister"] == u and r["firstBadLane"] == lane, r
            assert r["badCUs"] == r["cusTested"] > 0 and r["cusVerified"] == 0 and sum(r["perXcd"]) == 0, r
            assert 0 <= r["firstBadCU"] < 2048 and 0 <= r["firstBadSimd"] < 4


def test_a_hook_past_the_range_is_off(hip):
    for flip in ([512, 0, 0], [0, 64, 0], [0, 0, 32], [-1, 0, 0]):
        r = hip.regs(0, injectRegFlip=flip)
        assert r["passed"] and r["badBits"] == 0, (flip, r)
    r = hip.regs(0, injectRegSkip=512)
    assert r["passed"] and r["badBits"] == 0, r


@pytest.mark.parametrize("simd", (0, 1, 2, 3))
def test_a_flip_on_one_simd(hip, simd):
    r = hip.regs(0, injectRegFlip=[300, 17, 5], injectRegFaultSimd=simd)
    assert not r["passed"], r
    assert r["firstBadSimd"] == simd and r["badBits"] == r["workgroups"], r  # one wave of every workgroup
    assert r["firstBadRegister"] == 300 and r["firstBadLane"] == 17, r


def test_a_flip_on_one_xcd(hip, cus, clean):
    assert clean["passed"], clean
    r = hip.regs(0, injectRegFlip=[77, 9, 13], injectRegFaultXcc=3)
    assert not r["passed"] and r["cusTested"] == cus, r
    assert r["badCUs"] == clean["perXcd"][3] > 0, r  # the tested CUs of XCD 3, no other
    assert r["firstBadCU"] >> 8 == 3 and r["firstBadRegister"] == 77 and r["firstBadLane"] == 9, r
    assert r["perXcd"] == [0 if x == 3 else n for x, n in enumerate(clean["perXcd"])], r
    assert r["cusVerified"] == cus - r["badCUs"]
    assert 4 * r["badCUs"] <= r["badBits"] < 4 * r["workgroups"], r


@pytest.mark.parametrize("u", (0, 16, 300, 511))
def test_a_register_the_write_skipped(hip, u):
    """What the register still holds is another workgroup's or another run's value (the base depends
    on workgroup, wave, lane and the salted seed), so the verify fails there: a stale word equals the
    expected one with probability 2^-32 per lane, and 16 workgroups per CU of 256 lanes each put a
    CU whose every lane matched out of reach."""
    r = hip.regs(0, injectRegSkip=u, regsBlocksPerCU=16, requireAllCUs=0)
    assert not r["passed"] and r["badBits"] > 0, r
    assert r["firstBadRegister"] == u, r
    assert r["badCUs"] == r["cusTested"] and r["cusVerified"] == 0, r


def test_inside_the_claim_probe(hip, cus):
    r = hip.run(0, reg_check=True, **PROBE)
    assert set(r) == DEFAULT_KEYS | {"regs"}, sorted(r)
    assert list(r).index("regs") == list(r).index("ms") - 1
    assert list(r["regs"]) == BLOCK_KEYS and set(r["phases"]) == PHASE_KEYS
    print(f"regs inside the probe: {r['regs']['cusTested']}/{cus} CUs in {r['regs']['ms']:.3f} ms")
    assert r["hbm"]["ok"] and r["mfma"]["ok"] and r["cus"]["ok"], r
    assert r["regs"]["badBits"] == 0 and r["regs"]["cusVerified"] == r["regs"]["cusTested"] == cus, r["regs"]
    assert r["passed"] and r["regs"]["ok"], r
    for extra in ({}, {"regsFirst": 0}, {"regsFirst": 1}, {"overlap": 0}, {"mfma": False}):
        f = hip.run(0, reg_check=True, injectRegFlip=[256 + 3, 40, 1], **{**PROBE, **extra})
        assert not f["passed"] and not f["regs"]["ok"], f
        assert f["hbm"]["ok"] and f["mfma"]["ok"] and f.get("cus", {"ok": True})["ok"], f
        assert f["regs"]["badBits"] == 4 * f["regs"]["workgroups"] and f["regs"]["firstBadRegister"] == 259, f["regs"]
        err = Prober.explain(f)["error"]
        assert err.startswith(f"RegisterFileMismatch: {f['regs']['badBits']} flipped bit(s) on "
                              f"{f['regs']['badCUs']} CU(s), first on CU ") \
            and f" SIMD {f['regs']['firstBadSimd']} register a3 lane 40" in err, err
    both = hip.run(0, reg_check=True, lds_check=True, **PROBE)  # beside the LDS phase, after it in the report
    assert both["passed"] and list(both).index("regs") == list(both).index("lds") + 1, both
    # with the option off after runs with it on: exactly the default report
    for off in (hip.run(0, **PROBE), hip.run(0, reg_check=False, **PROBE)):
        assert set(off) == DEFAULT_KEYS and set(off["phases"]) == PHASE_KEYS and off["passed"], off


def test_bad_arguments_are_reports(hip):
    for r in (hip.regs(99), hip.regs(-1), hip.regs(99, want_stage=1)):
        assert r["passed"] is False and r["error"], r
        assert "regs" not in r and "registersPerLane" not in r and "data" not in r
    assert hip.regs(0, patterns=99)["patterns"] == 4  # clamped, not refused
    assert hip.run(0, **PROBE)["passed"]
