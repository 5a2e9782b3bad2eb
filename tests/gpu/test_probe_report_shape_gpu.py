"""The shape of every report the probe library returns, on a real MI355X (run with ``-m gpu``).

The agent, the scripts and the other tests read these reports by key; the ordered key sequence of
each report and of each nested block is pinned here, as the library produced it before its source
was split into per-phase headers (recorded from that build), so a change to the report writers
shows up as a diff of these lists. Small sizes: the whole file runs in under two seconds.
"""
from __future__ import annotations

import pytest

pytestmark = pytest.mark.gpu

MIB = 1 << 20
SMALL = dict(hbm_bytes=MIB, patterns=2, gemm_n=256)

HEAD = ["device", "hipUUID", "gcnArch", "passed", "hbm", "mfma"]
TAIL = ["ms", "phases", "reportMs"]
HBM = ["ok", "bytes", "patterns", "badBits", "firstBadOffset", "writeGBps", "readGBps", "GBps", "ms"]
MFMA = ["ok", "enabled", "n", "tile", "pipe", "elementMismatches", "abftMismatches", "tflops", "ms"]
CUS = ["expected", "mfmaVerified", "perXcd", "gemmTiles", "badWaves", "ok"]
LOWP = ["fp8", "mxfp8", "mxfp4"]
LOWP_ENTRY = ["ok", "n", "elementMismatches", "abftMismatches", "tflops", "ms", "cusVerified", "badWaves"]
HOST_LINK = ["ok", "bytes", "patterns", "seed", "badBits", "firstBadOffset", "hostSamples",
             "hostSampleMismatches", "writeGBps", "readGBps", "GBps", "ms", "allocMs"]
PHASES = ["arenaReused", "setupMs", "allocMs", "launchMs", "hbmFirst", "hbmWallMs", "mfmaWallMs", "freeMs"]
SWEEP = ["device", "passed", "offset", "bytes", "span", "badBits", "firstBadOffset", "GBps", "ms", "allocMs"]
RING = ["bytes", "links", "passed"]
LINK = ["src", "dst", "canAccessPeer", "passed", "badBits", "firstBadOffset", "bytes", "GBps", "ms", "seed"]


@pytest.fixture(scope="module")
def hip(native_built):
    from gpupool.ops import probe
    assert probe.init() >= 1, "no HIP device visible"
    return probe


def _common(r: dict) -> None:
    assert r["passed"] is True, r
    assert list(r["hbm"]) == HBM
    assert list(r["mfma"]) == MFMA
    assert list(r["phases"]) == PHASES
    assert r["hbm"]["firstBadOffset"] is None and r["hbm"]["bytes"] == MIB and r["hbm"]["patterns"] == 2


def test_plain_probe(hip):
    r = hip.run(0, **SMALL)
    assert list(r) == HEAD + ["cus"] + TAIL
    _common(r)
    assert list(r["cus"]) == CUS
    assert r["mfma"]["enabled"] is True and r["mfma"]["n"] == 256


def test_probe_with_low_precision_and_host_link(hip):
    r = hip.run(0, mfma_low_precision=("fp8", "mxfp8", "mxfp4"), host_link_bytes=MIB, **SMALL)
    assert list(r) == HEAD + ["cus", "lowp", "hostLink"] + TAIL
    _common(r)
    assert list(r["cus"]) == CUS
    assert list(r["lowp"]) == LOWP
    for name in LOWP:
        assert list(r["lowp"][name]) == LOWP_ENTRY, name
        assert r["lowp"][name]["ok"] is True, r["lowp"][name]
    assert list(r["hostLink"]) == HOST_LINK
    assert r["hostLink"]["ok"] is True and r["hostLink"]["firstBadOffset"] is None


def test_probe_without_mfma(hip):
    r = hip.run(0, mfma=False, **SMALL)
    assert list(r) == HEAD + TAIL  # no "cus" without the phase that fills it
    _common(r)
    assert r["mfma"]["enabled"] is False


def test_sweep_window(hip):
    # a small sweep buffer: everything but 16 GiB of the device stays reserved
    reserve = int(hip.identify(0)["totalMem"]) - (16 << 30)
    r = hip.hbm_sweep(0, 0, MIB, reserve=reserve, keep=False)
    assert list(r) == SWEEP, r
    assert r["passed"] is True and r["bytes"] == MIB and r["firstBadOffset"] is None, r


def test_peer_ring(hip):
    r = hip.peer_ring([0, 0], nbytes=MIB)
    assert list(r) == RING, r
    assert r["passed"] is True and len(r["links"]) == 2
    for link in r["links"]:
        assert list(link) == LINK
        assert link["passed"] is True and link["bytes"] == MIB


def test_host_link_alone(hip):
    r = hip.host_link(0, MIB)
    assert list(r) == ["device", "passed"] + HOST_LINK  # the block is the whole report, with the usual head
    assert r["passed"] is True and r["bytes"] == MIB
