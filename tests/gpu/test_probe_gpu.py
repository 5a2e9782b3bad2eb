"""Real-MI355X tests of the gfx950 HIP probe kernels (run on the GPU box with ``-m gpu``).

Numerics: the MFMA GEMM is checked bit-exactly against an fp32 VALU reference (256^3, asymmetric
operands) and exact ABFT row/column checksums (N^3, modulo 2^32); the HBM test compares every bit. These tests also
prove the checkers *detect* corruption by injecting faults between compute and check.
"""
from __future__ import annotations

import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NATIVE = os.path.join(ROOT, "build", "native")


@pytest.fixture(scope="module")
def hip(native_built):
    from gpupool.ops import probe
    n = probe.init()
    assert n >= 1, "no HIP device visible"
    return probe


def test_mfma_fragment_layout_selftest(native_built):
    r = subprocess.run([os.path.join(NATIVE, "probe_selftest")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout)
    assert out["mfma_layout_mismatches"] == 0 and out["mfma16_layout_mismatches"] == 0


def test_identify_is_gfx950(hip):
    info = hip.identify(0)
    assert info["gcnArch"].startswith("gfx950")
    assert info["hipUUID"].startswith("GPU-")
    assert info["computeUnits"] == 256


def test_probe_passes_and_is_fast(hip):
    r = hip.run(0, hbm_bytes=1 << 30)
    assert r["passed"], r
    assert r["hbm"]["badBits"] == 0 and r["mfma"]["elementMismatches"] == 0
    assert r["mfma"]["abftMismatches"] == 0
    assert r["ms"] < 50
    # performance floors at ~0.7x of what this MI355X measures with the phases run serially
    # (profiles/r1g: ~6.0 TB/s write+read; r1c: ~1210 TFLOP/s for the 4096^3 bf16 GEMM), so a
    # 1.5x regression fails here rather than passing a 3x-lower sanity bar
    best = max((hip.run(0, hbm_bytes=1 << 30, gemm_reps=3, overlap=0) for _ in range(3)),
               key=lambda x: x["mfma"]["tflops"])
    assert best["passed"], best
    assert best["hbm"]["GBps"] > 3900, best["hbm"]
    assert best["mfma"]["tflops"] > 850, best["mfma"]


def _first_flip_offset(nbytes: int, k: int) -> int:
    """Byte offset of the lowest 16-byte chunk ``injectBitFlips=k`` corrupts: one bit in each of
    the 32-bit words stride, 2 * stride, .. k * stride, stride = words // (k + 1)."""
    return 16 * ((nbytes // 16 * 4 // (k + 1)) // 4)


def test_hbm_checker_counts_injected_bit_flips(hip):
    r = hip.run(0, hbm_bytes=256 << 20, mfma=False, injectBitFlips=37)
    assert not r["passed"]
    assert r["hbm"]["badBits"] == 37  # every flipped bit found, nothing else
    assert r["hbm"]["firstBadOffset"] == _first_flip_offset(256 << 20, 37)


def test_abft_detects_single_corrupted_element(hip):
    r = hip.run(0, hbm_bytes=1 << 20, patterns=1, gemm_n=1024, injectGemmFault=1)
    assert not r["passed"]
    assert r["mfma"]["abftMismatches"] == 2  # its row and its column checksum
    assert r["mfma"]["elementMismatches"] == 0


@pytest.mark.parametrize("mode", [2, 3])
def test_abft_flags_fractional_and_nan_elements(hip, mode):
    """A corruption that keeps the integer part (+0.25) leaves the mod-2^32 checksums of the
    truncated values intact for non-negative elements; NaN would make the int cast undefined.
    The integrality/range check fused into the column-sum pass catches both."""
    r = hip.run(0, hbm_bytes=1 << 20, patterns=1, gemm_n=1024, injectGemmFault=mode)
    assert not r["passed"], r
    assert r["mfma"]["abftMismatches"] >= 1


def test_cu_census_covers_every_cu(hip):
    """Every one of the 256 CUs (8 XCDs x 32) proves its matrix cores with an exactly-checked
    MFMA chain, identified by the XCC_ID / HW_ID hardware registers of the wave."""
    r = hip.run(0, hbm_bytes=64 << 20)
    assert r["passed"], r
    cus = r["cus"]
    assert cus["expected"] == 256 and cus["mfmaVerified"] == 256 and cus["badWaves"] == 0, cus
    assert cus["perXcd"] == [32] * 8, cus
    assert 0 < cus["gemmTiles"] <= 256  # CUs that ran tiles of the timed 4096^3 GEMM


def test_cu_census_detects_a_bad_xcd(hip):
    r = hip.run(0, hbm_bytes=1 << 20, patterns=1, gemm_n=1024, injectCensusFaultXcc=3)
    assert not r["passed"], r
    cus = r["cus"]
    assert cus["perXcd"][3] == 0 and cus["mfmaVerified"] == 224 and cus["badWaves"] > 0, cus
    assert not cus["ok"]


@pytest.mark.parametrize("mnk", [(1024, 768, 512), (2048, 2048, 2048), (512, 2048, 1024)])
def test_probe_gemm_matches_torch_fp64_cpu(hip, mnk):
    """Independent numerics oracle: the probe's production MFMA GEMM on random normal bf16
    operands (non-integer: bf16 rounding and fp32 accumulation order are exercised) against a
    float64 CPU torch.matmul of the same bf16 values (torch's own HIP runtime cannot share device
    pointers with the probe library, so the oracle runs on the host). Tolerance: fp32
    accumulation of K products, |err| <= 2e-6 * sqrt(K) * max|ref|."""
    import torch
    m, n, k = mnk
    g = torch.Generator().manual_seed(m + n + k)
    a = torch.randn(m, k, generator=g).to(torch.bfloat16).contiguous()
    bt = torch.randn(n, k, generator=g).to(torch.bfloat16).contiguous()
    c = torch.full((m, n), float("nan"), dtype=torch.float32)
    hip.gemm_bf16(0, a.data_ptr(), bt.data_ptr(), c.data_ptr(), m, n, k)
    ref = a.double() @ bt.double().T
    err = (c.double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert torch.isfinite(c).all()
    assert err <= 2e-6 * (k ** 0.5) * scale, (err, scale)
    with pytest.raises(ValueError):
        hip.gemm_bf16(0, a.data_ptr(), bt.data_ptr(), c.data_ptr(), m + 1, n, k)


def test_hbm_sweep_windows_cover_free_hbm(hip):
    """The rotating sweep: windows of a buffer spanning (nearly) all free HBM are pattern-tested,
    an injected flip inside a window is found at the right offset, and the buffer is released."""
    a = hip.hbm_sweep(0, 0, 4 << 30, keep=True)
    assert a["passed"], a
    assert a["span"] > 200e9, a  # ~288 GB MI355X minus the 4 GiB reserve and what is in use
    far = a["span"] - (2 << 30)
    b = hip.hbm_sweep(0, far, 4 << 30, keep=True)
    assert b["passed"] and b["offset"] == far and b["bytes"] == 2 << 30, b
    c = hip.hbm_sweep(0, 64 << 30, 1 << 30, keep=True, injectBitFlips=11)
    assert not c["passed"] and c["badBits"] == 11 and c["firstBadOffset"] >= 64 << 30, c
    assert a["GBps"] > 3000, a
    assert hip.sweep_release(0) == 1 and hip.sweep_release(0) == 0


def test_probe_cli(native_built):
    r = subprocess.run([os.path.join(NATIVE, "mi355x-probe"), "--hbm-bytes", str(64 << 20),
                        "--gemm-n", "1024"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for line in r.stdout.strip().splitlines():
        assert json.loads(line)["passed"]


@pytest.mark.parametrize("n", [256, 512, 1280, 2048])
@pytest.mark.parametrize("tile", [128, 256])
def test_gemm_kernels_exact_at_sizes(hip, n, tile):
    """Both GEMM kernels (256x256 glds and 128x128 register-staged) are bit-exact (ABFT) at
    several N, including one that is not a power of two (1280 = 5 x 256)."""
    r = hip.run(0, hbm_bytes=1 << 20, patterns=1, gemm_n=n, gemm_tile=tile)
    assert r["passed"], r
    assert r["mfma"]["tile"] == tile and r["mfma"]["n"] == n
    assert r["mfma"]["abftMismatches"] == 0 and r["mfma"]["elementMismatches"] == 0


def test_poisoned_c_fails_when_the_gemm_does_not_run(hip):
    """The poisonC hook is only meaningful if an unwritten C fails the checks even though the
    reused arena still holds an identical earlier result: poison C, skip the GEMM (gemmSkip) and
    the ABFT checks must fail — with the poison and a real GEMM the probe passes (below)."""
    clean = hip.run(0, hbm_bytes=1 << 20, patterns=1, gemm_n=1024)
    assert clean["passed"], clean  # the arena now holds the right C for these operands
    r = hip.run(0, hbm_bytes=1 << 20, patterns=1, gemm_n=1024, poisonC=1, gemmSkip=1)
    assert not r["passed"] and r["mfma"]["abftMismatches"] > 0, r
    again = hip.run(0, hbm_bytes=1 << 20, patterns=1, gemm_n=1024, poisonC=1)
    assert again["passed"], again


@pytest.mark.parametrize("n", [1280, 2048, 4096])
@pytest.mark.parametrize("group_m", [2, 3, 4, 8])
def test_grouped_tile_order_is_exact(hip, n, group_m):
    """The grouped tile order (``gemmGroupM``) is a bijection over the tiles, also when the last
    group is short (1280 = 5 tile rows with groups of 2, 3, 4): every C element is written once
    and right (exact ABFT row/column checksums), and the census still sees every CU."""
    r = hip.run(0, hbm_bytes=1 << 20, patterns=1, gemm_n=n, gemmGroupM=group_m, poisonC=1)
    assert r["passed"], r
    assert r["mfma"]["abftMismatches"] == 0 and r["mfma"]["elementMismatches"] == 0


@pytest.mark.parametrize("n", [256, 1280, 4096])
def test_vectorised_c_store_gemm_is_exact(hip, n):
    """The transposed-MFMA variant with 16-byte C stores (``gemmVecC``, an option of the 2-phase
    loop: ``gemmPipe`` 0) computes the same C: the
    256^3 element-by-element check against the VALU reference and the exact ABFT checksums pass,
    with C poisoned before the GEMM."""
    r = hip.run(0, hbm_bytes=1 << 20, patterns=1, gemm_n=n, gemmPipe=0, gemmVecC=1, poisonC=1)
    assert r["passed"], r
    assert r["mfma"]["abftMismatches"] == 0 and r["mfma"]["elementMismatches"] == 0


@pytest.mark.parametrize("pipe", [0, 1, 2, 3, 21])
@pytest.mark.parametrize("n", [256, 512, 1280, 2048, 4096])
def test_half_tile_pipelined_gemm_is_exact_run_after_run(hip, n, pipe):
    """The K-loops of the 256x256 kernel — the 2-phase loop and the half-tile pipeline whose DMA
    stays in flight across barriers (``gemmPipe`` 1; 2 with the wave groups one barrier apart) —
    against the exact checks, with C poisoned
    before each run, several runs per size: a read placed before its DMA has landed would show as
    a wrong tile in some runs and not others (cdna_hip_programming.md §5 "Read a staged buffer
    one phase AFTER the wait that retires it"). 256 is one K-tile (prologue + last tile only)."""
    for _ in range(8):
        r = hip.run(0, hbm_bytes=1 << 20, patterns=1, gemm_n=n, gemmPipe=pipe, poisonC=1)
        assert r["passed"], r
        assert r["mfma"]["abftMismatches"] == 0 and r["mfma"]["elementMismatches"] == 0


def test_overlapped_and_serial_probe_agree(hip):
    """The two-stream probe (HBM test beside the MFMA phase) finds the same injected faults as
    the serial one and both pass clean runs."""
    for overlap in (0, 1):
        clean = hip.run(0, hbm_bytes=256 << 20, overlap=overlap)
        assert clean["passed"], clean
        bad = hip.run(0, hbm_bytes=256 << 20, gemm_n=1024, overlap=overlap, injectBitFlips=5,
                      injectGemmFault=1)
        assert not bad["passed"]
        assert bad["hbm"]["badBits"] == 5 and bad["mfma"]["abftMismatches"] == 2


@pytest.mark.parametrize("zero_in_kernel", [1, 0])
@pytest.mark.parametrize("overlap", [1, 0])
def test_counters_reset_after_a_faulty_probe(hip, overlap, zero_in_kernel):
    """The result counters live in the kept arena: a clean probe right after a faulty one must
    start from zero (and the first-bad offset from all-ones) on both reset paths — in-kernel
    (the first fill / operand kernel, default) and memsets."""
    kw = dict(hbm_bytes=256 << 20, gemm_n=1024, overlap=overlap, zeroInKernel=zero_in_kernel)
    bad = hip.run(0, injectBitFlips=7, injectGemmFault=1, injectCensusFaultXcc=3, **kw)
    assert not bad["passed"] and bad["hbm"]["badBits"] == 7 and bad["mfma"]["abftMismatches"] == 2
    assert bad["hbm"]["firstBadOffset"] == _first_flip_offset(256 << 20, 7) and bad["cus"]["badWaves"] > 0
    clean = hip.run(0, **kw)
    assert clean["passed"], clean
    assert clean["hbm"]["badBits"] == 0 and clean["hbm"]["firstBadOffset"] is None
    assert clean["mfma"]["abftMismatches"] == 0 and clean["mfma"]["elementMismatches"] == 0
    assert clean["cus"]["badWaves"] == 0 and clean["cus"]["ok"]


def test_peer_copy_path(hip):
    """The xGMI peer check's copy + bit-exact verify path. On a 1-GPU box src == dst exercises
    it as a local device copy; with more GPUs visible, 0 -> 1 goes over an xGMI link."""
    n = hip.init()
    r = hip.peer(0, 0, 64 << 20)
    assert r["passed"] and r["canAccessPeer"] and r["badBits"] == 0, r
    assert r["GBps"] > 100, r
    if n > 1:
        x = hip.peer(0, 1, 64 << 20)
        assert x["passed"] and x["badBits"] == 0, x
        assert x["GBps"] > 10, x


def test_peer_ring_in_one_call(hip):
    """The concurrent ring entry point (all links at once, windows kept between calls). On a
    1-GPU box rings of [0, 0] and [0, 0, 0] run every link as a local copy through the same code;
    with more GPUs visible, the first four form a real xGMI ring."""
    n = hip.init()
    for ring in ([0, 0], [0, 0, 0]):
        r = hip.peer_ring(ring, 32 << 20)
        assert r["passed"] and len(r["links"]) == len(ring), r
        for i, link in enumerate(r["links"]):
            assert (link["src"], link["dst"]) == (ring[i], ring[(i + 1) % len(ring)])
            assert link["passed"] and link["badBits"] == 0 and link["bytes"] == 32 << 20, link
            assert link["GBps"] > 50, link
    again = hip.peer_ring([0, 0], 32 << 20)  # windows reused
    assert again["passed"], again
    hip.trim(0)  # frees the ring windows with the arena; the next ring allocates them again
    assert hip.peer_ring([0, 0], 16 << 20)["passed"]
    if n > 1:
        ring = list(range(min(n, 4)))
        r = hip.peer_ring(ring, 64 << 20)
        assert r["passed"] and all(x["GBps"] > 10 for x in r["links"]), r


def test_probe_arena_reused_then_trimmed(hip):
    """The ~1.2 GiB probe arena is kept between back-to-back probes (no hipMalloc on the claim
    path) and handed back by trim(); a probe after a trim allocates again and still passes."""
    hip.trim(0)
    a = hip.run(0, hbm_bytes=1 << 30)
    b = hip.run(0, hbm_bytes=1 << 30)
    assert a["passed"] and b["passed"]
    assert a["phases"]["arenaReused"] is False and b["phases"]["arenaReused"] is True
    assert b["phases"]["allocMs"] < a["phases"]["allocMs"]
    assert hip.trim(0) == 1 and hip.trim(0) == 0
    c = hip.run(0, hbm_bytes=1 << 30)
    assert c["passed"] and c["phases"]["arenaReused"] is False
    hip.trim(0)


def test_concurrent_probes_of_one_device_serialise(hip):
    """Two probes of the same GPU at once (e.g. a claim and a periodic recheck): the per-device
    lock serialises them (wall >= the sum of their own kernel walls) and neither corrupts the
    other's arena (both pass, no flipped bits, no GEMM mismatches)."""
    import concurrent.futures as cf
    import time
    hip.run(0, hbm_bytes=1 << 30)  # arena warm
    with cf.ThreadPoolExecutor(2) as ex:
        t0 = time.perf_counter()
        futs = [ex.submit(hip.run, 0, 1 << 30) for _ in range(2)]
        rs = [f.result() for f in futs]
        wall_ms = (time.perf_counter() - t0) * 1e3
    for r in rs:
        assert r["passed"], r
        assert r["hbm"]["badBits"] == 0 and not r["mfma"].get("elementMismatches")
    assert wall_ms >= 0.9 * sum(r["ms"] for r in rs), (wall_ms, [r["ms"] for r in rs])
