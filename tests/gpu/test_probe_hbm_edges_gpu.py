"""The probe's HBM fill / verify kernels at the sizes where their loops split (run on the GPU box
with ``-m gpu``): one partial block, the unrolled main loop plus a tail chunk, a size that is no
multiple of 16 bytes — for both patterns and both layouts, after a run that left foreign data
behind, with a flipped bit at the first and the last chunk found at its exact offset. Also one
clean-and-faulty pair through each probe option no other test touches.
"""
from __future__ import annotations

import pytest

pytestmark = pytest.mark.gpu

MIB = 1 << 20
SIZES = [
    16 * 100,           # one partial block (n16 < 256): tail loop only, one workgroup
    4 * MIB + 16,       # 256 blocks: the fill's unrolled main loop once, plus one tail chunk
    64 * MIB + 16 * 77,
    64 * MIB + 8,       # no multiple of 16: the last 8 bytes are not tested
]
CONFIGS = [(1, 0), (1, 1), (0, 0)]  # (hbmPattern, hbmLayout); the tiled layout has pattern 1 only


@pytest.fixture(scope="module")
def hip(native_built):
    from gpupool.ops import probe
    n = probe.init()
    assert n >= 1, "no HIP device visible"
    return probe


def _run(hip, nbytes, config, **hooks):
    pattern, layout = config
    return hip.run(0, hbm_bytes=nbytes, mfma=False, patterns=2, hbmPattern=pattern, hbmLayout=layout,
                   **hooks)


def _assert_clean(r, nbytes):
    assert r["passed"] and r["hbm"]["ok"], r
    assert r["hbm"]["badBits"] == 0 and r["hbm"]["firstBadOffset"] is None, r["hbm"]
    assert r["hbm"]["bytes"] == nbytes // 16 * 16 and r["hbm"]["patterns"] == 2, r["hbm"]


def first_flip_offset(nbytes: int, k: int) -> int:
    """Byte offset of the lowest chunk ``injectBitFlips=k`` corrupts: it flips one bit in each of
    the words stride, 2 * stride, .. k * stride, stride = words // (k + 1)."""
    n16 = nbytes // 16
    return 16 * ((n16 * 4 // (k + 1)) // 4)


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: f"pattern{c[0]}-layout{c[1]}")
@pytest.mark.parametrize("nbytes", SIZES)
def test_hbm_clean_at_loop_split_sizes(hip, nbytes, config):
    """Clean at each size; and again after a run of the OTHER pattern at the same size (same
    arena), so a chunk the fill skipped holds foreign data, not the last run's identical pattern."""
    _assert_clean(_run(hip, nbytes, config), nbytes)
    other = (1 - config[0], 0)
    _assert_clean(_run(hip, nbytes, other), nbytes)
    r = _run(hip, nbytes, config)
    assert r["phases"]["arenaReused"], r["phases"]
    _assert_clean(r, nbytes)


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: f"pattern{c[0]}-layout{c[1]}")
@pytest.mark.parametrize("nbytes", SIZES)
def test_hbm_flip_at_first_and_last_chunk_is_found_there(hip, nbytes, config):
    n16 = nbytes // 16
    for chunk in (0, n16 - 1):
        r = _run(hip, nbytes, config, injectFlipAtChunk=chunk)
        assert not r["passed"] and not r["hbm"]["ok"], r
        assert r["hbm"]["badBits"] == 1 and r["hbm"]["firstBadOffset"] == 16 * chunk, (chunk, r["hbm"])
    _assert_clean(_run(hip, nbytes, config, injectFlipAtChunk=n16), nbytes)  # past the end: no flip


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: f"pattern{c[0]}-layout{c[1]}")
@pytest.mark.parametrize("nbytes", SIZES)
def test_hbm_spread_flips_counted_and_first_located(hip, nbytes, config):
    for k in (1, 6, 37):
        r = _run(hip, nbytes, config, injectBitFlips=k)
        assert not r["passed"], r
        assert r["hbm"]["badBits"] == k, (k, r["hbm"])
        assert r["hbm"]["firstBadOffset"] == first_flip_offset(nbytes, k), (k, r["hbm"])
    _assert_clean(_run(hip, nbytes, config), nbytes)


@pytest.mark.parametrize("options", [{"gemmPrio": 1, "gemmPipe": 0}, {"gemmPipe": 22}, {"hbmFirst": 0},
                                     {"hbmFirst": 2}], ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_untouched_probe_options_pass_clean_and_catch_a_fault(hip, options):
    """``gemmPrio`` is an option of the 2-phase loop: it takes effect with ``gemmPipe`` 0 only."""
    kw = dict(hbm_bytes=1 << 20, gemm_n=256, **options)
    clean = hip.run(0, **kw)
    assert clean["passed"], clean
    assert clean["hbm"]["badBits"] == 0
    assert clean["mfma"]["abftMismatches"] == 0 and clean["mfma"]["elementMismatches"] == 0
    assert clean["phases"]["hbmFirst"] == options.get("hbmFirst", 1)
    assert clean["mfma"]["pipe"] == options.get("gemmPipe", 2) and clean["mfma"]["tile"] == 256
    bad = hip.run(0, injectGemmFault=1, **kw)
    assert not bad["passed"] and bad["hbm"]["ok"], bad
    assert bad["mfma"]["abftMismatches"] == 2  # its row and its column checksum
    assert bad["mfma"]["elementMismatches"] == 0
