"""The probe's FP8 / MXFP8 / MXFP4 matrix-core checks on a real MI355X (run with ``-m gpu``).

``lowp_cases`` holds the operands and references. Everything is exact: C must equal the float64
host reference element by element, with C poisoned on host and device before every launch.
The encodings cases pin the OCP e4m3fn bias, the subnormals, 448 and the operand lane / nibble map
of ``v_mfma_f32_16x16x32_fp8_fp8`` and ``v_mfma_scale_f32_16x16x128_f8f6f4``; the exact cases run 1, 2,
3, 5 and 7 K-tiles and non-square grids; the ``probe.run`` cases prove the opt-in phase passes on
good hardware, that its checkers catch an injected fault in the right dtype only, and that a
probe that asks for no dtype reports what it always did.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from . import gemm_cases, lowp_cases

pytestmark = pytest.mark.gpu

DTYPES = lowp_cases.DTYPES
SCALED = ("mxfp8", "mxfp4")
PROBE = dict(hbm_bytes=64 << 20, gemm_n=512)
DEFAULT_KEYS = {"device", "hipUUID", "gcnArch", "passed", "hbm", "mfma", "cus", "ms", "phases", "reportMs"}


@pytest.fixture(scope="module")
def hip(native_built):
    from gpupool.ops import probe
    n = probe.init()
    assert n >= 1, "no HIP device visible"
    return probe


def _check(hip, o):
    c = lowp_cases.run(hip, o)
    v = gemm_cases.check(c, o.data, lowp_cases.TILE)
    assert v.ok, v.message


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_finite_encoding_comes_back_exact(hip, dtype):
    """C[m][n] = +-A[m][perm(n)] over every finite encoding, unit scales."""
    _check(hip, lowp_cases.encodings(dtype))


@pytest.mark.parametrize("dtype", SCALED)
def test_every_finite_encoding_times_its_block_scale(hip, dtype):
    """The same with per-row, per-block A scales spread over 2^-60 .. 2^60."""
    _check(hip, lowp_cases.encodings(dtype, True))


@pytest.mark.parametrize("shape", lowp_cases.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_matches_host_fp64_exactly(hip, dtype, shape):
    _check(hip, lowp_cases.exact(dtype, shape))


@pytest.mark.parametrize("dtype,shape,scales", [
    ("fp8", (128, 128, 64), False),      # k % 128
    ("fp8", (64, 128, 128), False),      # m % 128
    ("mxfp8", (128, 192, 128), True),    # n % 128
    ("mxfp4", (128, 128, 192), True),    # k % 128
    ("mxfp4", (0, 128, 128), True),
    ("fp6", (128, 128, 128), True),      # no such dtype
    ("fp8", (128, 128, 128), True),      # scales passed to fp8
    ("mxfp8", (128, 128, 128), False),   # a scaled dtype without its scales
])
def test_bad_shape_dtype_or_scales_is_refused(hip, dtype, shape, scales):
    m, n, k = shape
    a, bt = np.zeros((max(m, 1), max(k, 1)), dtype=np.uint8), np.zeros((n, max(k, 1)), dtype=np.uint8)
    sa, sb = np.full((max(m, 1), 8), 127, dtype=np.uint8), np.full((n, 8), 127, dtype=np.uint8)
    c = gemm_cases.poisoned_c(max(m, 1), n)
    with pytest.raises(ValueError):
        hip.gemm_lowp(0, dtype, a.ctypes.data, bt.ctypes.data, sa.ctypes.data if scales else None,
                      sb.ctypes.data if scales else None, c.ctypes.data, m, n, k, poison_c=1)
    assert (c.view(np.uint32) == gemm_cases.POISON_BITS).all()


@pytest.mark.parametrize("index", [-1, 3])
def test_unknown_dtype_index_is_refused_by_the_library(hip, index):
    a = np.zeros((128, 128), dtype=np.uint8)
    c = gemm_cases.poisoned_c(128, 128)
    rc = hip.lib().mi355x_probe_gemm_lowp(0, index, a.ctypes.data, a.ctypes.data, None, None, c.ctypes.data,
                                          128, 128, 128, ctypes.c_char_p(None))
    assert rc == -2
    assert (c.view(np.uint32) == gemm_cases.POISON_BITS).all()


def _clean(r, asked):
    assert r["passed"], r
    assert set(r["lowp"]) == set(asked), r["lowp"]
    for name in asked:
        e = r["lowp"][name]
        assert e["ok"] and e["n"] == PROBE["gemm_n"], e
        assert e["elementMismatches"] == 0 and e["abftMismatches"] == 0 and e["badWaves"] == 0, e
        assert e["cusVerified"] == r["cus"]["expected"], (e, r["cus"])
        assert e["tflops"] > 0 and e["ms"] > 0, e
    assert r["mfma"]["elementMismatches"] == 0 and r["mfma"]["abftMismatches"] == 0 and r["cus"]["ok"], r


@pytest.mark.parametrize("asked", [("fp8",), ("mxfp8",), ("mxfp4",), DTYPES], ids="+".join)
def test_probe_passes_with_low_precision_dtypes(hip, asked):
    _clean(hip.run(0, mfma_low_precision=asked, poisonC=1, **PROBE), asked)


@pytest.mark.parametrize("dtype", DTYPES)
def test_injected_fault_fails_that_dtype_only(hip, dtype):
    r = hip.run(0, mfma_low_precision=DTYPES, injectLowpFault=1 << DTYPES.index(dtype), **PROBE)
    assert not r["passed"], r
    for name in DTYPES:
        e = r["lowp"][name]
        assert e["abftMismatches"] == (2 if name == dtype else 0), (name, e)  # one row, one column
        assert e["ok"] == (name != dtype) and e["elementMismatches"] == 0, (name, e)
    assert r["mfma"]["ok"] and r["mfma"]["abftMismatches"] == 0, r["mfma"]
    _clean(hip.run(0, mfma_low_precision=DTYPES, **PROBE), DTYPES)  # the reused arena holds no fault


@pytest.mark.parametrize("dtype", DTYPES)
def test_census_detects_a_bad_xcd_on_that_instruction(hip, dtype):
    r = hip.run(0, mfma_low_precision=(dtype,), injectLowpCensusFaultXcc=3, **PROBE)
    assert not r["passed"], r
    e, cus = r["lowp"][dtype], r["cus"]
    assert e["cusVerified"] == cus["expected"] - cus["expected"] // 8 and e["badWaves"] > 0 and not e["ok"], e
    assert e["abftMismatches"] == 0 and e["elementMismatches"] == 0, e
    assert cus["ok"] and cus["mfmaVerified"] == cus["expected"], cus  # the bf16 census is untouched


def test_default_probe_reports_no_low_precision(hip):
    r = hip.run(0, **PROBE)
    assert r["passed"] and set(r) == DEFAULT_KEYS, sorted(r)
    r = hip.run(0, mfma=False, mfma_low_precision=("fp8",), **PROBE)  # needs the MFMA phase: ignored
    assert r["passed"] and "lowp" not in r, sorted(r)
