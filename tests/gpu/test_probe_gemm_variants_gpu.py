"""Every GEMM variant of the probe against a host float64 reference, at the small, odd and
non-square shapes the N^3 probe never reaches (run on the GPU box with ``-m gpu``).

``gemm_cases`` holds the cases, the operands and the comparer; ``tests/unit/
test_probe_gemm_cases.py`` proves on the CPU that the comparer catches a kernel's typical faults.
Each variant runs 1, 2, 3, 5 and 7 K-tiles (prologue, last-tile and odd-parity buffer paths),
non-square tile grids whose workgroup count is no multiple of the 8 XCDs, and the grouped tile
order with a short last group — element by element: bit-exact on integer operands (any partial
sum is exact in fp32) and inside a derived per-element bound on normal ones. C is poisoned on the
host and on the device before every launch, so an unwritten tile cannot pass on a stale result.
"""
from __future__ import annotations

import numpy as np
import pytest

from . import gemm_cases

pytestmark = pytest.mark.gpu

PIPELINED_RUNS = 4  # a read placed before its DMA has landed shows in some runs and not others


@pytest.fixture(scope="module")
def hip(native_built):
    from gpupool.ops import probe
    n = probe.init()
    assert n >= 1, "no HIP device visible"
    return probe


def _run(hip, d, **opts):
    m, n, k = d.shape
    c = gemm_cases.poisoned_c(m, n)
    hip.gemm_bf16(0, d.a.ctypes.data, d.bt.ctypes.data, c.ctypes.data, m, n, k, **opts)
    return c


@pytest.mark.parametrize("kind", gemm_cases.KINDS)
@pytest.mark.parametrize("case", gemm_cases.CASES, ids=lambda c: c.id)
def test_gemm_variant_matches_host_fp64(hip, case, kind):
    """``exact``: C == ref for every element, no tolerance. ``rounding``: C all finite and
    |C - ref| <= K * 2^-23 * (|A| @ |Bt|^T) for every element (see gemm_cases). The pipelined
    K-loops run four times, C poisoned again each time."""
    d = gemm_cases.data(case.shape, kind)
    for run in range(PIPELINED_RUNS if case.variant.pipelined else 1):
        c = _run(hip, d, poison_c=1, **case.opts)
        v = gemm_cases.check(c, d, case.variant.tile)
        print(f"gemm-ratio {case.variant.name} {case.id} {kind} run {run}: "
              f"max |C - ref| / bound = {v.max_ratio:.4g}")
        assert v.ok, f"{case.id} run {run}: {v.message}"


def test_default_options_written_out_give_the_same_bits(hip):
    """``gemm_bf16`` without options is the same launch as the defaults written out: one dispatch,
    one set of defaults (the claim-time probe's)."""
    d = gemm_cases.data((512, 1536, 448), "rounding")
    plain = _run(hip, d)
    spelled = _run(hip, d, gemm_tile=256, gemm_pipe=2, gemm_prio=0, gemm_vec_c=0, gemm_group_m=4,
                   poison_c=0)
    assert gemm_cases.check(plain, d, 256).ok
    assert np.array_equal(plain.view(np.uint32), spelled.view(np.uint32))


@pytest.mark.parametrize("shape,opts", [
    ((256, 256, 32), dict(gemm_tile=256)),    # k fits the 128 kernel only
    ((128, 256, 64), dict(gemm_tile=256)),    # m fits the 128 kernel only
    ((256, 384, 64), dict(gemm_pipe=3)),      # n
    ((128, 128, 48), dict(gemm_tile=128)),    # k % 32
    ((128, 192, 32), dict(gemm_tile=128)),    # n % 128
    ((256, 256, 64), dict(gemm_tile=64)),     # no such tile
    ((256, 256, 64), dict(gemm_pipe=11)),     # timing-only ablation: wrong C by design
    ((256, 256, 64), dict(gemm_pipe=12)),
    ((256, 256, 64), dict(gemm_pipe=7)),      # no such K-loop
])
def test_bad_tile_shape_or_pipe_is_refused(hip, shape, opts):
    m, n, k = shape
    a = np.zeros((m, k), dtype=np.uint16)
    bt = np.zeros((n, k), dtype=np.uint16)
    c = gemm_cases.poisoned_c(m, n)
    with pytest.raises(ValueError):
        hip.gemm_bf16(0, a.ctypes.data, bt.ctypes.data, c.ctypes.data, m, n, k, **opts)
    assert (c.view(np.uint32) == gemm_cases.POISON_BITS).all()  # refused before anything ran
