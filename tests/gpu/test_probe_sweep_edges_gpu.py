"""The rotating HBM sweep's window arithmetic on a real MI355X (run with ``-m gpu``): windows of
2-4 MiB placed where the arithmetic can go wrong — inside one 1 GiB chunk of the sweep buffer,
across a chunk seam, ending or starting exactly on one, clipped at the end of the span, wrapped
past it, and reaching into the last chunk, which is shorter than the others — each with one bit
flipped at a chunk counted from the window's start (``injectFlipAtChunk``): the first and the last
chunk of the window and the chunks on either side of the seam. Every flip must be counted once and
reported at its absolute byte offset in the buffer; all comparisons are exact.

One small buffer (all but 16 GiB of the device stays reserved) serves the whole module.
"""
from __future__ import annotations

import pytest

pytestmark = pytest.mark.gpu

MIB = 1 << 20
GIB = 1 << 30
SHAPES = ["inside_chunk_0", "straddles_first_seam", "ends_on_seam", "starts_on_seam", "clipped_at_span_end",
          "wrapped_past_span", "into_last_chunk", "unaligned_request"]


@pytest.fixture(scope="module")
def hip(native_built):
    from gpupool.ops import probe
    n = probe.init()
    assert n >= 1, "no HIP device visible"
    return probe


@pytest.fixture(scope="module")
def span(hip):
    """The span of the module's sweep buffer, held (``keep``) until the module is done."""
    reserve = int(hip.identify(0)["totalMem"]) - (16 << 30)
    try:
        first = hip.hbm_sweep(0, 0, 2 * MIB, reserve=reserve, keep=True)
        assert first["passed"] is True and first["offset"] == 0 and first["bytes"] == 2 * MIB, first
        yield int(first["span"])
    finally:
        hip.sweep_release(0)


def _need_two_seams(span: int) -> None:
    """The cases need two chunk seams inside the buffer: a smaller span fails the test (no skip)."""
    assert span >= 2 * GIB + 4 * MIB, f"sweep span {span} is below 2 GiB + 4 MiB: no room for the seam cases"
    assert span % (2 * MIB) == 0, span


def _shape(name: str, span: int):
    """-> (offset asked, bytes asked, offset tested, bytes tested, the window's first 16-byte chunk
    behind a seam or None)."""
    _need_two_seams(span)
    chunks = -(-span // GIB)
    last = span - (chunks - 1) * GIB  # what the last chunk holds
    assert 0 < last <= GIB and last % (2 * MIB) == 0
    return {
        "inside_chunk_0": (512 * MIB, 2 * MIB, 512 * MIB, 2 * MIB, None),
        "straddles_first_seam": (GIB - MIB, 2 * MIB, GIB - MIB, 2 * MIB, MIB // 16),
        "ends_on_seam": (GIB - 2 * MIB, 2 * MIB, GIB - 2 * MIB, 2 * MIB, None),
        "starts_on_seam": (GIB, 2 * MIB, GIB, 2 * MIB, None),
        "clipped_at_span_end": (span - MIB, 4 * MIB, span - MIB, MIB, None),
        "wrapped_past_span": (span + GIB - MIB, 2 * MIB, GIB - MIB, 2 * MIB, MIB // 16),
        # one MiB of the last full chunk, then two of the last one (short unless the span is whole GiBs)
        "into_last_chunk": ((chunks - 1) * GIB - MIB, 3 * MIB, (chunks - 1) * GIB - MIB, 3 * MIB, MIB // 16),
        "unaligned_request": (2 * GIB - MIB + 9, 2 * MIB + 5, 2 * GIB - MIB, 2 * MIB, MIB // 16),
    }[name]


def first_flip_offset(nbytes: int, k: int) -> int:
    """Byte offset of the lowest chunk ``injectBitFlips=k`` corrupts in a region of ``nbytes`` (the
    formula of test_probe_hbm_edges_gpu.py)."""
    n16 = nbytes // 16
    return 16 * ((n16 * 4 // (k + 1)) // 4)


def _sweep(hip, offset, nbytes, **hooks):
    return hip.hbm_sweep(0, offset, nbytes, keep=True, **hooks)


def _assert_clean(r, span, offset, nbytes):
    assert r["passed"] is True and r["badBits"] == 0 and r["firstBadOffset"] is None, r
    assert r["offset"] == offset and r["bytes"] == nbytes and r["span"] == span, (r, offset, nbytes)


@pytest.mark.parametrize("name", SHAPES)
def test_window_is_placed_and_a_flip_is_found_at_its_absolute_offset(hip, span, name):
    ask_offset, ask_bytes, offset, nbytes, seam = _shape(name, span)
    _assert_clean(_sweep(hip, ask_offset, ask_bytes), span, offset, nbytes)
    n16 = nbytes // 16
    where = [0, n16 - 1] + ([seam - 1, seam] if seam is not None else [])
    for chunk in sorted(set(where)):
        r = _sweep(hip, ask_offset, ask_bytes, injectFlipAtChunk=chunk)
        assert r["passed"] is False and r["badBits"] == 1, (name, chunk, r)
        assert r["firstBadOffset"] == offset + 16 * chunk, (name, chunk, r)
        assert r["offset"] == offset and r["bytes"] == nbytes, (name, chunk, r)
    for past in (n16, n16 + 1, 1 << 40):  # past the window: no flip
        _assert_clean(_sweep(hip, ask_offset, ask_bytes, injectFlipAtChunk=past), span, offset, nbytes)
    _assert_clean(_sweep(hip, ask_offset, ask_bytes), span, offset, nbytes)


def test_two_flips_on_either_side_of_a_seam_are_both_counted(hip, span):
    """The pieces' counters add up and the lowest offset wins across pieces: one flip behind the
    seam together with spread flips ahead of it."""
    _need_two_seams(span)
    offset, seam = GIB - MIB, MIB // 16
    r = _sweep(hip, offset, 2 * MIB, injectFlipAtChunk=seam + 5, injectBitFlips=6)
    # injectBitFlips spreads over the window's first piece (1 MiB here), as it always did
    assert r["passed"] is False and r["badBits"] == 7, r
    assert r["firstBadOffset"] == offset + first_flip_offset(MIB, 6), r
    _assert_clean(_sweep(hip, offset, 2 * MIB), span, offset, 2 * MIB)


@pytest.mark.parametrize("k", [1, 6, 37])
def test_spread_flips_land_in_the_first_piece(hip, span, k):
    _need_two_seams(span)
    offset = GIB - MIB
    r = _sweep(hip, offset, 2 * MIB, injectBitFlips=k)
    assert r["passed"] is False and r["badBits"] == k, r
    assert r["firstBadOffset"] == offset + first_flip_offset(MIB, k), r
    r = _sweep(hip, 512 * MIB, 2 * MIB, injectBitFlips=k)  # one piece: the whole window
    assert r["badBits"] == k and r["firstBadOffset"] == 512 * MIB + first_flip_offset(2 * MIB, k), r
