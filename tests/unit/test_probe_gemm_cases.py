"""CPU checks that keep the GPU tests of the probe GEMM variants honest (tests/gpu/gemm_cases.py):
the cases reach the K-loop paths they claim, "exact" is a fair demand on the exact data, and the
comparer passes a right C and flags each way a tiled MFMA kernel typically goes wrong."""
from __future__ import annotations

import numpy as np
import pytest

from tests.gpu import gemm_cases as gc

SHAPES = sorted({(c.variant.tile, c.shape) for c in gc.CASES})


def _right_c(d) -> np.ndarray:
    """What a correct kernel returns: the reference rounded to fp32 (exact for ``exact``)."""
    return d.ref.astype(np.float32)


def test_every_variant_and_shape_of_the_issue_is_listed():
    assert [v.name for v in gc.VARIANTS] == ["tile128", "pipe0", "pipe0-prio", "pipe0-vecc", "pipe1",
                                             "pipe2", "pipe21", "pipe22", "pipe3"]
    assert len({c.id for c in gc.CASES}) == len(gc.CASES)
    for v in gc.VARIANTS:
        mine = [c for c in gc.CASES if c.variant == v]
        if v.tile == 128:
            assert {c.shape for c in mine} == set(gc.SHAPES_128)
            assert all(c.group_m is None for c in mine)
            continue
        assert {c.shape for c in mine} == set(gc.SHAPES_256)
        for s in gc.SHAPES_256:
            groups = {c.group_m for c in mine if c.shape == s}
            assert groups == (set(gc.GROUPS) if s in gc.GROUPED_SHAPES else {None})
    assert {(1280, 768, 192), (512, 1536, 448)} == set(gc.GROUPED_SHAPES)
    assert set(gc.GROUPS) == {0, 2, 3, 4, 8}
    assert {v.name for v in gc.VARIANTS if v.pipelined} == {"pipe1", "pipe2", "pipe21", "pipe22", "pipe3"}


def test_shapes_satisfy_their_tile_and_cover_the_k_tile_counts():
    for c in gc.CASES:
        m, n, k = c.shape
        v = c.variant
        assert (v.tile, v.bk) in ((256, 64), (128, 32))
        assert m % v.tile == 0 and n % v.tile == 0 and k % v.bk == 0, c.id
        assert k <= 448  # the exactness argument of the exact data
    for tile, bk in ((256, 64), (128, 32)):
        counts = {s[2] // bk for t, s in SHAPES if t == tile}
        assert {1, 2, 3} <= counts, (tile, counts)
        assert any(x >= 5 and x % 2 for x in counts), (tile, counts)
    # non-square grids; one with a short last group whose workgroup count is no multiple of 8
    grids = {(s[0] // 256, s[1] // 256) for t, s in SHAPES if t == 256}
    assert (5, 3) in grids and (2, 6) in grids and (3, 1) in grids


def test_bf16_round_trip_helpers():
    x = np.array([0.0, 1.0, -1.0, 127.0, -127.0, 0.5, 3.140625, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8],
                 dtype=np.float32)
    bits = gc.bf16_bits(x)
    back = gc.bf16_value(bits)
    assert back[:7].tolist() == x[:7].tolist()        # exact in bf16
    assert back[7] == 1.0                             # tie: to even (down)
    assert back[8] == np.float32(1.0 + 2.0 ** -6)     # tie: to even (up)
    assert bits[1] == 0x3F80 and bits[2] == 0xBF80


@pytest.mark.parametrize("tile,shape", SHAPES, ids=lambda x: str(x))
def test_exact_data_makes_exact_a_fair_demand(tile, shape):
    d = gc.data(shape, "exact")
    for bits in (d.a, d.bt):
        v = gc.bf16_value(bits)
        assert (v == np.rint(v)).all() and np.abs(v).max() <= 127
        assert (gc.bf16_bits(v) == bits).all()        # survives a bf16 round trip unchanged
        assert len(np.unique(v)) > 200                # really draws from [-127, 127]
    assert np.abs(d.ref).max() < 2 ** 24
    assert shape[2] * 127 * 127 < 2 ** 24             # so is every partial sum, in any order
    assert (d.ref == np.rint(d.ref)).all()
    assert (_right_c(d).astype(np.float64) == d.ref).all()
    assert d.bound is None


@pytest.mark.parametrize("tile,shape", SHAPES, ids=lambda x: str(x))
def test_rounding_data_and_its_bound(tile, shape):
    d = gc.data(shape, "rounding")
    a = gc.bf16_value(d.a)
    assert (gc.bf16_bits(a) == d.a).all() and not (a == np.rint(a)).all()
    assert d.bound.shape == d.ref.shape and (d.bound > 0).all()
    # the bound is the derived one, and far below the data's scale: a wrong element cannot hide
    k = shape[2]
    r, q = 3, 5
    want = k * 2.0 ** -23 * float(np.abs(a[r].astype(np.float64)) @ np.abs(gc.bf16_value(d.bt[q]).astype(np.float64)))
    assert d.bound[r, q] == pytest.approx(want, rel=1e-12)
    assert d.bound.max() < 1e-2 * np.abs(d.ref).std()
    assert gc.data(shape, "rounding") is d            # computed once, shared
    with pytest.raises(ValueError):
        d.ref[0, 0] = 1.0                             # and left unchanged


@pytest.mark.parametrize("kind", gc.KINDS)
@pytest.mark.parametrize("tile,shape", SHAPES, ids=lambda x: str(x))
def test_comparer_passes_a_right_c(tile, shape, kind):
    d = gc.data(shape, kind)
    v = gc.check(_right_c(d), d, tile)
    assert v.ok and v.message == "", v.message
    assert v.max_ratio <= (0.0 if kind == "exact" else 1.0)


def _mutations(d, tile):
    """(name, wrong C, elements that must be flagged at least) for each typical fault."""
    m, n, k = d.shape
    good = _right_c(d)
    tm, tn = (m // tile) - 1, (n // tile) - 1       # the last tile: any tile must be caught
    r0, q0 = tm * tile, tn * tile
    a64, bt64 = gc.bf16_value(d.a).astype(np.float64), gc.bf16_value(d.bt).astype(np.float64)

    c = good.copy()
    c[r0 + 17, q0 + 33] = np.nextafter(c[r0 + 17, q0 + 33], np.float32(np.inf))
    if d.kind == "exact":
        yield "one element off by one fp32 ulp", c, 1

    c = good.copy()
    c[[r0 + 4, r0 + 5], q0:q0 + tile] = c[[r0 + 5, r0 + 4], q0:q0 + tile]
    yield "two rows of one tile swapped", c, tile

    bk = 64 if k >= 64 else k                        # one 64-wide K-tile (all of K if K is 32)
    k0 = ((k // bk) - 1) * bk
    c = (d.ref - a64[:, k0:k0 + bk] @ bt64[:, k0:k0 + bk].T).astype(np.float32)
    yield "one K-tile left out of the product", c, m * n // 2

    c = good.copy()
    c[r0 + 16:r0 + 32, q0 + 48:q0 + 64] = c[r0 + 16:r0 + 32, q0 + 48:q0 + 64].T.copy()
    yield "one 16x16 sub-tile transposed", c, 16 * 15 // 2

    c = good.copy()
    c[r0:r0 + tile, q0:q0 + tile] = gc.poisoned_c(tile, tile)
    yield "one tile left as poison", c, tile * tile


@pytest.mark.parametrize("kind", gc.KINDS)
@pytest.mark.parametrize("tile,shape", SHAPES, ids=lambda x: str(x))
def test_comparer_flags_every_mutation(tile, shape, kind):
    d = gc.data(shape, kind)
    names = []
    for name, c, at_least in _mutations(d, tile):
        names.append(name)
        v = gc.check(c, d, tile)
        assert not v.ok, f"{name} passed the comparer"
        count = int(v.message.split(": ")[1].split(" of ")[0])
        assert count >= at_least, (name, v.message)
        m, n, _ = shape
        last = (m // tile - 1, n // tile - 1)
        if name == "one tile left as poison":
            assert count == tile * tile and "all of them the poison" in v.message, v.message
            assert f"in 1 tile(s) [{last}]" in v.message, v.message
            assert f"[({last[0]}, {last[1]}, 0, 0), ({last[0]}, {last[1]}, 0, 1)" in v.message
        elif name == "one element off by one fp32 ulp":
            assert count == 1 and "none of them the poison" in v.message, v.message
            assert f"[({last[0]}, {last[1]}, 17, 33)]" in v.message, v.message
        elif name != "one K-tile left out of the product":
            assert "none of them the poison" in v.message and f"[{last}]" in v.message, v.message
    assert len(names) == (5 if kind == "exact" else 4)


def test_comparer_reports_a_mix_of_poison_and_wrong_values():
    d = gc.data((256, 256, 64), "exact")
    c = _right_c(d).copy()
    c[0:2, 0:4] = gc.poisoned_c(2, 4)
    c[200, 100] += 1.0
    v = gc.check(c, d, 256)
    assert not v.ok
    assert "9 of 65536 elements wrong, 8 of them the poison (never written), 1 written wrong" in v.message
    assert "8 not finite" in v.message
    inf = _right_c(d).copy()
    inf[7, 7] = np.inf
    assert not gc.check(inf, d, 256).ok
    dr = gc.data((256, 256, 64), "rounding")
    inf = _right_c(dr).copy()
    inf[7, 7] = np.inf
    v = gc.check(inf, dr, 256)
    assert not v.ok and "1 not finite" in v.message
