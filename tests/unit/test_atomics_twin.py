"""The twin of the probe's atomic-unit phase (gpupool/ops/atomics.py): pinned to the table the native
reference is pinned to, its finals independent of the order the atomics arrive in, every lost workgroup
visible in the dev rows, and the exactness bound of the floating-point rows."""
from __future__ import annotations

import random

import numpy as np
import pytest

from gpupool.ops import atomics as tw

SEED = tw.SEED_BASE + 1
# native/tests/test_atomics_spec.cc quotes the same 48 words: per seed and step count the digests of the lds
# region, its return digests, the l2 region, its return digests, the dev rows of 3 workgroups on XCDs 0, 1, 0
# and the lds layer's second addressing; 64 steps reach the packed rows' limit of 256
PINNED = {
    (SEED, 1): [0xc28da422, 0xeba259fd, 0x372ebeb3, 0x4550707f, 0xd9db3aa6, 0x01fe68d2],
    (SEED, 2): [0xb9fa6f41, 0x15987d4e, 0x43250b05, 0xf7ee838b, 0x0d11cf6b, 0xd561b263],
    (SEED, 3): [0x3d287087, 0xa98c0d33, 0x5f742a88, 0xe30c5932, 0x91d24352, 0x7047aeb5],
    (SEED, 64): [0x9318c9f7, 0x0c7a97c4, 0x14de922f, 0x7083aec3, 0xfc5975c4, 0x211b5da0],
    (12345, 1): [0x741c5e04, 0x7011b87b, 0x41e3f4d7, 0xa12a9381, 0x7cd52cae, 0xba8a670e],
    (12345, 2): [0x3c50af5e, 0xc0ee6937, 0x1a6fc171, 0xc6e58e7c, 0xadd15f39, 0x0fa818b3],
    (12345, 3): [0xd95975f1, 0xbd865dff, 0x5ea558b1, 0x5a78fc64, 0xd8d94199, 0x9a69ef0a],
    (12345, 64): [0x5ed99ee4, 0x20f54654, 0x3f0828e1, 0xea2568b8, 0x7f4c3ffb, 0x3b160526],
}


@pytest.mark.parametrize("seed,iters", sorted(PINNED))
def test_the_twin_equals_the_pinned_table(seed, iters):
    assert tw.pinned(seed, iters) == PINNED[seed, iters]


def test_layout_and_operand_streams():
    assert (tw.ROWSET_WORDS, tw.REGION_WORDS, tw.DUMP_WORDS, tw.DUMP_BYTES) == (1408, 2688, 24064, 96256)
    assert len(tw.OPS) == 24 and tw.OPS[tw.CAS] == "cas" and tw.OPS[tw.TICKET] == "ticket" and tw.OPS[tw.RETURNS] == "returns"
    assert tw.fold(0, 1) == 0x9E3779B1
    streams = {tw.raw(layer, op, 0, 0, 0, 5) for layer in range(3) for op in range(22)}
    assert len(streams) == 66 and tw.raw(3, 0, 0, 0, 0, 5) not in streams  # no two (layer, op) pairs share an operand stream
    assert tw.int_to_fp(256, 7, 127) == 0x4380 and tw.int_to_fp(3, 23, 127) == 0x40400000
    assert tw.int_to_fp(2048, 10, 15) == 0x6800 and tw.int_to_fp(5, 52, 1023) == 0x4014000000000000
    with pytest.raises(AssertionError):
        tw.int_to_fp(257, 7, 127)  # not a bf16 number: the plan must never get there


@pytest.mark.parametrize("iters", [1, 2, 3])
def test_finals_do_not_depend_on_the_arrival_order(iters):
    wg_xcc = [0, 1]
    e = tw.expected(SEED, iters, 2, wg_xcc)
    for order in range(3):
        s = tw.simulate(SEED, iters, wg_xcc, random.Random(1000 * iters + order))
        for b in range(2):
            assert (s["lds"][b] == e["lds"][:tw.ROWSET_WORDS]).all()
            assert (s["l2"][b] == e["l2"][:tw.ROWSET_WORDS]).all()
        assert (s["dev"] == e["dev"]).all()


def test_float_rows_stay_exact_at_the_extreme_plan():
    # 16 x 256 workgroups, 64 steps, 4 waves, the largest operand of each row
    n = 16 * 256 * 64 * 4
    assert 3 * n < 1 << 24 and 7 * n < 1 << 53
    assert 64 * 4 <= 256  # lds, l2: one bit per half from every wave and step, exact in bf16 (and f16 <= 2048)
    assert sum(tw.issues(tw.DEV, 11, t, w, b) for b in range(16 * 256) for t in range(64) for w in range(4)) == 256
    assert max(tw.operand(tw.DEV, 9, w) for w in range(8)) == 3 and max(tw.operand(tw.L2, 15, w) for w in range(16)) == 7
    # the hardware's own arithmetic reaches the integer sums: 256 ones in bf16, 2048 in f16
    v = 0
    for _ in range(256):
        v = tw._hw_apply(11, v, 3)
    assert v == 0x43804380
    v = 0
    for _ in range(256):
        v = tw._hw_apply(10, v, 1)
    assert v == tw.int_to_fp(256, 10, 15)


def test_every_lost_workgroup_changes_a_dev_slot():
    wg_xcc = [0, 1, 0, 3, 1, 0]
    full = tw.dev_rows(SEED, 2, wg_xcc)
    for lost in range(len(wg_xcc)):
        # the rows as they end up when workgroup ``lost`` contributes nothing: it is struck by a hook that
        # skips everything, modelled by taking it out of the population while the others keep their index
        class Gone(tw._Hook):
            def skips(self, layer, op, step, wave, lane):
                return True
        hook, none = Gone(), tw._Hook()
        rows = np.zeros_like(full)
        for op in range(tw.N_CONTENDED):
            for lane in range(tw.LANES):
                for s in range(tw.DEV_ROWSETS):
                    slot = tw._Slot(op)
                    for b, x in enumerate(wg_xcc):
                        if s != tw.ALL_XCD and x != s:
                            continue
                        for a in tw._dev_contribution(op, lane, SEED, 2, hook if b == lost else none, b):
                            slot.apply(a)
                    tw._put(rows[s], op, lane, slot.bits())
        changed = {s for s in range(tw.DEV_ROWSETS) if (rows[s] != full[s]).any()}
        assert changed == {wg_xcc[lost], tw.ALL_XCD}
        for s in changed:  # every linear row sees it: add, sub, or, and, add_f32, add_x2, add_f64
            for op in (0, 1, 2, 3, 9, 12, 15):
                w0 = tw.row_word(op)
                w1 = w0 + (128 if tw.wide(op) else 64)
                assert (rows[s][w0:w1] != full[s][w0:w1]).any(), (lost, s, tw.OPS[op])


def test_single_hooks_and_the_prediction():
    wg_xcc = [0, 1, 0, 2]
    # a skipped add in every workgroup: one lds slot per workgroup, nothing else
    p = tw.predict(SEED, 2, wg_xcc, skip=(tw.LDS, 0, 1, 31))
    assert p["ldsBadSlots"] == 4 and p["badWorkgroups"] == 4 and p["l2BadSlots"] == p["devBadSlots"] == p["badReturns"] == 0
    assert (p["firstBadLayer"], p["firstBadOp"], p["firstBadSlot"], p["firstBadXcc"]) == ("lds", "add", 31, 0)
    # on one XCD only: its own row and the all-XCD row
    p = tw.predict(SEED, 2, wg_xcc, flip=(tw.DEV, 4, 0, 63, 0), xcc=1)
    assert p["devBadSlots"] == 2 and p["badWorkgroups"] == 0
    assert (p["firstBadLayer"], p["firstBadOp"], p["firstBadSlot"], p["firstBadXcc"]) == ("dev", "xor", 63, 1)
    # two workgroups flipping the same xor bit cancel in their rows
    p = tw.predict(SEED, 2, wg_xcc, flip=(tw.DEV, 4, 0, 63, 0), xcc=0)
    assert p["devBadSlots"] == 0 and p["firstBadLayer"] is None
    # a flipped cas value: the next step's cas fails, the digest and the word are off
    p = tw.predict(SEED, 2, wg_xcc, flip=(tw.L2, tw.CAS, 0, 5, 31), workgroup=3)
    assert p["l2BadSlots"] == 1 and p["badReturns"] == 1 and p["badWorkgroups"] == 1
    assert (p["firstBadLayer"], p["firstBadOp"], p["firstBadSlot"], p["firstBadXcc"]) == ("l2", "cas", 5, 2)
    p = tw.predict(SEED, 1, wg_xcc, skip=(tw.LDS, tw.TICKET, 0, 9), xcc=0)
    assert p["ticketFaults"] == 2 and p["firstBadOp"] == "ticket"
    # layers not run report nothing
    assert tw.predict(SEED, 2, wg_xcc, layers=6, skip=(tw.LDS, 0, 1, 31))["ldsBadSlots"] == 0


def test_decisive_helpers():
    for layer in (tw.LDS, tw.L2, tw.LDS16):
        # add xor or umin add_x2 add_f32 pk_add_bf16; in the second addressing 32 operands meet in a slot and
        # saturate or (every bit set) and umin, so there only the linear ops have a decisive hook
        for op in (0, 4, 3, 5, 12, 9, 11) if layer != tw.LDS16 else (0, 4, 12, 9, 11):
            d = tw.decisive(layer, op, SEED, 2)
            assert d is not None and tw.decisive(layer, op, SEED, 2, skip=True) is not None, (layer, tw.OPS[op])
            t, lane, bit = d
            if layer == tw.LDS16:
                clean, hit = tw.lds16(SEED, 2), tw.lds16(SEED, 2, flip=(layer, op, t, lane, bit))
            else:
                clean, hit = tw.region(layer, SEED, 2)[0], tw.region(layer, SEED, 2, flip=(layer, op, t, lane, bit))[0]
            assert (clean != hit).sum() in (1, 2)  # one slot, 4 or 8 bytes
    for op in (20, 21):  # swap, cas: the digest or the word
        assert tw.decisive(tw.L2, op, SEED, 2) is not None and tw.decisive(tw.LDS, op, SEED, 2, skip=True) is not None
    wg_xcc = [b % 8 for b in range(64)]
    # dev: or / and arrive once per workgroup, in the lane that holds its bit
    assert tw.decisive(tw.DEV, 3, SEED, 2, wg_xcc, skip=True, workgroup=37) == (0, 1)
    assert tw.decisive(tw.DEV, 3, SEED, 2, wg_xcc, skip=True, prefer=31) == (0, 0)
    assert tw.decisive(tw.DEV, 0, SEED, 1, [0]) is not None


@pytest.mark.parametrize("op", [5, 6, 7, 8, 13, 16])  # umin umax smin smax umax_x2 max_f64
def test_the_deciding_workgroup_of_a_dev_min_max_slot(op):
    wg_xcc = [b % 8 for b in range(64)]
    full = tw.dev_rows(SEED, 2, wg_xcc, only_op=op)
    named = 0
    for lane in (0, 31, 32, 63):
        for s, pop in ((tw.ALL_XCD, range(64)), (3, [b for b in range(64) if b % 8 == 3])):
            w = tw.decisive_workgroup(op, lane, SEED, 2, pop)
            # losing one arrival of one workgroup changes the slot exactly when it is the one the twin names
            for b in list(pop)[:6] + ([w] if w is not None else []):
                rows = tw.dev_rows(SEED, 2, wg_xcc, [b], skip=(tw.DEV, op, 0, lane), only_op=op)
                i = tw.row_word(op) + (2 * lane if tw.wide(op) else lane)
                changed = bool((rows[s][i:i + 2] != full[s][i:i + 2]).any()) if tw.wide(op) else bool(rows[s][i] != full[s][i])
                assert changed == (b == w), (tw.OPS[op], lane, s, b, w)
            named += w is not None
        assert tw.decisive_workgroup(op, lane, SEED, 2, []) is None
    assert named >= 4  # with 8 or 64 own operands against 7 shared ones, a workgroup decides most slots
