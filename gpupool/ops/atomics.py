"""Twin of the probe's atomic-unit phase (native/src/probe/atomics.h): what every slot must hold and
what every returning atomic must return, in Python integers, written from the phase's description
and independent of native/src/probe/atomics_ref.h. Both are pinned to one table of digests
(tests/unit/test_atomics_twin.py, native/tests/test_atomics_spec.cc).

Layout. A row-set is one row of 64 slots per contended op, ops 0..11 with 4-byte slots and 12..16 with
8-byte slots: 1408 words. A region (the LDS table of a workgroup, its private global region) is a
row-set followed by the private words [5 returning ops][4 waves][64 lanes]: 2688 words. The dev
layer has nine row-sets: 0..7 hit by the workgroups of that XCD, 8 by every workgroup.

``simulate`` applies every atomic of a run one at a time in a random arrival order with the
hardware's own arithmetic (numpy float32 / float16, bf16 rounded to nearest even): the finals it
reaches must not depend on the order, and must equal ``expected``.
"""
from __future__ import annotations

import functools
import random

import numpy as np

LANES, WAVES = 64, 4
LAYERS = ("lds", "l2", "dev")
LDS, L2, DEV = 0, 1, 2
LDS16, SLOTS16, PACKED_STEPS16 = 3, 16, 16  # a hook's layer 3: the lds layer's second addressing, slot = lane & 15
OPS = ("add", "sub", "and", "or", "xor", "umin", "umax", "smin", "smax", "add_f32", "pk_add_f16",
       "pk_add_bf16", "add_x2", "umax_x2", "xor_x2", "add_f64", "max_f64", "add_rtn", "inc", "dec",
       "swap", "cas", "ticket", "returns")
N_CONTENDED, N_NARROW, FIRST_RET, CAS, TICKET, RETURNS = 17, 12, 17, 21, 22, 23
ROWSET_WORDS = N_NARROW * LANES + (N_CONTENDED - N_NARROW) * 2 * LANES  # 1408
PRIV_WORDS = 5 * WAVES * LANES  # 1280
REGION_WORDS = ROWSET_WORDS + PRIV_WORDS  # 2688
DEV_ROWSETS, ALL_XCD = 9, 8
PACKED_WORKGROUPS = 256  # dev: only workgroups below it add to the packed rows, wave 0, step 0
MAX_RECORDS = 4096
# the dump of mi355x_probe_atomics, in words
DUMP_LDS, DUMP_LDS_DIGEST = 0, REGION_WORDS
DUMP_L2_DIGEST = DUMP_LDS_DIGEST + WAVES * LANES
DUMP_REGION = DUMP_L2_DIGEST + WAVES * LANES
DUMP_DEV = DUMP_REGION + REGION_WORDS
DUMP_RECORDS = DUMP_DEV + DEV_ROWSETS * ROWSET_WORDS  # each workgroup's CU key (its XCD: key >> 8)
DUMP_LDS16 = DUMP_RECORDS + MAX_RECORDS  # the second addressing's LDS row-set
DUMP_WORDS = DUMP_LDS16 + ROWSET_WORDS
DUMP_BYTES = 4 * DUMP_WORDS
SEED_BASE = 0x41544D00
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def mix(idx: int, seed: int) -> int:
    """hbm.h's pattern_word."""
    x = ((idx & M32) * 0x9E3779B1 ^ (idx >> 32) * 0x85EBCA77) & M32
    x ^= seed
    x ^= x >> 15
    x = x * 0x2C1B3C6D & M32
    x ^= x >> 12
    return x


def fold(h: int, r: int) -> int:
    return (((h << 5 | h >> 27) & M32) ^ r) * 0x9E3779B1 & M32


def wide(op: int) -> bool:
    return N_NARROW <= op < N_CONTENDED


def identity(op: int) -> int:
    return {2: M32, 5: M32, 7: 0x7FFFFFFF, 8: 0x80000000}.get(op, 0)


def row_word(op: int) -> int:
    return op * LANES if op < N_NARROW else N_NARROW * LANES + (op - N_NARROW) * 2 * LANES


def priv_word(op: int, wave: int, lane: int) -> int:
    return ROWSET_WORDS + ((op - FIRST_RET) * WAVES + wave) * LANES + lane


def raw(layer: int, op: int, step: int, wave: int, lane: int, seed: int) -> int:
    def word(part):
        return mix(layer << 40 | op << 32 | step << 10 | part << 8 | wave << 6 | lane, seed)
    return word(1) << 32 | word(0) if wide(op) else word(0)


def rotl13(w: int) -> int:
    return (w << 13 | w >> 19) & M32


def operand(layer: int, op: int, w: int) -> int:
    """The raw integer (a flip already made) as the op's operand; small integers for the floats."""
    w32 = w & M32
    name = OPS[op]
    if name == "and":
        return w32 if layer == DEV else w32 | rotl13(w32)
    if name == "or":
        return w32 if layer == DEV else w32 & rotl13(w32)
    if name in ("add_f32", "pk_add_f16", "pk_add_bf16"):
        return w32 & 3
    if name == "add_f64":
        return w & 7
    if name == "max_f64":
        return w & 0xFFFFF
    if name in ("inc", "dec"):
        return w32 & 7
    return w if wide(op) else w32


def dev_bit(op: int, b: int, lane: int) -> int:
    bit = 1 << (b & 31) if lane == (b >> 5) & 63 else 0
    return bit ^ M32 if OPS[op] == "and" else bit


def issues(layer: int, op: int, step: int, wave: int, b: int) -> bool:
    packed = OPS[op] in ("pk_add_f16", "pk_add_bf16")
    if layer == DEV and (packed or OPS[op] in ("and", "or")):  # one arrival per workgroup
        return wave == 0 and step == 0 and (not packed or b < PACKED_WORKGROUPS)
    if layer == LDS16 and packed:
        return step < PACKED_STEPS16
    return True


def _signed(v: int) -> int:
    return v - (1 << 32) if v & 0x80000000 else v


def int_to_fp(n: int, mant: int, bias: int) -> int:
    """A non-negative integer, exactly representable, as that binary format's bits."""
    if n == 0:
        return 0
    e = n.bit_length() - 1
    assert n == (n >> max(0, e - mant)) << max(0, e - mant), "not representable"
    m = n << (mant - e) if e <= mant else n >> (e - mant)
    return (e + bias) << mant | (m & ((1 << mant) - 1))


class _Hook:
    """injectAtomSkip / injectAtomFlip as the kernel applies them: on wave 0."""

    def __init__(self, skip=None, flip=None):
        self.skip = tuple(skip) if skip else None
        self.flip = tuple(flip) if flip else None

    def skips(self, layer, op, step, wave, lane):
        s = self.skip
        return bool(s) and wave == 0 and s[0] == layer and s[1] == op and (s[2] == step or op == TICKET) and s[3] == lane

    def flips(self, layer, op, step, wave, lane):
        f = self.flip
        return 1 << f[4] if f and wave == 0 and f[:4] == (layer, op, step, lane) else 0


class _Slot:
    """One contended slot, in exact integers: sums stay integers until ``bits``."""

    def __init__(self, op):
        self.op, self.v, self.lo, self.hi = op, identity(op), 0, 0

    def apply(self, a, times=1):
        """``times`` arrivals of operand ``a``."""
        if times <= 0:
            return
        n = OPS[self.op]
        if n == "add":
            self.v = (self.v + a * times) & M32
        elif n == "sub":
            self.v = (self.v - a * times) & M32
        elif n == "and":
            self.v &= a
        elif n == "or":
            self.v |= a
        elif n in ("xor", "xor_x2"):
            self.v ^= a if times & 1 else 0
        elif n == "umin":
            self.v = min(self.v, a)
        elif n in ("umax", "umax_x2", "max_f64"):
            self.v = max(self.v, a)
        elif n == "smin":
            self.v = min(_signed(self.v), _signed(a)) & M32
        elif n == "smax":
            self.v = max(_signed(self.v), _signed(a)) & M32
        elif n == "add_x2":
            self.v = (self.v + a * times) & M64
        elif n in ("pk_add_f16", "pk_add_bf16"):
            self.lo += (a & 1) * times
            self.hi += (a >> 1 & 1) * times
        else:  # add_f32, add_f64
            self.v += a * times

    def bits(self):
        n = OPS[self.op]
        if n == "add_f32":
            return int_to_fp(self.v, 23, 127)
        if n in ("add_f64", "max_f64"):
            return int_to_fp(self.v, 52, 1023)
        if n == "pk_add_f16":
            return int_to_fp(self.lo, 10, 15) | int_to_fp(self.hi, 10, 15) << 16
        if n == "pk_add_bf16":
            return int_to_fp(self.lo, 7, 127) | int_to_fp(self.hi, 7, 127) << 16
        return self.v


def _put(words, op, lane, bits):
    w = row_word(op) + (2 * lane if wide(op) else lane)
    words[w] = bits & M32
    if wide(op):
        words[w + 1] = bits >> 32


def _contribution(layer, op, lane, seed, iters, hook, b=0):
    """The operands one workgroup sends to slot ``lane`` of ``op``'s row, as a list."""
    out = []
    for t in range(iters):
        for w in range(WAVES):
            if not issues(layer, op, t, w, b) or hook.skips(layer, op, t, w, lane):
                continue
            r = dev_bit(op, b, lane) if layer == DEV and OPS[op] in ("and", "or") else raw(layer, op, t, w, lane, seed)
            out.append(operand(layer, op, r ^ hook.flips(layer, op, t, w, lane)))
    return out


def region(layer: int, seed: int, iters: int, skip=None, flip=None):
    """One workgroup's region of layer lds or l2 after ``iters`` steps -> (uint32[2688], digests uint32[4][64]),
    read-only: computed once per argument set."""
    return _region(layer, seed, iters, tuple(skip) if skip else None, tuple(flip) if flip else None)


@functools.lru_cache(maxsize=256)
def _region(layer, seed, iters, skip, flip):
    hook = _Hook(skip, flip)
    words = np.zeros(REGION_WORDS, dtype=np.uint32)
    for op in range(N_CONTENDED):
        for lane in range(LANES):
            s = _Slot(op)
            for a in _contribution(layer, op, lane, seed, iters, hook):
                s.apply(a)
            _put(words, op, lane, s.bits())
    digest = np.zeros((WAVES, LANES), dtype=np.uint32)
    for w in range(WAVES):
        for lane in range(LANES):
            mem = [0] * 5
            h = cur = 0
            for t in range(iters):
                for op in range(FIRST_RET, CAS):
                    a = operand(layer, op, raw(layer, op, t, w, lane, seed) ^ hook.flips(layer, op, t, w, lane))
                    if hook.skips(layer, op, t, w, lane):
                        continue
                    i = op - FIRST_RET
                    h = fold(h, mem[i])
                    v = mem[i]
                    mem[i] = {"add_rtn": (v + a) & M32, "inc": 0 if v >= a else v + 1,
                              "dec": a if v == 0 or v > a else v - 1, "swap": a}[OPS[op]]
                clean = raw(layer, CAS, t, w, lane, seed)
                if not hook.skips(layer, CAS, t, w, lane):  # compare with what the program tracks: must succeed
                    h = fold(h, mem[4])
                    if mem[4] == cur:
                        mem[4] = clean ^ hook.flips(layer, CAS, t, w, lane)
                cur = clean
                h = fold(h, mem[4])  # compare with a wrong value: must fail
                if mem[4] == clean ^ M32:
                    mem[4] = clean ^ 0x5A5A5A5A
            digest[w, lane] = h
            for i in range(5):
                words[priv_word(FIRST_RET + i, w, lane)] = mem[i]
    words.setflags(write=False)
    digest.setflags(write=False)
    return words, digest


OWN = ("umin", "umax", "smin", "smax", "umax_x2", "max_f64")  # dev: wave 0's operand at step 0 is the workgroup's own


def dev_own_raw(op: int, b: int, lane: int, seed: int) -> int:
    def word(part):
        return mix(DEV << 40 | op << 32 | part << 8 | lane | (b + 1) << 44, seed)
    return word(1) << 32 | word(0) if wide(op) else word(0)


def _dev_contribution(op, lane, seed, iters, hook, b):
    """The operands workgroup ``b`` sends to slot ``lane`` of ``op``'s dev rows."""
    out = []
    for t in range(iters):
        for w in range(WAVES):
            if not issues(DEV, op, t, w, b) or hook.skips(DEV, op, t, w, lane):
                continue
            if OPS[op] in ("and", "or"):
                r = dev_bit(op, b, lane)
            elif OPS[op] in OWN and t == 0 and w == 0:
                r = dev_own_raw(op, b, lane, seed)
            else:
                r = raw(DEV, op, t, w, lane, seed)
            out.append(operand(DEV, op, r ^ hook.flips(DEV, op, t, w, lane)))
    return out


def dev_rows(seed: int, iters: int, wg_xcc, struck=(), skip=None, flip=None, only_op=None):
    """The nine dev row-sets after a run of len(wg_xcc) workgroups, workgroup b on XCD wg_xcc[b];
    the hooks apply to the workgroups in ``struck``. -> uint32[9][1408], read-only: computed once per
    argument set. ``only_op``: that op's rows only, the others zero (for searches)."""
    skip, flip = (tuple(h) if h and h[0] == DEV else None for h in (skip, flip))  # another layer's hook: no effect
    return _dev_rows(seed, iters, tuple(wg_xcc), tuple(sorted(struck)) if skip or flip else (), skip, flip, only_op)


@functools.lru_cache(maxsize=64)
def _dev_rows(seed, iters, wg_xcc, struck, skip, flip, only_op):
    hook, none = _Hook(skip, flip), _Hook()
    struck = set(struck)
    pops = [[b for b, x in enumerate(wg_xcc) if s == ALL_XCD or x == s] for s in range(DEV_ROWSETS)]
    out = np.zeros((DEV_ROWSETS, ROWSET_WORDS), dtype=np.uint32)
    for op in range(N_CONTENDED) if only_op is None else (only_op,):
        name = OPS[op]
        for lane in range(LANES):
            if name in OWN or name in ("and", "or"):  # the contribution depends on the workgroup
                per_b = {}
                for b in range(len(wg_xcc)):
                    if name in ("and", "or") and b not in struck and lane != (b >> 5) & 63:
                        continue  # an untouched workgroup sends the identity to every other lane
                    per_b[b] = _dev_contribution(op, lane, seed, iters, hook if b in struck else none, b)
                for s, pop in enumerate(pops):
                    slot = _Slot(op)
                    for b in pop:
                        for a in per_b.get(b, ()):
                            slot.apply(a)
                    _put(out[s], op, lane, slot.bits())
                continue
            clean = _dev_contribution(op, lane, seed, iters, none, 0)
            hit = _dev_contribution(op, lane, seed, iters, hook, 0)
            for s, pop in enumerate(pops):
                if name in ("pk_add_f16", "pk_add_bf16"):
                    pop = [b for b in pop if b < PACKED_WORKGROUPS]
                n_hit = sum(1 for b in pop if b in struck)
                slot = _Slot(op)
                for a in clean:
                    slot.apply(a, len(pop) - n_hit)
                for a in hit:
                    slot.apply(a, n_hit)
                _put(out[s], op, lane, slot.bits())
    out.setflags(write=False)
    return out


def lds16(seed: int, iters: int, skip=None, flip=None):
    """The lds layer's second addressing (hook layer LDS16): a row-set of which slots 0..15 of every row
    receive lanes j, j + 16, j + 32, j + 48 of every wave; the other slots keep the initial value."""
    return _lds16(seed, iters, tuple(skip) if skip else None, tuple(flip) if flip else None)


@functools.lru_cache(maxsize=256)
def _lds16(seed, iters, skip, flip):
    hook = _Hook(skip, flip)
    words = np.zeros(ROWSET_WORDS, dtype=np.uint32)
    for op in range(N_CONTENDED):
        for lane in range(LANES):
            _put(words, op, lane, identity(op))
        for j in range(SLOTS16):
            s = _Slot(op)
            for lane in range(j, LANES, SLOTS16):
                for a in _contribution(LDS16, op, lane, seed, iters, hook):
                    s.apply(a)
            _put(words, op, j, s.bits())
    words.setflags(write=False)
    return words


def _struck(wg_xcc, hooked, xcc, workgroup):
    return [b for b in range(len(wg_xcc))
            if hooked and (xcc is None or wg_xcc[b] == xcc) and (workgroup is None or b == workgroup)]


def expected(seed: int, iters: int, workgroups: int, wg_xcc, skip=None, flip=None, xcc=None, workgroup=None) -> dict:
    """What a run must leave behind. ``wg_xcc``: the XCD of each of the ``workgroups`` workgroups. The
    hooks strike wave 0 of every workgroup, of XCD ``xcc``'s or of workgroup ``workgroup`` only.
    -> {"lds", "lds_digest", "lds16", "l2", "l2_digest"} of a struck workgroup (of any, without hooks),
    {"clean_lds", ...} of the others, "dev" uint32[9][1408] and "struck", the struck workgroups."""
    wg_xcc = list(wg_xcc)
    assert len(wg_xcc) == workgroups
    struck = _struck(wg_xcc, bool(skip or flip), xcc, workgroup)
    out = {"struck": struck}
    for name, layer in (("lds", LDS), ("l2", L2)):
        out["clean_" + name], out["clean_" + name + "_digest"] = region(layer, seed, iters)
        mine = [h if h and h[0] == layer else None for h in (skip, flip)]  # another layer's hook: no effect
        out[name], out[name + "_digest"] = region(layer, seed, iters, *mine)
    out["clean_lds16"] = lds16(seed, iters)
    out["lds16"] = lds16(seed, iters, *[h if h and h[0] == LDS16 else None for h in (skip, flip)])
    out["dev"] = dev_rows(seed, iters, wg_xcc, struck, skip, flip)
    out["clean_dev"] = dev_rows(seed, iters, wg_xcc)
    return out


def _slots(words):
    """A region's or row-set's words as slot values: (op, index, value)."""
    out = []
    for op in range(N_CONTENDED):
        for lane in range(LANES):
            w = row_word(op) + (2 * lane if wide(op) else lane)
            out.append((op, lane, int(words[w]) | (int(words[w + 1]) << 32 if wide(op) else 0)))
    for i in range(ROWSET_WORDS, len(words)):
        j = i - ROWSET_WORDS
        out.append((FIRST_RET + j // (WAVES * LANES), j % (WAVES * LANES), int(words[i])))
    return out


def predict(seed: int, iters: int, wg_xcc, layers: int = 7, skip=None, flip=None, xcc=None, workgroup=None) -> dict:
    """The counts and the first fault the report must show for a run with these hooks."""
    wg_xcc = list(wg_xcc)
    struck = _struck(wg_xcc, bool(skip or flip), xcc, workgroup)
    n = len(struck)
    first = []  # (layer, op, slot, row)
    counts = {"ldsBadSlots": 0, "l2BadSlots": 0, "devBadSlots": 0, "badReturns": 0, "ticketFaults": 0}
    bad_wg = False
    hooked = {h[0] for h in (skip, flip) if h}  # the layers a hook can change
    for bit, name, layer in ((1, "lds", LDS), (2, "l2", L2)):
        if not layers & bit or not n or layer not in hooked:
            continue
        x0 = min(wg_xcc[b] for b in struck)
        mine = [h if h and h[0] == layer else None for h in (skip, flip)]
        (words, digest), (clean, clean_digest) = region(layer, seed, iters, *mine), region(layer, seed, iters)
        diff = [(op, i) for (op, i, v), (_, _, c) in zip(_slots(words), _slots(clean)) if v != c]
        counts[name + "BadSlots"] = len(diff) * n
        first += [(layer, op, i, x0) for op, i in diff]
        dd = np.argwhere(digest != clean_digest)
        counts["badReturns"] += len(dd) * n
        first += [(layer, RETURNS, int(w) * LANES + int(l), x0) for w, l in dd]
        bad_wg = bad_wg or bool(diff) or len(dd) > 0
    if layers & 1 and n and LDS16 in hooked:  # the second addressing: the lds layer's, slots 64..79
        x0 = min(wg_xcc[b] for b in struck)
        mine = [h if h and h[0] == LDS16 else None for h in (skip, flip)]
        diff = [(op, i) for (op, i, v), (_, _, c) in zip(_slots(lds16(seed, iters, *mine)), _slots(lds16(seed, iters))) if v != c]
        counts["ldsBadSlots"] += len(diff) * n
        first += [(LDS, op, LANES + i, x0) for op, i in diff]
        bad_wg = bad_wg or bool(diff)
    if layers & 1 and n and skip and skip[0] == LDS and skip[1] == TICKET:
        counts["ticketFaults"] = n
        first.append((LDS, TICKET, 0, min(wg_xcc[b] for b in struck)))
        bad_wg = True
    if layers & 4 and n and DEV in hooked:
        ops = {h[1] for h in (skip, flip) if h and h[0] == DEV}
        only = ops.pop() if len(ops) == 1 else None  # a hook changes its own op's rows only: the others need no look
        rows, clean = (dev_rows(seed, iters, wg_xcc, struck, skip, flip, only_op=only),
                       dev_rows(seed, iters, wg_xcc, only_op=only))
        for s in range(DEV_ROWSETS):
            diff = [(op, i) for (op, i, v), (_, _, c) in zip(_slots(rows[s]), _slots(clean[s])) if v != c]
            counts["devBadSlots"] += len(diff)
            first += [(DEV, op, i, s) for op, i in diff]
    counts["badWorkgroups"] = n if bad_wg else 0
    f = min(first) if first else None
    counts.update(firstBadLayer=LAYERS[f[0]] if f else None, firstBadOp=OPS[f[1]] if f else None,
                  firstBadSlot=f[2] if f else None, firstBadXcc=f[3] if f else None)
    return counts


def decisive(layer: int, op: int, seed: int, iters: int, wg_xcc=(0,), skip: bool = False, prefer: int = 0, xcc=None,
             workgroup=None):
    """A (step, lane, bit) whose flip — or, ``skip``, a (step, lane) whose skip — changes the final value of a
    slot of ``op`` (the min / max family, ``or`` / ``and`` and the masked operands absorb most hooks), or
    None. The hook strikes every workgroup, XCD ``xcc``'s or workgroup ``workgroup`` only (dev layer: of the
    placement ``wg_xcc``). Lane ``prefer`` is tried first, then the seam lanes 0, 31, 32, 63, then the rest."""
    lanes = list(dict.fromkeys([prefer, 0, 31, 32, 63] + list(range(LANES))))
    struck = _struck(list(wg_xcc), True, xcc, workgroup)
    steps = range(iters) if issues(layer, op, 1, 0, 0) else (0,)  # some dev ops arrive at step 0 only
    for lane in lanes:
        for t in steps:
            for bit in (None,) if skip else (0, 31, 32, 63) if wide(op) else (0, 31):
                hook = dict(skip=(layer, op, t, lane)) if skip else dict(flip=(layer, op, t, lane, bit))
                if layer == DEV:
                    changed = (dev_rows(seed, iters, wg_xcc, struck, only_op=op, **hook) !=
                               dev_rows(seed, iters, wg_xcc, only_op=op)).any()
                elif layer == LDS16:
                    changed = (lds16(seed, iters, **hook) != lds16(seed, iters)).any()
                else:
                    a, b = region(layer, seed, iters, **hook), region(layer, seed, iters)
                    changed = (a[0] != b[0]).any() or (a[1] != b[1]).any()
                if changed:
                    return (t, lane) if skip else (t, lane, bit)
    return None


def decisive_workgroup(op: int, lane: int, seed: int, iters: int, population) -> int | None:
    """dev layer, min / max family: the workgroup of ``population`` whose own operand (wave 0, step 0) is
    slot ``lane``'s extreme, so that the slot changes when that one arrival is lost; None when an operand
    every workgroup shares, or a tie, decides the slot."""
    assert OPS[op] in OWN
    none = _Hook()
    shared = _Slot(op)
    for a in _dev_contribution(op, lane, seed, iters, none, 0)[1:]:  # [0] is the own operand of workgroup 0
        shared.apply(a)
    own = {b: operand(DEV, op, dev_own_raw(op, b, lane, seed)) for b in population}
    if not own:
        return None
    full = _Slot(op)
    full.v = shared.v
    for a in own.values():
        full.apply(a)
    winners = [b for b, a in own.items() if a == full.v or (OPS[op] in ("smin", "smax") and a & M32 == full.v)]
    without = _Slot(op)
    without.v = shared.v
    for b, a in own.items():
        if winners and b != winners[0]:
            without.apply(a)
    return winners[0] if len(winners) == 1 and without.v != full.v else None


# ---------------------------------------------------------------------------- one atomic at a time

def _bf16_round(x: np.float32) -> int:
    u = int(np.float32(x).view(np.uint32))
    return (u + 0x7FFF + (u >> 16 & 1)) >> 16 & 0xFFFF


def _hw_apply(op: int, old: int, a: int) -> int:
    """One atomic as the hardware performs it, on the slot's bits."""
    n = OPS[op]
    if n in ("add", "add_rtn"):
        return (old + a) & M32
    if n == "sub":
        return (old - a) & M32
    if n == "and":
        return old & a
    if n == "or":
        return old | a
    if n in ("xor", "xor_x2"):
        return old ^ a
    if n == "umin":
        return min(old, a)
    if n in ("umax", "umax_x2"):
        return max(old, a)
    if n == "smin":
        return min(_signed(old), _signed(a)) & M32
    if n == "smax":
        return max(_signed(old), _signed(a)) & M32
    if n == "add_x2":
        return (old + a) & M64
    if n == "add_f32":
        return int((np.uint32(old).view(np.float32) + np.float32(a)).view(np.uint32))
    if n == "add_f64":
        return int((np.uint64(old).view(np.float64) + np.float64(a)).view(np.uint64))
    if n == "max_f64":
        return int(np.maximum(np.uint64(old).view(np.float64), np.float64(a)).view(np.uint64))
    if n == "pk_add_f16":
        lo = np.uint16(old & 0xFFFF).view(np.float16) + np.float16(a & 1)
        hi = np.uint16(old >> 16).view(np.float16) + np.float16(a >> 1 & 1)
        return int(lo.view(np.uint16)) | int(hi.view(np.uint16)) << 16
    if n == "pk_add_bf16":
        lo = np.uint32((old & 0xFFFF) << 16).view(np.float32) + np.float32(a & 1)
        hi = np.uint32(old >> 16 << 16).view(np.float32) + np.float32(a >> 1 & 1)
        return _bf16_round(lo) | _bf16_round(hi) << 16
    raise ValueError(n)


def simulate(seed: int, iters: int, wg_xcc, rng: random.Random) -> dict:
    """Every contended atomic of a clean run, one at a time in an order drawn from ``rng``, with the
    hardware's arithmetic. -> {"lds": [per workgroup uint32[1408]], "l2": likewise, "dev": uint32[9][1408]}
    (the row-sets only: the private words have one writer and no arrival order)."""
    def fresh():
        return {(op, lane): identity(op) for op in range(N_CONTENDED) for lane in range(LANES)}
    nwg = len(wg_xcc)
    mem = {("lds", b): fresh() for b in range(nwg)}
    mem.update({("l2", b): fresh() for b in range(nwg)})
    mem.update({("dev", s): fresh() for s in range(DEV_ROWSETS)})
    events = []
    for b in range(nwg):
        for layer in (LDS, L2, DEV):
            for op in range(N_CONTENDED):
                for t in range(iters):
                    for w in range(WAVES):
                        if not issues(layer, op, t, w, b):
                            continue
                        for lane in range(LANES):
                            if layer == DEV and OPS[op] in ("and", "or"):
                                r = dev_bit(op, b, lane)
                            elif layer == DEV and OPS[op] in OWN and t == 0 and w == 0:
                                r = dev_own_raw(op, b, lane, seed)
                            else:
                                r = raw(layer, op, t, w, lane, seed)
                            a = operand(layer, op, r)
                            if layer == DEV:
                                events.append((("dev", wg_xcc[b]), op, lane, a))
                                events.append((("dev", ALL_XCD), op, lane, a))
                            else:
                                events.append(((LAYERS[layer], b), op, lane, a))
    rng.shuffle(events)
    for where, op, lane, a in events:
        m = mem[where]
        m[op, lane] = _hw_apply(op, m[op, lane], a)

    def words(m):
        out = np.zeros(ROWSET_WORDS, dtype=np.uint32)
        for (op, lane), v in m.items():
            _put(out, op, lane, v)
        return out
    return {"lds": [words(mem["lds", b]) for b in range(nwg)], "l2": [words(mem["l2", b]) for b in range(nwg)],
            "dev": np.stack([words(mem["dev", s]) for s in range(DEV_ROWSETS)])}


def digest_of(words) -> int:
    h = 0
    for w in np.asarray(words, dtype=np.uint32).ravel().tolist():
        h = fold(h, w)
    return h


def pinned(seed: int, iters: int) -> list[int]:
    """The digests both sides are pinned to: the lds region, its return digests, the l2 region, its
    return digests, the dev rows of 3 workgroups on XCDs 0, 1, 0, and the lds layer's second addressing."""
    lds, ld = region(LDS, seed, iters)
    l2, l2d = region(L2, seed, iters)
    return [digest_of(lds), digest_of(ld), digest_of(l2), digest_of(l2d), digest_of(dev_rows(seed, iters, [0, 1, 0])),
            digest_of(lds16(seed, iters))]
