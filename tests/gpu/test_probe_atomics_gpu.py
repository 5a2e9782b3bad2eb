"""The probe's atomic-unit phase on a real MI355X (run with ``-m gpu``).

The phase's workgroups run a fixed program of atomic read-modify-write instructions through their CU's LDS
atomic unit, through the L2 atomic units on a region of their own, and at device scope on nine row-sets
that the workgroups of an XCD, or of all XCDs, add to. The tests compare workgroup 0's dump word for word
with the twin (``gpupool.ops.atomics``: Python integers), which proves that every atomic computes and
returns what its definition says and that no update is lost or doubled under contention, and prove on
the hardware that one update that is not issued, or one flipped operand bit (in every workgroup, on one
XCD, in one workgroup), is found where the twin says it must show: the same counts, the same first fault.

The shapes: ``iters`` 1, 2, 3 and the default; grid factors 1 and 3; lanes 0, 31, 32, 63; bits 0, 31 and,
for the 8-byte ops, 32 and 63. A hook the arithmetic absorbs (a flipped bit the operand's mask drops, an
even number of workgroups flipping one xor bit, an ``or`` the other steps repeat) must report a clean
run: the twin predicts that too, and the tests take what it says.
"""
from __future__ import annotations

import pytest

from gpupool.agent import simprobe
from gpupool.agent.prober import Prober
from gpupool.ops import atomics as tw

pytestmark = pytest.mark.gpu

SEED = tw.SEED_BASE  # device ordinal 0
ITERS = simprobe.SIM_ATOM_ITERS  # the library's default (options.h atom::kIters)
MIB = 1 << 20
PROBE = dict(hbm_bytes=64 * MIB, gemm_n=512)
DEFAULT_KEYS = {"device", "hipUUID", "gcnArch", "passed", "hbm", "mfma", "cus", "ms", "phases", "reportMs"}
BLOCK_KEYS = ["ok", "iters", "layers", "workgroups", "wgPerXcd", "cusTested", "cusVerified", "perXcd", "badCUs",
              "badWorkgroups", "ldsBadSlots", "l2BadSlots", "devBadSlots", "badReturns", "ticketFaults", "firstBadCU",
              "firstBadLayer", "firstBadOp", "firstBadSlot", "firstBadXcc", "ms"]
COUNTS = BLOCK_KEYS[9:15]
DUMP_KEYS = ["dumpCU", "dumpSimds", "ldsTable", "ldsTable16", "ldsDigests", "l2Digests", "region", "devRows", "wgKeys",
             "wgXcc"]
PREDICTED = COUNTS + ["firstBadLayer", "firstBadOp", "firstBadSlot", "firstBadXcc"]
# a representative op of each class: add xor or umin add_x2 add_f32 pk_add_bf16, and swap and cas
CONTENDED = (0, 4, 3, 5, 12, 9, 11)
RETURNING = (20, 21)
HOOK_ITERS = 2


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
def placement(hip):
    """Where the workgroups of a factor-1 grid ran: the CU key of each, from one dump. The dispatcher deals
    them out anew every run, so a test that needs the placement of ITS run takes it from that run's report
    (wgPerXcd) and uses this one only for what does not depend on it."""
    r = hip.atomics(0, iters=1, want_stage=2)
    assert r["passed"], r
    return r["wgKeys"]


@pytest.mark.parametrize("iters", sorted({1, 2, 3, ITERS}))
@pytest.mark.parametrize("stage", (1, 2))
def test_dump_of_workgroup_0_equals_the_twin(hip, stage, iters):
    """Stage 1: the LDS tables and the digests as they stood after step 0 of a run of ``iters`` steps, which
    goes on and is verified in full; stage 2: after the last step. The region and the dev rows are the whole
    run's either way."""
    r = hip.atomics(0, iters=iters, want_stage=stage)
    assert list(r) == ["device", "passed"] + BLOCK_KEYS + DUMP_KEYS, list(r)
    assert r["passed"] and r["iters"] == iters, {k: r[k] for k in BLOCK_KEYS}
    assert 0 <= r["dumpCU"] < 2048 and sorted(r["dumpSimds"]) == [0, 1, 2, 3], r["dumpSimds"]
    assert r["dumpCU"] == r["wgKeys"][0]
    assert [r["wgXcc"].count(x) for x in range(8)] == r["wgPerXcd"] and len(r["wgXcc"]) == r["workgroups"]
    then = tw.expected(SEED, 1 if stage == 1 else iters, r["workgroups"], r["wgXcc"])
    full = tw.expected(SEED, iters, r["workgroups"], r["wgXcc"])
    for got, e, want in (("ldsTable", then, "lds"), ("ldsTable16", then, "lds16"), ("ldsDigests", then, "lds_digest"),
                         ("l2Digests", then, "l2_digest"), ("region", full, "l2"), ("devRows", full, "dev")):
        diff = (r[got] != e[want]).sum()
        assert diff == 0, f"{got}: {diff} word(s) differ from the twin"
    # the dump is data, not an untouched buffer: the add rows hold sums, the digests the second cas's return
    assert r["devRows"][:, :64].any(axis=1).all() and r["ldsTable"][:64].any() and r["region"][:64].any()
    assert r["ldsTable16"][:16].any() and r["ldsDigests"].any() and r["l2Digests"].any()


def test_clean_run_at_the_defaults(hip, cus):
    r = hip.atomics(0)
    print(f"atomics: {r['cusVerified']}/{cus} CUs by {r['workgroups']} workgroups x {r['iters']} steps in {r['ms']:.3f} ms")
    assert list(r) == ["device", "passed"] + BLOCK_KEYS, list(r)
    assert r["passed"] and r["ok"], r
    assert r["iters"] == ITERS and r["layers"] == simprobe.SIM_ATOM_LAYERS, r
    assert r["cusVerified"] == r["cusTested"] == cus == sum(r["perXcd"]), r
    assert sum(r["wgPerXcd"]) == r["workgroups"] == simprobe.SIM_ATOM_BLOCKS_PER_CU * cus, r
    assert all(r[k] == 0 for k in COUNTS) and r["badCUs"] == 0, r
    assert all(r[k] is None for k in ("firstBadCU", "firstBadLayer", "firstBadOp", "firstBadSlot", "firstBadXcc")), r
    for factor in (1, 3):  # workgroups == atomBlocksPerCU x CUs: all of them ran, and a larger grid grows the buffers
        for iters in (1, 2, 3, ITERS):
            f = hip.atomics(0, iters=iters, atomBlocksPerCU=factor)
            assert f["passed"] and f["iters"] == iters and sum(f["wgPerXcd"]) == f["workgroups"] == factor * cus, f
    for layers in (1, 2, 4, 5):  # each layer alone
        f = hip.atomics(0, iters=2, atomLayers=layers)
        assert f["passed"] and f["layers"] == layers, f


def test_clean_run_inside_the_claim_probe(hip, cus):
    plain = hip.run(0, **PROBE)
    assert set(plain) == DEFAULT_KEYS and plain["passed"], sorted(plain)
    r = hip.run(0, atom_check=True, **PROBE)
    assert set(r) == DEFAULT_KEYS | {"atomics"}, sorted(r)
    assert list(r).index("atomics") == list(r).index("ms") - 1 and list(r["atomics"]) == BLOCK_KEYS
    assert set(r["phases"]) == set(plain["phases"])
    print(f"atomics inside the probe: {r['atomics']['cusVerified']}/{cus} CUs in {r['atomics']['ms']:.3f} ms")
    assert r["passed"] and r["atomics"]["ok"] and r["atomics"]["cusVerified"] == cus, r
    for extra in ({"atomFirst": 1}, {"overlap": 0}, {"mfma": False}, {"alu_check": True, "lds_check": True}):
        f = hip.run(0, atom_check=True, **{**PROBE, **extra})
        assert f["passed"] and f["atomics"]["ok"] and list(f).index("atomics") == list(f).index("ms") - 1, f
    off = hip.run(0, atom_check=False, **PROBE)  # with the option off after runs with it on: the default report
    assert set(off) == DEFAULT_KEYS and off["passed"], off


def _check(hip, r, kw, wg_xcc, iters=HOOK_ITERS):
    p = tw.predict(SEED, iters, wg_xcc, skip=kw.get("injectAtomSkip"), flip=kw.get("injectAtomFlip"),
                   xcc=kw.get("injectAtomFaultXcc"), workgroup=kw.get("injectAtomFaultWorkgroup"))
    got = {k: r[k] for k in PREDICTED}
    assert got == p, (kw, got, p)
    assert r["passed"] == (not any(p[k] for k in COUNTS)), r
    return p


def _hooks(layer, op):
    """A skip and a flip of ``op`` in ``layer`` that the twin finds decisive when every workgroup is struck;
    the search starts at a seam lane."""
    lane = (0, 31, 32, 63)[(layer + op) % 4]
    s, f = (tw.decisive(layer, op, SEED, HOOK_ITERS, skip=k, prefer=lane) for k in (True, False))
    assert s is not None and f is not None, (layer, tw.OPS[op])  # these layers' operands leave these classes a decisive hook
    return [dict(injectAtomSkip=[layer, op, *s]), dict(injectAtomFlip=[layer, op, *f])]


# the second addressing (hook layer 3) puts 32 operands on a slot: or and umin saturate, the linear ops do not
@pytest.mark.parametrize("layer,op", [(layer, op) for layer in (tw.LDS, tw.L2) for op in CONTENDED + RETURNING] +
                         [(tw.LDS16, op) for op in (0, 4, 12, 9, 11)])
def test_faults_in_the_lds_and_l2_layers_are_found_where_they_are(hip, cus, placement, layer, op):
    for kw in _hooks(layer, op):
        # every workgroup: the counts do not depend on the placement
        r = hip.atomics(0, iters=HOOK_ITERS, **kw)
        p = _check(hip, r, kw, [k >> 8 for k in placement])
        assert not r["passed"] and p["badWorkgroups"] == r["workgroups"] and r["badCUs"] == cus and r["cusVerified"] == 0, r
        assert p["l2BadSlots" if layer == tw.L2 else "ldsBadSlots"] + p["badReturns"] >= r["workgroups"], p
        if layer == tw.LDS16:
            assert 64 <= r["firstBadSlot"] < 80 and r["firstBadLayer"] == "lds", r
        # one XCD: that XCD's workgroups and CUs, nothing on the others
        x = 5
        r = hip.atomics(0, iters=HOOK_ITERS, injectAtomFaultXcc=x, **kw)
        wg_xcc = [xx for xx in range(8) for _ in range(r["wgPerXcd"][xx])]  # which ones ran there does not matter here
        _check(hip, r, {**kw, "injectAtomFaultXcc": x}, wg_xcc)
        assert r["badWorkgroups"] == r["wgPerXcd"][x] and r["firstBadXcc"] == x and r["firstBadCU"] >> 8 == x, r
        assert [cus // 8 - v for v in r["perXcd"]] == [r["badCUs"] if xx == x else 0 for xx in range(8)], r
        # one workgroup: one CU, the one in its record
        w = 77
        r = hip.atomics(0, iters=HOOK_ITERS, want_stage=2, injectAtomFaultWorkgroup=w, **kw)
        _check(hip, r, {**kw, "injectAtomFaultWorkgroup": w}, r["wgXcc"])
        assert r["badWorkgroups"] == 1 and r["badCUs"] == 1 and r["firstBadCU"] == r["wgKeys"][w], r
        assert r["cusVerified"] == cus - 1
        # the clean workgroup 0's dump is the clean twin's
        e = tw.expected(SEED, HOOK_ITERS, r["workgroups"], r["wgXcc"])
        assert (r["ldsTable"] == e["clean_lds"]).all() and (r["region"] == e["clean_l2"]).all()
        assert (r["ldsTable16"] == e["clean_lds16"]).all()
    assert hip.atomics(0, iters=HOOK_ITERS)["passed"]  # right after a faulted run: the values were restored


def _dev_hooks(op, n, scope):
    """A skip and a flip of ``op`` in the dev layer that the twin finds decisive for ``scope`` (every workgroup,
    or one), with the workgroup to strike. The row every workgroup hits does not depend on the placement, so
    the search runs on a made-up one. The min / max family: the struck workgroup is the one whose own operand
    decides the slot. None where the arithmetic leaves no decisive hook."""
    canon = [b % 8 for b in range(n)]
    lane = (0, 31, 32, 63)[op % 4]
    w = None
    if scope == "one":
        w = 131
        if tw.OPS[op] in tw.OWN:
            lane, w = next((ln, tw.decisive_workgroup(op, ln, SEED, HOOK_ITERS, range(n))) for ln in (lane, 0, 31, 32, 63, 1, 2, 3)
                           if tw.decisive_workgroup(op, ln, SEED, HOOK_ITERS, range(n)) is not None)
    s, f = (tw.decisive(tw.DEV, op, SEED, HOOK_ITERS, canon, skip=k, prefer=lane, workgroup=w) for k in (True, False))
    return w, [dict(injectAtomSkip=[tw.DEV, op, *s]) if s else None, dict(injectAtomFlip=[tw.DEV, op, *f]) if f else None]


def _dev_rows_match(r, op, kw, xcc=None, workgroup=None):
    """The dumped rows of the struck op equal the twin's with the same hook on this run's placement (the other
    ops' rows are the clean run's: the kernel's own count says so). -> the row-sets the hook changed."""
    struck = [b for b, x in enumerate(r["wgXcc"]) if (xcc is None or x == xcc) and (workgroup is None or b == workgroup)]
    hit = tw.dev_rows(SEED, HOOK_ITERS, r["wgXcc"], struck, kw.get("injectAtomSkip"), kw.get("injectAtomFlip"), only_op=op)
    clean = tw.dev_rows(SEED, HOOK_ITERS, r["wgXcc"], only_op=op)
    w0 = tw.row_word(op)
    w1 = w0 + (128 if tw.wide(op) else 64)
    assert (r["devRows"][:, w0:w1] == hit[:, w0:w1]).all()
    return {s for s in range(tw.DEV_ROWSETS) if (hit[s] != clean[s]).any()}


@pytest.mark.parametrize("op", CONTENDED)
def test_faults_in_the_dev_layer_are_found_where_they_are(hip, cus, op):
    n = simprobe.SIM_ATOM_BLOCKS_PER_CU * cus
    for scope in ("every", "one"):
        w, hooks = _dev_hooks(op, n, scope)
        # an even number of workgroups that drop or flip the same xor operand cancel in every row they share: the
        # only class and scope without a decisive hook
        assert all(hooks) or (tw.OPS[op] == "xor" and scope == "every" and n % 2 == 0), (tw.OPS[op], scope, hooks)
        for kw in filter(None, hooks):
            extra = {} if w is None else {"injectAtomFaultWorkgroup": w}
            r = hip.atomics(0, iters=HOOK_ITERS, want_stage=2, **extra, **kw)  # the per-XCD rows depend on this run's placement
            p = _check(hip, r, {**kw, **extra}, r["wgXcc"])
            assert not r["passed"] and p["devBadSlots"] >= 1, (kw, extra, p)  # found, not absorbed
            assert r["ldsBadSlots"] == r["l2BadSlots"] == r["badReturns"] == r["badCUs"] == 0 and r["cusVerified"] == cus, r
            assert r["firstBadCU"] is None and r["firstBadLayer"] == "dev" and r["firstBadOp"] == tw.OPS[op], r
            bad_rows = _dev_rows_match(r, op, kw, workgroup=w)
            if w is not None:  # the struck workgroup's own XCD row, if the hook shows there, and the all-XCD row
                assert tw.ALL_XCD in bad_rows and bad_rows <= {r["wgXcc"][w], tw.ALL_XCD}, (bad_rows, r)
            # one XCD only: that XCD's row and the all-XCD row, whatever the twin says of the counts
            x = 2
            r = hip.atomics(0, iters=HOOK_ITERS, want_stage=2, injectAtomFaultXcc=x, **kw)
            p = _check(hip, r, {**kw, "injectAtomFaultXcc": x}, r["wgXcc"])
            bad_rows = _dev_rows_match(r, op, kw, xcc=x)
            assert bad_rows <= {x, tw.ALL_XCD} and (not p["devBadSlots"] or r["firstBadXcc"] == x), (bad_rows, r)
    assert hip.atomics(0, iters=HOOK_ITERS)["passed"]


def test_the_hooks_find_something_in_every_layer_and_class(hip):
    """The predictions above may be "nothing to find"; these are known to be decisive."""
    for kw, key in ((dict(injectAtomSkip=[0, 0, 0, 0]), "ldsBadSlots"), (dict(injectAtomFlip=[1, 12, 0, 63, 63]), "l2BadSlots"),
                    (dict(injectAtomSkip=[2, 0, 1, 32], injectAtomFaultWorkgroup=3), "devBadSlots"),
                    (dict(injectAtomFlip=[2, 9, 0, 31, 0], injectAtomFaultXcc=7), "devBadSlots"),
                    (dict(injectAtomFlip=[2, 11, 0, 0, 1], injectAtomFaultWorkgroup=0), "devBadSlots"),
                    (dict(injectAtomSkip=[1, 20, 0, 31]), "badReturns"), (dict(injectAtomFlip=[0, 21, 0, 32, 31]), "badReturns")):
        r = hip.atomics(0, iters=HOOK_ITERS, **kw)
        assert not r["passed"] and r[key] >= 1, (kw, r)


def test_ticket_test(hip, cus):
    r = hip.atomics(0, injectAtomSkip=[0, tw.TICKET, 0, 63])
    assert not r["passed"] and r["ticketFaults"] == r["workgroups"] == r["badWorkgroups"] and r["badCUs"] == cus, r
    assert (r["firstBadLayer"], r["firstBadOp"], r["firstBadSlot"]) == ("lds", "ticket", 0), r
    assert r["ldsBadSlots"] == r["badReturns"] == 0, r
    r = hip.atomics(0, injectAtomSkip=[0, tw.TICKET, 0, 0], injectAtomFaultXcc=6)
    assert r["ticketFaults"] == r["wgPerXcd"][6] >= 1 and r["firstBadXcc"] == 6, r
    assert [cus // 8 - v for v in r["perXcd"]] == [r["badCUs"] if x == 6 else 0 for x in range(8)], r
    r = hip.atomics(0, want_stage=2, injectAtomSkip=[0, tw.TICKET, 0, 31], injectAtomFaultWorkgroup=200)
    assert r["ticketFaults"] == 1 and r["badCUs"] == 1 and r["firstBadCU"] == r["wgKeys"][200], r
    assert hip.atomics(0, atomLayers=6, injectAtomSkip=[0, tw.TICKET, 0, 63])["passed"]  # the lds layer is not run


def test_back_to_back_runs_start_clean(hip):
    assert hip.atomics(0, iters=3)["passed"] and hip.atomics(0, iters=3)["passed"]
    assert not hip.atomics(0, iters=3, injectAtomSkip=[2, 12, 2, 63])["passed"]
    assert not hip.atomics(0, iters=3, injectAtomFlip=[1, 21, 1, 0, 0])["passed"]
    r = hip.atomics(0, iters=3)  # right after faulted runs: atom_verify stored every initial value back
    assert r["passed"] and all(r[k] == 0 for k in COUNTS), r
    assert hip.atomics(0, iters=3, atomSeed=12345)["passed"]  # another seed: a new expectation table


def test_a_hook_past_the_range_is_off(hip):
    for kw in (dict(injectAtomSkip=[4, 0, 0, 0]), dict(injectAtomSkip=[3, 20, 0, 0]), dict(injectAtomSkip=[0, 0, HOOK_ITERS, 0]), dict(injectAtomFlip=[0, 0, 0, 0, 32]),
               dict(injectAtomFlip=[2, 20, 0, 0, 0]), dict(injectAtomSkip=[0, 0, 0, 64]), dict(injectAtomSkip=[1, 22, 0, 0])):
        assert hip.atomics(0, iters=HOOK_ITERS, **kw)["passed"], kw


def test_failure_reason_through_the_prober(hip):
    f = hip.run(0, atom_check=True, atomIters=2, injectAtomSkip=[1, 4, 1, 32], injectAtomFaultXcc=4, **PROBE)
    assert not f["passed"] and f["hbm"]["ok"] and f["mfma"]["ok"] and f["cus"]["ok"], f  # a skip fails only "atomics"
    a = f["atomics"]
    k = a["firstBadCU"]
    assert a["l2BadSlots"] == a["badCUs"] == a["wgPerXcd"][4] and k >> 8 == 4, a
    assert Prober.explain(f)["error"] == (f"AtomicResultMismatch(l2/xor): {a['l2BadSlots']} slot(s) on {a['badCUs']} CU(s), "
                                          f"first on CU 4/{(k >> 5) & 7}/{(k >> 4) & 1}/{k & 15} slot 32")
    f = hip.run(0, atom_check=True, injectAtomFlip=[2, 0, 0, 31, 31], injectAtomFaultWorkgroup=9, **PROBE)
    a = f["atomics"]
    assert not f["passed"] and a["devBadSlots"] == 2 and a["firstBadXcc"] < 8, a
    assert Prober.explain(f)["error"] == (f"AtomicResultMismatch(dev/add): 2 slot(s) on 0 CU(s), first in the XCD "
                                          f"{a['firstBadXcc']} row slot 31")
    assert hip.run(0, atom_check=True, **PROBE)["passed"]


def test_a_dump_holds_nothing_of_an_earlier_call(hip):
    full = hip.atomics(0, iters=2, want_stage=2)  # fills every section
    assert full["passed"] and any(full["wgKeys"]) and full["ldsTable"].any()
    r = hip.atomics(0, iters=2, want_stage=2, atomLayers=3)  # no dev layer: no records in the dump, rows at their identities
    assert r["passed"] and not any(r["wgKeys"]) and r["ldsTable"].any() and r["region"].any()
    assert (r["devRows"] == tw.dev_rows(SEED, 2, [])).all()
    r = hip.atomics(0, iters=2, want_stage=1, atomLayers=6)  # no lds layer: nothing of it in a stage-1 dump
    assert r["passed"] and not r["ldsTable"].any() and not r["ldsTable16"].any() and not r["ldsDigests"].any()
    assert r["l2Digests"].any() and any(r["wgKeys"])


def test_each_kernels_time(hip):
    runs = [hip.atomics(0, atomTimeKernels=1) for _ in range(9)]
    r = runs[0]
    assert list(r) == ["device", "passed"] + BLOCK_KEYS + ["marchMs", "verifyMs"], list(r)
    march, verify = (sorted(x[k] for x in runs)[4] for k in ("marchMs", "verifyMs"))
    print(f"atom_march {march:.4f} ms, atom_verify {verify:.4f} ms at {r['iters']} steps")
    assert 0 < verify < march, (march, verify)  # the verifier's grid is sized to cost less than the march
    assert "marchMs" not in hip.atomics(0) and "marchMs" not in hip.run(0, atom_check=True, atomTimeKernels=1, **PROBE)["atomics"]


def test_bad_arguments_are_reports(hip):
    for r in (hip.atomics(99), hip.atomics(-1), hip.atomics(99, want_stage=1)):
        assert r["passed"] is False and r["error"], r
        assert "atomics" not in r and "iters" not in r and "region" not in r
    assert hip.atomics(0, iters=0)["iters"] == 1 and hip.atomics(0, iters=99)["iters"] == 64  # clamped, not refused
    assert hip.run(0, **PROBE)["passed"]
