"""The probe's checker kernels against host references on a real MI355X (run with ``-m gpu``).

A device is handed out when the checkers say so: ``gen_operand``, the VALU references with
``count_diff``, and the ABFT sequence (``colsum_partial`` / ``colsum``, ``rowdot``, ``count_ne_u32``).
Here each is compared with ``abft_cases`` (integers on the host) through the test surfaces
``abft_check``, ``gemm_ref``, ``count_diff`` and ``gen_operands``, which launch the production
kernels with the production grids. Every comparison is exact. A checker that skips rows or columns
passes every clean run, because it skips the same part of both sides of its identity; so faults are
placed at every position class of the kernels' loops, and the three counters (integrality / range,
columns, rows) are read apart.
"""
from __future__ import annotations

import numpy as np
import pytest

from . import abft_cases as ac
from . import gemm_cases

pytestmark = pytest.mark.gpu

LOWP = ac.lowp.DTYPES
NONE = 2 ** 64 - 1   # what an output that was never written still holds


def _id(x):
    return "x".join(map(str, x)) if isinstance(x, tuple) else str(x)


@pytest.fixture(scope="module")
def hip(native_built):
    from gpupool.ops import probe
    n = probe.init()
    assert n >= 1, "no HIP device visible"
    return probe


def _assert_vectors(got: np.ndarray, want: ac.Vectors, shape, skip=()):
    m, n, k = shape
    at = 0
    for name, size in (("acol", k), ("bcol", k), ("col_c", n), ("exp_col", n), ("row_c", m), ("exp_row", m)):
        g, w = got[at:at + size], getattr(want, name)
        at += size
        if name in skip:
            continue
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, (f"{name}: {bad.size} of {size} wrong, first at {bad[:8].tolist()}: "
                               f"got {g[bad[:4]].tolist()}, want {w[bad[:4]].tolist()}")


# ------------------------------------------------------------------ clean data
CLEAN = [(d, s, "probe") for d in ac.DTYPES for s in ac.shapes(d)] + \
        [(ac.BF16, (65, 1028, 2056), "max")] + [(d, (65, 260, 1056), "max") for d in LOWP]


@pytest.mark.parametrize("dtype,shape,kind", CLEAN, ids=_id)
def test_clean_vectors_equal_the_host_and_nothing_is_counted(hip, dtype, shape, kind):
    o = ac.operands(dtype, shape, kind)
    vec, counts, _ = ac.run_check(hip, o, o.c)
    _assert_vectors(vec, ac.clean_vectors(o), shape)
    assert counts == (0, 0, 0)


# ------------------------------------------------------------------ one fault, every position class
FAULT_CASES = [(ac.BF16, ac.FAULT_SHAPE), (ac.BF16, (65, 1028, 2056))] + [(d, ac.FAULT_SHAPE) for d in LOWP]
# kind -> (the corrupted value of an element c, the counts; None: not asserted, a clamp decides it)
KINDS = {
    "plus1": (lambda c, b: c + np.float32(1), (0, 1, 1)),
    "plus-quarter": (lambda c, b: c + np.float32(0.25), (1, 0, 0)),
    "nan": (lambda c, b: np.full_like(c, np.nan), (1, None, None)),
    "inf": (lambda c, b: np.full_like(c, np.inf), (1, None, None)),
    "3e9": (lambda c, b: np.full_like(c, 3e9), (1, None, None)),
    "bound+1": (lambda c, b: np.full_like(c, b + 1), (1, 1, 1)),   # an integer no element equals
}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype,shape", FAULT_CASES, ids=_id)
def test_single_fault_at_every_position_class(hip, dtype, shape, kind):
    o = ac.operands(dtype, shape)
    m, n, _ = shape
    pos = ac.fault_positions(m, n)
    idx = np.array([r * n + c for r, c in pos], dtype=np.int64)
    c = o.c
    value, want = KINDS[kind]
    vals = value(c.ravel()[idx], np.float32(o.bound)).astype(np.float32)
    if kind in ("plus1", "plus-quarter"):
        assert (vals.astype(np.float64) == c.ravel()[idx].astype(np.float64) + (1 if kind == "plus1" else 0.25)).all()
    _, counts, fc = ac.run_check(hip, o, c, faults=(idx, vals))
    assert counts == (0, 0, 0)
    for j, w in enumerate(want):
        if w is None:
            continue
        bad = np.nonzero(fc[:, j] != w)[0]
        assert bad.size == 0, (f"counter {j} (odd, columns, rows): want {w} per fault; {bad.size} of {len(pos)} "
                               f"positions differ, first (row, col, got): "
                               f"{[(pos[i][0], pos[i][1], int(fc[i, j])) for i in bad[:8]]}")


# ------------------------------------------------------------------ several elements at once
def _multi(o):
    """name -> (corrupted C, the counts known by construction or None: the predictor's)."""
    m, n, _ = o.shape
    out = {}
    c = o.c
    c[m // 3, 1] += 1
    c[m // 3, n - 2] -= 1
    out["plus-minus-in-a-row"] = (c, (0, 2, 0))
    c = o.c
    c[0, n // 2] += 1
    c[m - 1, n // 2] -= 1
    out["plus-minus-in-a-column"] = (c, (0, 0, 2))
    c = o.c
    c[m - 1] += 1
    out["plus1-on-a-row"] = (c, (0, n, 1))
    c = o.c
    c[[1, m - 2]] = c[[m - 2, 1]]
    out["two-rows-swapped"] = (c, None)
    if m == n:
        out["transposed"] = (np.ascontiguousarray(o.c.T), None)
    return out


MULTI = [(d, s, name) for d, s in FAULT_CASES
         for name in ("plus-minus-in-a-row", "plus-minus-in-a-column", "plus1-on-a-row", "two-rows-swapped", "transposed")
         if name != "transposed" or s[0] == s[1]]   # a non-square C has no transpose of its shape


@pytest.mark.parametrize("dtype,shape,name", MULTI, ids=_id)
def test_multi_element_corruption_counts_are_the_hosts(hip, dtype, shape, name):
    o = ac.operands(dtype, shape)
    cases = _multi(o)
    c, known = cases[name]
    want = ac.predict_counts(o, c)
    if known is not None:
        assert want == known
    if name == "transposed":
        assert want[0] == 0 and want[1] > 0 and want[2] > 0
    vec, counts, _ = ac.run_check(hip, o, c)
    assert counts == want
    _assert_vectors(vec, ac.vectors(o.a_int, o.bt_int, ac.kernel_int(c)), shape, skip=("exp_col", "exp_row"))
    _assert_vectors(vec, ac.clean_vectors(o), shape, skip=("col_c", "row_c"))


# ------------------------------------------------------------------ the element check's reference and comparer
REF = [(ac.BF16, s) for s in ((1, 4, 8), (5, 260, 520), (256, 256, 256))] + \
      [(d, s) for d in LOWP for s in ((1, 4, 32), (65, 260, 1056), (256, 256, 256))]


@pytest.mark.parametrize("kind", ["probe", "max"])
@pytest.mark.parametrize("dtype,shape", REF, ids=_id)
def test_valu_reference_equals_fp64_bit_for_bit(hip, dtype, shape, kind):
    """Integer operands, for the scaled dtypes under their block scales: the float64 product is exact."""
    o = ac.operands(dtype, shape, kind)
    r = ac.run_ref(hip, o)
    bad = np.argwhere(r.view(np.uint32) != o.c.view(np.uint32))
    assert bad.size == 0, (len(bad), [(int(i), int(j), float(r[i, j]), int(o.c_int[i, j])) for i, j in bad[:6]])


GRID = 64 * 256   # count_diff's threads


@pytest.mark.parametrize("count", [1, GRID - 1, GRID, GRID + 1, 70001])
def test_count_diff_counts_what_was_planted(hip, count):
    rng = np.random.default_rng(count)
    x = rng.integers(-1000, 1000, count).astype(np.float32)
    same = x.copy()
    assert hip.count_diff(0, x.ctypes.data, same.ctypes.data, count) == 0
    planted = {0, count - 1} | {GRID * i + j for i in range(5) for j in (0, 1, 63, 64, 255, 256, GRID - 1)}
    planted = sorted(p for p in planted if p < count)
    for subset in (planted[:1], planted[-1:], planted):
        y = x.copy()
        y[subset] += 1
        assert hip.count_diff(0, x.ctypes.data, y.ctypes.data, count) == len(subset)
    y = x.copy()
    y[count // 2] = np.nan
    assert hip.count_diff(0, x.ctypes.data, y.ctypes.data, count) == 1   # NaN against a number


def test_count_diff_compares_bits_not_values(hip):
    """Bit-exact: a zero of the other sign differs, a NaN equals the NaN of the same bits and differs
    from one of other bits. (While the kernel compared with ``!=`` this test pinned the opposite on
    the MI355X: 0 for the three zeros, 1 for the NaN pair.)"""
    x = np.zeros(GRID + 3, dtype=np.float32)
    y = x.copy()
    y[[0, 70, GRID + 2]] = -0.0
    assert (x.view(np.uint32) != y.view(np.uint32)).sum() == 3 and (x == y).all()
    assert hip.count_diff(0, x.ctypes.data, y.ctypes.data, len(x)) == 3
    x = np.zeros(GRID + 3, dtype=np.float32)
    y = x.copy()
    x.view(np.uint32)[5] = y.view(np.uint32)[5] = 0x7FC00000
    assert hip.count_diff(0, x.ctypes.data, y.ctypes.data, len(x)) == 0
    y.view(np.uint32)[5] = 0x7FC00001
    assert hip.count_diff(0, x.ctypes.data, y.ctypes.data, len(x)) == 1


# ------------------------------------------------------------------ the in-probe operands
SIZES = (1, ac.GEN_GRID - 1, ac.GEN_GRID + 1, 512 * 512)
TAIL = 32   # bytes behind what the generator may write


def _gen_bf16(hip, seed, span, count, nzero):
    op = np.zeros(count + TAIL // 2, dtype=np.uint16)
    zero = np.zeros(nzero + 4, dtype=np.uint32)
    hip.gen_operands(0, ac.BF16, seed, span, count, nzero, op.ctypes.data, op.nbytes, None, 0,
                     zero.ctypes.data, zero.nbytes)
    assert (op[count:] == 0xFFFF).all(), "the generator wrote past its last element"
    return op[:count], zero


@pytest.mark.parametrize("seed,span", ac.BF16_SEEDS, ids=lambda v: hex(v) if v > 9 else str(v))
def test_bf16_operands_are_the_documented_integers(hip, seed, span):
    for count in SIZES:
        want = ac.gen_bf16(count, seed, span)
        for nzero in (0, 7, 3 * 512):
            got, zero = _gen_bf16(hip, seed, span, count, nzero)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (count, nzero, bad.size, bad[:8].tolist())
            assert (zero[:nzero] == 0).all() and (zero[nzero:] == ac.MASK).all(), (count, nzero, zero[:8], zero[nzero:])
        v = gemm_cases.bf16_value(got)
        assert (np.abs(v) <= span).all() and (v == np.rint(v)).all()
        if count > 1000:
            assert set(v.astype(int).tolist()) == set(range(-span, span + 1))


def test_a_and_b_of_one_probe_differ(hip):
    for (sa, span), (sb, _), count in ((ac.BF16_SEEDS[0], ac.BF16_SEEDS[1], 256 * 256),
                                       (ac.BF16_SEEDS[2], ac.BF16_SEEDS[3], 512 * 512)):
        a, _ = _gen_bf16(hip, sa, span, count, 0)
        b, _ = _gen_bf16(hip, sb, span, count, 0)
        same = int((a == b).sum())
        # independent draws from 2 span + 1 values agree at about count / (2 span + 1) places
        assert same < count // 2, (hex(sa), hex(sb), same)
        n = int(np.sqrt(count))
        assert not np.array_equal(a.reshape(n, n), a.reshape(n, n).T)   # asymmetric
    for dtype in LOWP:
        sd = ac.lowp_seeds(dtype)
        for s0, s1 in ((sd[0], sd[1]), (sd[2], sd[3])):
            a, _ = _gen_lowp(hip, dtype, s0, 256 * 256)
            b, _ = _gen_lowp(hip, dtype, s1, 256 * 256)
            assert int((a == b).sum()) < len(a) // 2


def _gen_lowp(hip, dtype, seed, count):
    nbytes, nscales = count * ac.lowp.BITS[dtype] // 8, count // 32
    op = np.zeros(nbytes + TAIL, dtype=np.uint8)
    sc = np.zeros(nscales + TAIL, dtype=np.uint8) if ac.lowp.SCALED[dtype] else None
    hip.gen_operands(0, dtype, seed, ac.SCALE_LO[dtype], count, 0, op.ctypes.data, op.nbytes,
                     None if sc is None else sc.ctypes.data, 0 if sc is None else sc.nbytes)
    assert (op[nbytes:] == 0xFF).all(), "the generator wrote past its last word"
    if sc is not None:
        assert (sc[nscales:] == 0xFF).all(), "the generator wrote past its last scale"
        sc = sc[:nscales]
    return op[:nbytes], sc


@pytest.mark.parametrize("dtype", LOWP)
def test_lowp_operands_and_scales_are_the_documented_ones(hip, dtype):
    e = 32 // ac.lowp.BITS[dtype]
    sizes = [e, e * (ac.GEN_GRID - 1), e * (ac.GEN_GRID + 1), 512 * 512]
    for i, seed in enumerate(ac.lowp_seeds(dtype)):
        # once per dtype: more scales than the grid has threads
        for count in sizes + ([32 * (ac.GEN_GRID + 1)] if i == 2 else []):
            got, sc = _gen_lowp(hip, dtype, seed, count)
            want, want_sc = ac.gen_lowp(dtype, count, seed, ac.SCALE_LO[dtype])
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (hex(seed), count, bad.size, bad[:8].tolist())
            if ac.lowp.BITS[dtype] == 8:
                v = ac.lowp.e4m3_decode(got)
                assert (np.abs(v) <= 8).all() and (v == np.rint(v)).all()
                if count > 1000:
                    assert set(v.astype(int).tolist()) == set(range(-8, 9))
            elif count > 1000:
                assert set(ac.lowp.unpack_fp4(got).tolist()) == set(range(16))
            if ac.lowp.SCALED[dtype]:
                assert np.array_equal(sc, want_sc), (hex(seed), count)
                lo = 127 + ac.SCALE_LO[dtype]
                if count >= 32 * 64:
                    assert set(sc.tolist()) == {lo, lo + 1}
                else:
                    assert set(sc.tolist()) <= {lo, lo + 1}
            else:
                assert sc is None


# ------------------------------------------------------------------ refused arguments
REFUSED = [
    (ac.BF16, (8, 8, 12), False),      # k % 8
    (ac.BF16, (8, 6, 8), False),       # n % 4
    (ac.BF16, (0, 8, 8), False),       # m = 0
    (ac.BF16, (8, 8, 8), True),        # bf16 takes no scales
    ("fp8", (8, 8, 40), False),        # k % 32
    ("fp8", (8, 8, 32), True),         # scales passed to fp8
    ("mxfp8", (8, 8, 32), False),      # a scaled dtype without its scales
    ("mxfp4", (8, 8, 32), False),
    ("mxfp4", (8, 10, 64), True),      # n % 4
    ("mxfp8", (0, 8, 32), True),       # m = 0
    ("fp6", (8, 8, 32), True),         # no such dtype
]


@pytest.mark.parametrize("dtype,shape,scales", REFUSED, ids=_id)
def test_bad_arguments_are_refused_before_anything_runs(hip, dtype, shape, scales):
    m, n, k = shape
    a = np.zeros((max(m, 1), 2 * k), dtype=np.uint8)
    bt = np.zeros((n, 2 * k), dtype=np.uint8)
    s = np.full((max(m, n, 1), k), 127, dtype=np.uint8)
    sp = s.ctypes.data if scales else None
    c = np.zeros((max(m, 1), n), dtype=np.float32)
    vec = np.full(2 * (m + n + k), ac.MASK, dtype=np.uint32)
    counts = np.full(3, NONE, dtype=np.uint64)
    with pytest.raises(ValueError):
        hip.abft_check(0, dtype, a.ctypes.data, bt.ctypes.data, sp, sp, c.ctypes.data, m, n, k, 100.0,
                       vec.ctypes.data, counts.ctypes.data)
    assert (vec == ac.MASK).all() and (counts == NONE).all()
    r = gemm_cases.poisoned_c(max(m, 1), n)
    with pytest.raises(ValueError):
        hip.gemm_ref(0, dtype, a.ctypes.data, bt.ctypes.data, sp, sp, r.ctypes.data, m, n, k)
    assert (r.view(np.uint32) == gemm_cases.POISON_BITS).all()


@pytest.mark.parametrize("index", [-2, 3])
def test_unknown_dtype_index_is_refused_by_the_library(hip, index):
    a = np.zeros((8, 64), dtype=np.uint8)
    c = np.zeros((8, 8), dtype=np.float32)
    vec = np.full(2 * (8 + 8 + 32), ac.MASK, dtype=np.uint32)
    counts = np.full(3, NONE, dtype=np.uint64)
    rc = hip.lib().mi355x_probe_abft_check(0, index, a.ctypes.data, a.ctypes.data, None, None, c.ctypes.data, 8, 8, 32,
                                           100.0, vec.ctypes.data, counts.ctypes.data, 0, None, None, None)
    assert rc == -2 and (vec == ac.MASK).all() and (counts == NONE).all()
    r = gemm_cases.poisoned_c(8, 8)
    assert hip.lib().mi355x_probe_gemm_ref(0, index, a.ctypes.data, a.ctypes.data, None, None, r.ctypes.data, 8, 8, 32) == -2
    assert (r.view(np.uint32) == gemm_cases.POISON_BITS).all()
    op = np.zeros(64, dtype=np.uint8)
    assert hip.lib().mi355x_probe_gen_operands(0, index, 1, 0, 32, 0, op.ctypes.data, op.nbytes, None, 0, None, 0) == -2
    assert not op.any()


def test_a_fault_outside_c_and_bad_generator_arguments_are_refused(hip):
    o = ac.operands(ac.BF16, (5, 260, 520))
    m, n, k = o.shape
    c = o.c
    vec = np.full(2 * (m + n + k), ac.MASK, dtype=np.uint32)
    counts, fc = np.full(3, NONE, dtype=np.uint64), np.full(3, NONE, dtype=np.uint64)
    val = np.ones(1, dtype=np.float32)
    for bad_index in (-1, m * n):
        idx = np.array([bad_index], dtype=np.int64)
        with pytest.raises(ValueError):
            hip.abft_check(0, ac.BF16, o.a.ctypes.data, o.bt.ctypes.data, None, None, c.ctypes.data, m, n, k, o.bound,
                           vec.ctypes.data, counts.ctypes.data, 1, idx.ctypes.data, val.ctypes.data, fc.ctypes.data)
        assert (vec == ac.MASK).all() and (counts == NONE).all() and (fc == NONE).all()
    buf = np.zeros(16, dtype=np.uint16)
    for args in ((ac.BF16, 1, 0, 8, 0), (ac.BF16, 1, 2, 0, 0), (ac.BF16, 1, 2, 9, 0), ("fp8", 1, 0, 6, 0),
                 ("mxfp4", 1, 1, 8, 3)):   # span 0; no element; a buffer too small; half a word; lowp zeroes nothing
        dtype, seed, arg, count, nzero = args
        with pytest.raises(ValueError):
            hip.gen_operands(0, dtype, seed, arg, count, nzero, buf.ctypes.data, 16,
                             buf.ctypes.data if dtype == "mxfp4" else None, 16 if dtype == "mxfp4" else 0)
        assert not buf.any()


# ------------------------------------------------------------------ the fault hooks of a probe, by position
PROBE = dict(gemm_n=512, hbm_bytes=1 << 20, patterns=1)
POSITIONS = ((0, 0), (0, 511), (511, 0), (511, 511), (63, 255), (64, 256), (255, 3), (256, 4))


@pytest.mark.parametrize("zero_in_kernel", [1, 0])
def test_probe_counts_an_injected_fault_wherever_it_is(hip, zero_in_kernel):
    for row, col in POSITIONS:
        for mode in (1, 2, 3):
            r = hip.run(0, injectGemmFault=mode, injectGemmFaultRow=row, injectGemmFaultCol=col,
                        zeroInKernel=zero_in_kernel, **PROBE)
            got = r["mfma"]["abftMismatches"]
            assert not r["passed"] and r["mfma"]["elementMismatches"] == 0, (row, col, mode, r)
            assert (got == 2 if mode == 1 else got == 1 if mode == 2 else 1 <= got <= 3), (row, col, mode, got)
    for row, col in ((512, 0), (0, 512), (-2, 5), (5, -2)):   # out of range: no fault
        r = hip.run(0, injectGemmFault=1, injectGemmFaultRow=row, injectGemmFaultCol=col,
                    zeroInKernel=zero_in_kernel, **PROBE)
        assert r["passed"] and r["mfma"]["abftMismatches"] == 0, (row, col, r)
    r = hip.run(0, zeroInKernel=zero_in_kernel, **PROBE)   # the reused arena holds no fault
    assert r["passed"] and r["mfma"]["abftMismatches"] == 0 and r["mfma"]["elementMismatches"] == 0, r


@pytest.mark.parametrize("dtype", LOWP)
def test_probe_counts_an_injected_lowp_fault_wherever_it_is(hip, dtype):
    for row, col in POSITIONS:
        r = hip.run(0, mfma_low_precision=LOWP, injectLowpFault=1 << LOWP.index(dtype), injectGemmFaultRow=row,
                    injectGemmFaultCol=col, **PROBE)
        assert not r["passed"], (row, col, r)
        for name in LOWP:
            e = r["lowp"][name]
            assert e["abftMismatches"] == (2 if name == dtype else 0) and e["elementMismatches"] == 0, (row, col, name, e)
        assert r["mfma"]["ok"] and r["mfma"]["abftMismatches"] == 0, r["mfma"]
    r = hip.run(0, mfma_low_precision=LOWP, injectLowpFault=1 << LOWP.index(dtype), injectGemmFaultRow=512,
                injectGemmFaultCol=0, **PROBE)
    assert r["passed"] and all(e["abftMismatches"] == 0 for e in r["lowp"].values()), r
    r = hip.run(0, mfma_low_precision=LOWP, **PROBE)
    assert r["passed"] and all(e["ok"] for e in r["lowp"].values()), r
