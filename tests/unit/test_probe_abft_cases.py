"""The host references of the probe's checker kernels (tests/gpu/abft_cases.py) against each other,
on the CPU: the checksum identities hold on clean data at every shape the GPU tests use, the count
predictor answers the corruptions whose answer is known by construction, and the generator replica
reproduces values computed by the C++ ``pattern_word`` itself."""
from __future__ import annotations

import numpy as np
import pytest

from tests.gpu import abft_cases as ac

CASES = [(d, s, k) for d in ac.DTYPES for s in ac.shapes(d) for k in ("probe", "max")]

# (index, seed, value): hbm.h's __host__ pattern_word, compiled for the CPU and printed once
PATTERN_WORDS = (
    (0x0, 0x0, 0x00000000), (0x1, 0x0, 0xc80d83e3), (0x2, 0x0, 0x34f40b27),
    (0x7ffff, 0x0, 0xe15030b4), (0x80000, 0x0, 0xde932c3c), (0xffffffff, 0x0, 0x190e577a),
    (0x100000000, 0x0, 0xf63a927f), (0x123456789, 0x0, 0x624e9308),
    (0x0, 0x51, 0xf491579c), (0x1, 0x51, 0xd36fd358), (0x80000, 0x51, 0x4fd1abf8),
    (0x100000000, 0x51, 0xeadaa2dd), (0x123456789, 0x51, 0xfebfb623),
    (0x0, 0x1234, 0xdfca0c5b), (0x2, 0x1234, 0xbcb73fe0), (0xffffffff, 0x1234, 0x14970fc6),
    (0x123456789, 0x1234, 0xda6a0e85),
    (0x1, 0xbeef, 0x2a71c8eb), (0x7ffff, 0xbeef, 0xbf289c36), (0x100000000, 0xbeef, 0xcfe482b1),
    (0x0, 0x10F0 ^ 0x5CA1E, 0xd3ffe0ac), (0x123456789, 0x10F0 ^ 0x5CA1E, 0x0922f0a4),
)


def test_pattern_word_replica_reproduces_the_cpp_function():
    for idx, seed, want in PATTERN_WORDS:
        assert int(ac.pattern_word(np.array([idx], dtype=np.uint64), seed)[0]) == want, (hex(idx), hex(seed))
    idx = np.array([p[0] for p in PATTERN_WORDS if p[1] == 0x51], dtype=np.uint64)
    assert ac.pattern_word(idx, 0x51).tolist() == [p[2] for p in PATTERN_WORDS if p[1] == 0x51]


def test_small_int_bf16_is_the_exact_encoding():
    h = np.arange(0, 50, dtype=np.uint32)
    for span in (2, 3, 8):
        v = ac.small_int(h, span)
        assert v.min() == -span and v.max() == span and len(set(v.tolist())) == 2 * span + 1
        bits = ac.small_int_bf16(h, span)
        assert (ac.gemm_cases.bf16_value(bits) == v).all()
    assert int(ac.small_int_bf16(np.array([0xFFFFFFFF], dtype=np.uint32), 3)[0]) == \
        int(ac.gemm_cases.bf16_bits(np.array([0xFFFFFFFF % 7 - 3], dtype=np.float32))[0])


@pytest.mark.parametrize("dtype", ac.lowp.DTYPES)
def test_lowp_generator_replica_is_in_range(dtype):
    seed = ac.lowp_seeds(dtype)[2]
    data, scales = ac.gen_lowp(dtype, 64 * 1024, seed, ac.SCALE_LO[dtype])
    assert data.dtype == np.uint8 and len(data) == 64 * 1024 * ac.lowp.BITS[dtype] // 8
    if ac.lowp.BITS[dtype] == 8:
        v = ac.lowp.e4m3_decode(data)
        assert set(v.tolist()) == set(range(-8, 9))
    else:
        assert set(ac.lowp.unpack_fp4(data).tolist()) == set(range(16))
    if ac.lowp.SCALED[dtype]:
        lo = 127 + ac.SCALE_LO[dtype]
        assert len(scales) == 2048 and set(scales.tolist()) == {lo, lo + 1}
    else:
        assert scales is None


@pytest.mark.parametrize("dtype,shape,kind", CASES, ids=lambda x: x if isinstance(x, str) else "x".join(map(str, x)))
def test_identities_hold_on_clean_data(dtype, shape, kind):
    o = ac.operands(dtype, shape, kind)
    v = ac.clean_vectors(o)
    m, n, k = shape
    assert [len(x) for x in (v.acol, v.bcol, v.col_c, v.exp_col, v.row_c, v.exp_row)] == [k, k, n, n, m, m]
    assert (v.col_c == v.exp_col).all() and (v.row_c == v.exp_row).all()
    # against Python integers of unbounded size
    for j in {0, n - 1, n // 2}:
        want = sum(int(x) * int(y) for x, y in zip(o.bt_int[j], o.a_int.sum(axis=0))) % (1 << 32)
        assert int(v.exp_col[j]) == want == int(o.c_int[:, j].sum()) % (1 << 32)
    for i in {0, m - 1, m // 2}:
        want = sum(int(x) * int(y) for x, y in zip(o.a_int[i], o.bt_int.sum(axis=0))) % (1 << 32)
        assert int(v.exp_row[i]) == want == int(o.c_int[i].sum()) % (1 << 32)
    assert ac.predict_counts(o, o.c) == (0, 0, 0)
    if kind == "max":   # every sum is a large positive number, nothing cancels
        assert int(o.c_int.min()) == k * ac.SPAN[dtype] ** 2 == int(o.bound)
    elif m * k >= 64:   # signed operands: negative sums that wrap
        assert (o.a_int < 0).any() and (o.bt_int < 0).any()
        assert len(set(o.a_int.ravel().tolist())) > 2 and not np.array_equal(o.a_int[:1, :8], o.bt_int[:1, :8])


def test_negative_sums_wrap_in_the_vectors():
    o = ac.operands(ac.BF16, (65, 1028, 2056))
    v = ac.clean_vectors(o)
    assert (o.a_int.sum(axis=0) < 0).any() and (o.c_int.sum(axis=0) < 0).any()
    j = int(np.argmin(o.c_int.sum(axis=0)))
    assert int(v.col_c[j]) == int(o.c_int[:, j].sum()) + (1 << 32)


def test_predictor_on_known_corruptions():
    o = ac.operands(ac.BF16, (65, 1028, 2056))
    m, n, _ = o.shape
    neg = tuple(int(x) for x in np.argwhere(o.c_int < 0)[0])
    pos = tuple(int(x) for x in np.argwhere(o.c_int > 0)[0])

    def one(at, f):
        c = o.c
        c[at] = f(c[at])
        return ac.predict_counts(o, c)
    for at in (neg, pos, (0, 0), (m - 1, n - 1)):
        assert one(at, lambda x: x + np.float32(1)) == (0, 1, 1)
        assert one(at, lambda x: x + np.float32(0.25)) == (1, 0, 0)     # the integer part survives
        assert one(at, lambda x: np.float32("nan"))[0] == 1
        assert one(at, lambda x: np.float32("inf"))[0] == 1
        assert one(at, lambda x: np.float32(3e9))[0] == 1
        assert one(at, lambda x: np.float32(o.bound + 1)) == (1, 1, 1)
    c = o.c
    c[3, 5] += 1
    c[3, 900] -= 1
    assert ac.predict_counts(o, c) == (0, 2, 0)      # the row's sum is unchanged
    c = o.c
    c[3, 5] += 1
    c[64, 5] -= 1
    assert ac.predict_counts(o, c) == (0, 0, 2)      # the column's sum is unchanged
    c = o.c
    c[7] += 1
    assert ac.predict_counts(o, c) == (0, n, 1)
    c = o.c
    c[[2, 40]] = c[[40, 2]]
    odd, cols, rows = ac.predict_counts(o, c)
    assert (odd, cols) == (0, 0) and rows == 2 * (o.c_int[2].sum() != o.c_int[40].sum())
    c = o.c
    c[0, 0] += np.float32(2.0 ** 32 / 2 ** 9)        # 2^23: an integer, within fp32, beyond the bound
    assert ac.predict_counts(o, c) == (1, 1, 1)


def test_transposed_square_c_is_caught():
    o = ac.operands(ac.BF16, (256, 256, 256))
    odd, cols, rows = ac.predict_counts(o, np.ascontiguousarray(o.c.T))
    assert odd == 0 and cols > 0 and rows > 0


def test_fault_positions_cover_every_class():
    for m, n in ((512, 512), (65, 1028)):
        pos = ac.fault_positions(m, n)
        assert {r % 64 for r, _ in pos} == set(range(min(64, m)))
        edges = set(range(0, n, 256)) | {n}
        for e in edges:
            for c in range(e - 16, e + 16):
                if 0 <= c < n:
                    assert any(q == c for _, q in pos), (e, c)
        assert {(0, 0), (0, n - 1), (m - 1, 0), (m - 1, n - 1)} <= set(pos)
        assert all(0 <= r < m and 0 <= c < n for r, c in pos) and len(pos) < 1000
