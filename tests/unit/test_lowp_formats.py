"""The host side of the probe's low-precision checks (gpupool/ops/lowp.py, tests/gpu/lowp_cases.py):
the codecs against torch and the format definitions, the exactness of the GPU tests' operand sets,
and the comparer against the ways a low-precision tiled kernel goes wrong. No GPU."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from gpupool.ops import lowp
from tests.gpu import gemm_cases, lowp_cases


def test_e4m3_matches_torch_on_all_256_bytes():
    b = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(b.copy()).view(torch.float8_e4m3fn).to(torch.float32).numpy()
    got = lowp.e4m3_decode(b)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).sum() == 2
    fin = ~np.isnan(want)
    assert np.array_equal(got[fin].view(np.uint32), want[fin].view(np.uint32))  # -0 included
    assert np.array_equal(lowp.e4m3_encode(got[fin]), b[fin])
    assert float(np.nanmax(got)) == 448.0 and float(got[1]) == 2.0 ** -9  # OCP, not fnuz (240, 2^-10)
    # values between two codes round to nearest, ties to even, and saturate at 448
    x = torch.tensor([0.3, 17.0, 18.0, 19.0, 20.0, 21.0, -1.0625, 447.0, 1e6, -1e6, 2.0 ** -10, 3 * 2.0 ** -10])
    want_b = x.to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    want_b[8:10] = [0x7E, 0xFE]  # torch overflows to NaN where the probe's encoder saturates
    assert np.array_equal(lowp.e4m3_encode(x.numpy()), want_b)


def test_e2m1_table_e8m0_and_nibble_packing():
    assert lowp.e2m1_decode(np.arange(16)).tolist() == \
        [0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6]
    for c in range(16):  # sign 1, exponent 2 (bias 1), mantissa 1
        s, e, m = c >> 3, (c >> 1) & 3, c & 1
        v = (m * 0.5 if e == 0 else (1 + m / 2) * 2.0 ** (e - 1)) * (-1) ** s
        assert float(lowp.E2M1[c]) == v
    assert np.array_equal(lowp.e2m1_encode(lowp.E2M1), np.arange(16))
    assert lowp.e2m1_encode(np.array([2.5, 3.5, 5.0, 7.0, 0.25, -0.75])).tolist() == [4, 6, 6, 7, 0, 10]
    assert lowp.e8m0_decode(np.array([0, 126, 127, 128, 254])).tolist() == \
        [2.0 ** -127, 0.5, 1.0, 2.0, 2.0 ** 127]
    assert np.isnan(lowp.e8m0_decode(np.array([255])))[0]
    assert lowp.e8m0_encode(np.array([-127, -1, 0, 60])).tolist() == [0, 126, 127, 187]
    with pytest.raises(ValueError):
        lowp.e8m0_encode(np.array([128]))
    n = np.random.default_rng(0).integers(0, 16, (5, 64), dtype=np.uint8)
    p = lowp.pack_fp4(n)
    assert p.shape == (5, 32) and np.array_equal(lowp.unpack_fp4(p), n)
    assert lowp.pack_fp4(np.array([0x3, 0xA])).tolist() == [0xA3]  # even k in the low nibble
    with pytest.raises(ValueError):
        lowp.pack_fp4(np.zeros(3, dtype=np.uint8))


def test_dtype_names_and_mask():
    assert lowp.DTYPES == ("fp8", "mxfp8", "mxfp4")
    assert lowp.dtype_mask(("mxfp4", "fp8")) == 5 and lowp.dtype_mask(()) == 0
    assert lowp.mask_names(6) == ["mxfp8", "mxfp4"]
    for bad in (("fp6",), ("fp8", "fp8")):
        with pytest.raises(ValueError):
            lowp.dtype_mask(bad)
    from gpupool.ops import probe
    assert b"mfmaLowPrecision" not in probe._run_opts(1 << 20, True, 512, 2, 1, 256, ())
    assert b'"mfmaLowPrecision": 5' in probe._run_opts(1 << 20, True, 512, 2, 1, 256, (), ("fp8", "mxfp4"))


def test_windows_hold_what_they_claim():
    assert len(lowp_cases.FINITE_E4M3) == 254 and len(lowp_cases.WINDOW_E4M3) == 80
    v = lowp.e4m3_decode(lowp_cases.WINDOW_E4M3).astype(np.float64)
    assert np.abs(v).max() == 15 and np.array_equal(v * 8, np.rint(v * 8))
    for dtype in lowp_cases.DTYPES:
        o = lowp_cases.encodings(dtype)
        codes = lowp.unpack_fp4(o.a) if lowp.BITS[dtype] == 4 else o.a
        want = set(range(16)) if lowp.BITS[dtype] == 4 else set(lowp_cases.FINITE_E4M3.tolist())
        assert set(codes.ravel().tolist()) == want
        for c in want:  # every encoding sits at K positions of every 32-block and both parities
            ks = np.nonzero(codes == c)[1]
            assert set(ks // 32) == {0, 1, 2, 3} and set(ks % 2) == {0, 1}
    p = lowp_cases.perm(np.arange(128))
    assert sorted(p.tolist()) == list(range(128)) and not np.array_equal(p[p], np.arange(128))
    sc = lowp.e8m0_decode(lowp_cases.encodings("mxfp8", True).scale_a)
    assert sc.min() == 2.0 ** -60 and sc.max() == 2.0 ** 60


@pytest.mark.parametrize("shape", lowp_cases.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", lowp_cases.DTYPES)
def test_exact_operands_are_exact_in_fp32(dtype, shape):
    """quantum x bound < 2^24 (worst case for fp8 and mxfp4; for mxfp8, whose worst case does not
    fit, the result and every partial sum in K order of the drawn data), and an fp32 sum of the
    products in shuffled order equals the float64 reference."""
    o = lowp_cases.exact(dtype, shape)
    k, q = shape[2], lowp_cases.QUANTUM[dtype]
    a = lowp.decode_operand(dtype, o.a, o.scale_a)
    b = lowp.decode_operand(dtype, o.bt, o.scale_bt)
    for x in (a, b):  # products are multiples of the quantum, at most PRODUCT_MAX
        assert np.array_equal(x / np.sqrt(q), np.rint(x / np.sqrt(q)))
        assert np.abs(x).max() ** 2 <= lowp_cases.PRODUCT_MAX[dtype]
    if dtype == "mxfp8":
        assert np.abs(o.data.ref).max() / q < 2 ** 24
        rows = slice(0, 16)
        prefix = np.cumsum(a[rows, None, :] * b[None, :, :], axis=2)
        assert np.abs(prefix).max() / q < 2 ** 24
    else:
        assert lowp_cases.PRODUCT_MAX[dtype] * k / q < 2 ** 24
        assert lowp_cases.abs_sum_max(o) / q < 2 ** 24
    rng = np.random.default_rng(7)
    order = rng.permutation(k)
    rows = rng.choice(shape[0], 8, replace=False)
    prod = (a[rows][:, None, order] * b[None, :, order]).astype(np.float32)
    acc = np.zeros(prod.shape[:2], dtype=np.float32)
    for i in range(k):
        acc += prod[:, :, i]
    assert np.array_equal(acc.astype(np.float64), o.data.ref[rows])


def _c(o):
    return o.data.ref.astype(np.float32)


@pytest.mark.parametrize("dtype", lowp_cases.DTYPES)
def test_comparer_accepts_the_reference_and_flags_kernel_faults(dtype):
    shape = (256, 768, 896)
    o = lowp_cases.exact(dtype, shape)
    assert gemm_cases.check(_c(o), o.data, lowp_cases.TILE).ok
    # a transposed 16x16 tile inside one block tile
    c = _c(o).copy()
    c[128:144, 256:272] = c[128:144, 256:272].T.copy()
    v = gemm_cases.check(c, o.data, lowp_cases.TILE)
    assert not v.ok and "(1, 2)" in v.message
    # an unwritten tile
    c = _c(o).copy()
    c[:128, 640:] = gemm_cases.poisoned_c(128, 128)
    assert "all of them the poison" in gemm_cases.check(c, o.data, lowp_cases.TILE).message
    if lowp.SCALED[dtype]:  # one K-block's scale taken from its neighbour (the lane map of the scale)
        sa = o.scale_a.copy()
        sa[:, 5] = np.where(sa[:, 6] == sa[:, 5], sa[:, 5] ^ 1, sa[:, 6])
        bad = lowp.reference(dtype, o.a, o.bt, sa, o.scale_bt).astype(np.float32)
        assert not gemm_cases.check(bad, o.data, lowp_cases.TILE).ok
    if lowp.BITS[dtype] == 4:  # nibbles swapped in every byte of A
        swapped = ((o.a << 4) | (o.a >> 4)).astype(np.uint8)
        bad = lowp.reference(dtype, swapped, o.bt, o.scale_a, o.scale_bt).astype(np.float32)
        assert not gemm_cases.check(bad, o.data, lowp_cases.TILE).ok


@pytest.mark.parametrize("dtype", lowp_cases.DTYPES)
def test_encodings_case_pins_the_lane_nibble_and_scale_maps(dtype):
    """A kernel that reads each lane's K-block from a wrong place computes other single products."""
    o = lowp_cases.encodings(dtype)
    assert gemm_cases.check(_c(o), o.data, lowp_cases.TILE).ok
    codes = lowp.unpack_fp4(o.a) if lowp.BITS[dtype] == 4 else o.a
    pack = lowp.pack_fp4 if lowp.BITS[dtype] == 4 else (lambda x: x)
    blocks = codes.reshape(128, 4, 32)
    wrong = {"K-blocks 1 and 2 swapped": blocks[:, [0, 2, 1, 3]].reshape(128, 128),
             "adjacent elements swapped": codes.reshape(128, 64, 2)[:, :, ::-1].reshape(128, 128)}
    for what, w in wrong.items():
        bad = lowp.reference(dtype, pack(np.ascontiguousarray(w)), o.bt, o.scale_a, o.scale_bt)
        assert not gemm_cases.check(bad.astype(np.float32), o.data, lowp_cases.TILE).ok, what
    if dtype != "fp8":
        # e4m3 as fnuz (bias 8) would halve every normal value; the 2^-60 .. 2^60 run also pins
        # which lane group's scale a K position falls under: the 16 + 16 byte split of the e4m3
        # operand registers puts k = 16 .. 31 under K-block 0's scale, not a lane's own
        s = lowp_cases.encodings(dtype, True)
        assert gemm_cases.check(_c(s), s.data, lowp_cases.TILE).ok
        sa = s.scale_a[:, [0, 0, 1, 1]] if dtype == "mxfp8" else s.scale_a[:, [1, 0, 3, 2]]
        bad = lowp.reference(dtype, s.a, s.bt, np.ascontiguousarray(sa), s.scale_bt).astype(np.float32)
        assert not gemm_cases.check(bad, s.data, lowp_cases.TILE).ok
