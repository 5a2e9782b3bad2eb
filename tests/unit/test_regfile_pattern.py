"""The numpy twin of the register-file phase's pattern (gpupool/ops/regfile.py): shape, constants,
distinct values across the 512 registers of a lane and across lanes, waves, workgroups and seeds, the
complement, and the arithmetic against a scalar re-implementation of pattern16<1>."""
from __future__ import annotations

import numpy as np
import pytest

from gpupool.ops import hostlink, regfile

SEED = regfile.SEED_BASE ^ 0x5A17


@pytest.fixture(scope="module")
def image():
    e = regfile.expected(0, SEED)
    e.setflags(write=False)
    return e


def _base(workgroup: int, thread: int, seed: int) -> int:
    """pattern16<1>((workgroup << 32) | thread, seed, 0).x, in plain integers."""
    m = 0xFFFFFFFF
    h = ((thread ^ seed) * 0x9E3779B1) & m
    h ^= ((workgroup << 7) | (workgroup >> 25)) & m
    return h ^ (h >> 15)


def test_constants_and_shape(image):
    assert regfile.SEED_BASE == 0x52454700 and regfile.MULTIPLIER == 0x9E3779B1 and regfile.MULTIPLIER & 1
    assert (regfile.WAVES, regfile.REGISTERS, regfile.LANES) == (4, 512, 64)
    assert regfile.IMAGE_BYTES == 4 * 512 * 64 * 4 == image.nbytes
    assert image.shape == (4, 512, 64) and image.dtype == np.uint32
    assert regfile.base_words(0, SEED).shape == (4, 64)


def test_values_follow_the_formula(image):
    for b, w, u, lane in ((0, 0, 0, 0), (0, 3, 511, 63), (0, 1, 16, 31), (0, 2, 256, 32), (0, 0, 255, 1)):
        want = (_base(b, 64 * w + lane, SEED) + u * 0x9E3779B1) & 0xFFFFFFFF
        assert int(image[w, u, lane]) == want, (w, u, lane)
    other = regfile.expected(7, SEED)
    assert int(other[2, 300, 5]) == (_base(7, 64 * 2 + 5, SEED) + 300 * 0x9E3779B1) & 0xFFFFFFFF
    big = regfile.expected(2047, SEED)  # the workgroup sits in the index's high half
    assert int(big[0, 0, 0]) == _base(2047, 0, SEED)
    # register 0 is the base itself: the first word of the shared pattern
    assert (image[:, 0, :].reshape(-1) == hostlink.pattern_words(0, 256, SEED)[:, 0]).all()


def test_registers_of_a_lane_are_distinct(image):
    for w in range(4):
        for lane in range(64):
            assert np.unique(image[w, :, lane]).size == 512, (w, lane)


def test_lanes_waves_workgroups_and_seeds_differ(image):
    for u in (0, 15, 16, 255, 256, 511):
        assert np.unique(image[:, u, :]).size == 256, u  # 4 waves x 64 lanes of one register
    assert np.unique(image).size > 0.99 * image.size  # 32-bit values: a few chance collisions at most
    assert not (regfile.expected(1, SEED) == image).any(axis=1).all()
    assert (regfile.expected(1, SEED)[:, 0, :] != image[:, 0, :]).all()
    assert (regfile.expected(0, SEED ^ 1)[:, 0, :] != image[:, 0, :]).all()  # the salt moves every base


def test_complement_is_the_bitwise_inverse(image):
    c = regfile.expected(0, SEED, 0xFFFFFFFF)
    assert (c == ~image).all() and ((c ^ image) == 0xFFFFFFFF).all()
    assert (regfile.expected(0, SEED, 0) == image).all()


def test_register_names():
    assert [regfile.register_name(u) for u in (0, 17, 255, 256, 259, 511)] == ["v0", "v17", "v255", "a0", "a3", "a255"]
