"""Cases, operands and the comparer of the probe GEMM variant tests. Needs no GPU and no torch:
``test_probe_gemm_variants_gpu.py`` runs the cases on an MI355X, ``tests/unit/
test_probe_gemm_cases.py`` checks on the CPU that the cases reach what they claim to reach and
that the comparer flags the ways a tiled MFMA kernel goes wrong.

C[m][n] (fp32) = A[m][k] (bf16) x Bt[n][k]^T (bf16), both operands row-major. bf16 values travel
as uint16 bit patterns (numpy has no bf16).

Two kinds of data per shape:

``exact``     integers drawn uniformly from [-127, 127]: every value is exact in bf16 (8 significant
              bits) and, with K <= 448, |C| <= 448 * 127^2 = 7 225 792 < 2^24, so every partial sum
              in any order is an integer below 2^24, exact in fp32. The kernel must return the
              float64 reference bit for bit: no tolerance.
``rounding``  standard normal values rounded to bf16. The products are exact in fp32 (8 x 8
              significant bits); each of the K additions loses at most one unit in the last place of
              an fp32 partial sum no larger than sum_k |a||b|, under either rounding mode, so
              |C - ref| <= K * 2^-23 * (|A| @ |Bt|^T) element by element, in float64.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

POISON_BITS = 0xFFFFFFFF  # what ``poison_c`` leaves in an unwritten element (a NaN)
KINDS = ("exact", "rounding")


@dataclasses.dataclass(frozen=True)
class Variant:
    name: str
    tile: int           # edge of the block tile: 256 | 128
    bk: int             # K-tile of the kernel: 64 | 32
    opts: tuple         # keyword options of gpupool.ops.probe.gemm_bf16, as sorted items
    pipelined: bool     # DMA in flight across barriers: run several times


def _v(name, tile, pipelined=False, **opts):
    return Variant(name, tile, 64 if tile == 256 else 32, tuple(sorted(opts.items())), pipelined)


VARIANTS = (
    _v("tile128", 128, gemm_tile=128),
    _v("pipe0", 256, gemm_pipe=0),
    _v("pipe0-prio", 256, gemm_pipe=0, gemm_prio=1),
    _v("pipe0-vecc", 256, gemm_pipe=0, gemm_vec_c=1),
    _v("pipe1", 256, True, gemm_pipe=1),
    _v("pipe2", 256, True, gemm_pipe=2),
    _v("pipe21", 256, True, gemm_pipe=21),
    _v("pipe22", 256, True, gemm_pipe=22),
    _v("pipe3", 256, True, gemm_pipe=3),
)

# (m, n, k): the smallest shapes that reach each path
SHAPES_256 = (
    (256, 256, 64),     # 1 K-tile: prologue + last tile only
    (256, 256, 128),    # 2 K-tiles
    (256, 512, 192),    # 3 K-tiles, odd-parity buffer flip
    (768, 256, 320),    # 5 K-tiles, 3x1 tiles
    (512, 1536, 448),   # 7 K-tiles, 2x6 tiles: an XCD's range spans two tile-row groups
    (1280, 768, 192),   # 5x3 tiles: short last group, 15 workgroups (no multiple of 8)
)
SHAPES_128 = ((128, 128, 32), (128, 256, 64), (384, 128, 96), (640, 384, 160))
GROUPED_SHAPES = ((1280, 768, 192), (512, 1536, 448))
GROUPS = (0, 2, 3, 4, 8)


@dataclasses.dataclass(frozen=True)
class Case:
    variant: Variant
    shape: tuple
    group_m: int | None  # None: the kernel's default tile order

    @property
    def id(self) -> str:
        g = "" if self.group_m is None else f"-g{self.group_m}"
        return f"{self.variant.name}-{'x'.join(map(str, self.shape))}{g}"

    @property
    def opts(self) -> dict:
        o = dict(self.variant.opts)
        if self.group_m is not None:
            o["gemm_group_m"] = self.group_m
        return o


def _cases():
    out = []
    for v in VARIANTS:
        if v.tile == 128:  # no tile order option
            out += [Case(v, s, None) for s in SHAPES_128]
            continue
        for s in SHAPES_256:
            out += [Case(v, s, g) for g in (GROUPS if s in GROUPED_SHAPES else (None,))]
    return tuple(out)


CASES = _cases()


# ------------------------------------------------------------------ bf16 <-> float32, host side
def bf16_bits(x: np.ndarray) -> np.ndarray:
    """float32 -> bf16 bit patterns (uint16), round to nearest even. Finite inputs only."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u += 0x7FFF + ((u >> 16) & 1)
    return (u >> 16).astype(np.uint16)


def bf16_value(bits: np.ndarray) -> np.ndarray:
    """bf16 bit patterns (uint16) -> the float32 they denote."""
    return (bits.astype(np.uint32) << 16).view(np.float32)


@dataclasses.dataclass(frozen=True)
class Data:
    kind: str
    shape: tuple
    a: np.ndarray      # [m][k] uint16, bf16 bits
    bt: np.ndarray     # [n][k] uint16, bf16 bits
    ref: np.ndarray    # [m][n] float64: A @ Bt^T of the bf16 values
    bound: np.ndarray | None  # [m][n] float64 error bound (``rounding``), None: exact


def _raw_operands(shape, kind):
    m, n, k = shape
    rng = np.random.default_rng([m, n, k, KINDS.index(kind)])
    if kind == "exact":
        a = rng.integers(-127, 128, size=(m, k)).astype(np.float32)
        bt = rng.integers(-127, 128, size=(n, k)).astype(np.float32)
    else:
        a = rng.standard_normal((m, k), dtype=np.float32)
        bt = rng.standard_normal((n, k), dtype=np.float32)
    return a, bt


@functools.lru_cache(maxsize=None)
def data(shape: tuple, kind: str) -> Data:
    """Operands and reference of one shape and kind: computed once, shared, read-only."""
    a32, bt32 = _raw_operands(shape, kind)
    a, bt = bf16_bits(a32), bf16_bits(bt32)
    a64, bt64 = bf16_value(a).astype(np.float64), bf16_value(bt).astype(np.float64)
    ref = a64 @ bt64.T
    bound = None
    if kind == "rounding":
        bound = shape[2] * 2.0 ** -23 * (np.abs(a64) @ np.abs(bt64).T)
    for x in (a, bt, ref, bound):
        if x is not None:
            x.setflags(write=False)
    return Data(kind, shape, a, bt, ref, bound)


def poisoned_c(m: int, n: int) -> np.ndarray:
    """A host C of all-ones words: a copy-back that never happened shows as the poison too."""
    return np.full((m, n), POISON_BITS, dtype=np.uint32).view(np.float32)


# ------------------------------------------------------------------ the comparer
@dataclasses.dataclass(frozen=True)
class Verdict:
    ok: bool
    message: str
    max_ratio: float  # ``rounding``: largest |C - ref| / bound; ``exact``: 0.0 or inf


def check(c: np.ndarray, d: Data, tile: int, show: int = 6) -> Verdict:
    """Compare a kernel's C with the reference of ``d``: every element, exact (``exact``) or inside
    the per-element bound (``rounding``), and all finite. The message of a failure names the count
    of wrong elements, the first few as (tile_m, tile_n, row in tile, col in tile), and whether
    the wrong values are the poison."""
    m, n, _ = d.shape
    assert c.shape == (m, n) and c.dtype == np.float32, (c.shape, c.dtype)
    c64 = c.astype(np.float64)
    finite = np.isfinite(c)
    with np.errstate(invalid="ignore"):
        err = np.abs(c64 - d.ref)
        if d.bound is None:
            wrong = ~(c64 == d.ref)  # NaN compares unequal
            max_ratio = float("inf") if wrong.any() else 0.0
        else:
            wrong = ~(err <= d.bound)  # NaN fails
            ratio = np.where(finite & (d.bound > 0), err / np.where(d.bound > 0, d.bound, 1.0), 0.0)
            max_ratio = float(ratio.max())
    wrong |= ~finite
    count = int(wrong.sum())
    if count == 0:
        return Verdict(True, "", max_ratio)
    rows, cols = np.nonzero(wrong)
    bits = c.view(np.uint32)[rows, cols]
    poison = int((bits == POISON_BITS).sum())
    where = [(int(r) // tile, int(q) // tile, int(r) % tile, int(q) % tile)
             for r, q in zip(rows[:show], cols[:show])]
    tiles = sorted({(int(r) // tile, int(q) // tile) for r, q in zip(rows, cols)})
    vals = [(float(c[r, q]), float(d.ref[r, q])) for r, q in zip(rows[:show], cols[:show])]
    if poison == count:
        what = "all of them the poison (never written)"
    elif poison:
        what = f"{poison} of them the poison (never written), {count - poison} written wrong"
    else:
        what = "none of them the poison (written, but wrong)"
    msg = (f"{d.kind} {d.shape}: {count} of {m * n} elements wrong, {what}; "
           f"{int((~finite).sum())} not finite; in {len(tiles)} tile(s) {tiles[:show]}; "
           f"first (tile_m, tile_n, row, col): {where}; (got, want): {vals}")
    return Verdict(False, msg, max_ratio)
