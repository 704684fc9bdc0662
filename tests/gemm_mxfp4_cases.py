"""Operand builders, a NumPy twin of the quantiser and the reference for the MXFP4 GEMM tests
(native/kernels/gemm_mxfp4.hip).

Plain Python on torch and NumPy, no GPU: ``tests/test_gemm_mxfp4_cases.py`` checks on the CPU that the operands built
here have the properties the GPU tests rely on, ``tests/test_gpu_gemm_mxfp4.py`` and ``tests/test_gpu_quant_mxfp4.py``
feed them to the kernels.  The comparison is ``tests/gemm_cases.py``'s: the raw 16 bits of every element.

The format is gsx_kernels.h's.  An operand is a pair ``(q, s)``: ``q`` uint8 ``[rows][K / 2]``, two e2m1 codes per
byte, element k in byte k / 2, low nibble for even k (``torch.float4_e2m1fn_x2``); ``s`` uint8 ``[rows][K / 32]``,
e8m0 (``torch.float8_e8m0fnu``): code c is 2^(c - 127) for elements 32 g .. 32 g + 31 of its row.  The builders work
on one e2m1 code per byte (``[rows][K]``, 0..15) and ``pack`` them at the end.

The reference is the fp64 value of

    C[i][j] = sum_g 2^(sa[i][g] - 127) 2^(sb[j][g] - 127) sum_{k in block g} A[i][k] B[j][k]

rounded once to fp32 and then to bf16.  Every case satisfies the exactness condition that ``exactness`` checks: all
terms of a dot product, scales included, are multiples of one unit u, the sum of their magnitudes is below 2^24 u,
and u and that sum are normal fp32 numbers.  Then every partial sum in any order is exact in fp32, and so is any
aligner that keeps 24 bits: what the kernel has to produce is the reference, bit for bit.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests import gemm_cases as gc

E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])  # the magnitudes of codes 0..7; bit 3 is the sign
MIDPOINTS = (E2M1[:-1] + E2M1[1:]) / 2
BLOCK = 32
BK = 256  # a K-tile of the kernels
A_BAND, S_BAND = 0x77, 0xFE  # the guard bands: two +6.0 around A and B, the largest code around the scales


# ---- the format ------------------------------------------------------------------------------------------------

def values(codes: np.ndarray) -> np.ndarray:
    """fp64 values of e2m1 codes 0..15."""
    codes = np.asarray(codes)
    return np.where(codes & 8, -1.0, 1.0) * E2M1[codes & 7]


def pack(codes: np.ndarray) -> np.ndarray:
    """``[rows][K]`` codes -> ``[rows][K / 2]`` bytes: even k in the low nibble."""
    codes = np.asarray(codes, dtype=np.uint8)
    assert codes.ndim == 2 and codes.shape[1] % 2 == 0 and int(codes.max(initial=0)) < 16
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)


def unpack(q: np.ndarray) -> np.ndarray:
    q = np.asarray(q, dtype=np.uint8)
    out = np.empty((q.shape[0], q.shape[1] * 2), dtype=np.uint8)
    out[:, 0::2], out[:, 1::2] = q & 15, q >> 4
    return out


def dequant(codes: np.ndarray, s: np.ndarray) -> np.ndarray:
    """fp64 ``[rows][K]``: the value of every element with its block scale applied (exact)."""
    assert s.shape == (codes.shape[0], codes.shape[1] // BLOCK)
    return values(codes) * np.repeat(np.ldexp(1.0, s.astype(np.int64) - 127), BLOCK, axis=1)


def reference(ac, sa, bc, sb) -> torch.Tensor:
    """The formula above in fp64 (exact for every case here), rounded once to fp32 and then to bf16."""
    acc = torch.from_numpy(dequant(ac, sa)) @ torch.from_numpy(dequant(bc, sb)).t()
    return acc.float().bfloat16()


def accumulator(ac, sa, bc, sb) -> torch.Tensor:
    return (torch.from_numpy(dequant(ac, sa)) @ torch.from_numpy(dequant(bc, sb)).t()).float()


def exactness(ac, sa, bc, sb) -> dict:
    """What the exactness condition needs, for the case's worst dot product.  The unit of (i, j) is a quarter of the
    smallest scale product 2^(sa[i][g] + sb[j][g] - 254) among the blocks g in which both rows hold a nonzero: every
    nonzero term is a multiple of it (products of e2m1 values are multiples of 1/4).  Where that minimum over (i, j,
    g) is too large a table, the smaller 2^(min_g sa[i][g] + min_g sb[j][g] - 254) / 4 stands in, which asks for more.
    Returns the largest ``sum|terms| / unit`` (has to be below 2^24), the smallest unit and the largest sum of
    magnitudes (have to be normal fp32)."""
    nb = sa.shape[1]
    if ac.shape[0] * bc.shape[0] * nb <= 1 << 25:
        far = 1 << 12  # a block of zeros does not count
        ea = np.where((ac.reshape(ac.shape[0], nb, BLOCK) & 7).any(axis=2), sa.astype(np.int32), far)
        eb = np.where((bc.reshape(bc.shape[0], nb, BLOCK) & 7).any(axis=2), sb.astype(np.int32), far)
        e = (ea[:, None, :] + eb[None, :, :]).min(axis=2)
        unit = np.ldexp(1.0, np.where(e >= far, 254, e) - 254) / 4
    else:
        ua = np.ldexp(1.0, sa.astype(np.int64).min(axis=1) - 127)
        ub = np.ldexp(1.0, sb.astype(np.int64).min(axis=1) - 127)
        unit = ua[:, None] * ub[None, :] / 4
    mag = (torch.from_numpy(np.abs(dequant(ac, sa))) @ torch.from_numpy(np.abs(dequant(bc, sb))).t()).numpy()
    return {"units": float((mag / unit).max()), "min_unit": float(unit.min()), "max_sum": float(mag.max())}


def assert_bits_equal(got: torch.Tensor, want: torch.Tensor, what: str = "", zeros_by_value: bool = False) -> None:
    """``gemm_cases.assert_bits_equal``; with ``zeros_by_value`` a zero of either sign is accepted wherever ``want``
    is a zero."""
    got = got.cpu()
    if zeros_by_value:
        both_zero = ((gc.bits(got) & 0x7FFF) == 0) & ((gc.bits(want) & 0x7FFF) == 0)
        got = torch.where(both_zero, want, got)
    gc.assert_bits_equal(got, want, what)


class Case:
    """One problem: codes and scales of A and B on the host and the bf16 result wanted.  Built once and shared: not
    to be written to."""

    def __init__(self, ac, sa, bc, sb):
        self.ac, self.sa, self.bc, self.sb = (np.ascontiguousarray(x, dtype=np.uint8) for x in (ac, sa, bc, sb))
        self.m, self.k = self.ac.shape
        self.n = self.bc.shape[0]
        assert self.bc.shape[1] == self.k and self.k % BK == 0
        assert 1 <= int(min(self.sa.min(), self.sb.min())) and int(max(self.sa.max(), self.sb.max())) <= 254
        self.aq, self.bq = pack(self.ac), pack(self.bc)

    @functools.cached_property
    def want(self) -> torch.Tensor:
        return reference(self.ac, self.sa, self.bc, self.sb)

    @functools.cached_property
    def want_unit(self) -> torch.Tensor:
        """What the ablation configuration computes: every scale taken as 127."""
        one = np.full_like(self.sa, 127), np.full_like(self.sb, 127)
        return reference(self.ac, one[0], self.bc, one[1])


# ---- the exact generator ---------------------------------------------------------------------------------------

def _rng(*key) -> np.random.Generator:
    return np.random.default_rng([0x4D58, *key])


@functools.lru_cache(maxsize=None)
def exact_case(m: int, n: int, k: int) -> Case:
    """Random codes (all 16) and random scales ``base[row] + d[row][g]``: the per-row bases move whole rows and
    columns across the e8m0 range (66 .. 179, so that units and sums stay normal fp32: the sum of two bases is in
    132 .. 358), and ``d`` spreads the blocks of a row over 0 .. D, D = 2 up to K = 4096 and 1 beyond.  The
    combined exponents inside one dot product then spread over 2 D bits; with |products| at most 36 = 144 quarters
    the magnitudes sum to less than 2^24 units (checked, not assumed, by ``exactness``)."""
    r = _rng(m, n, k)
    d = 2 if k <= 4096 else 1
    ac = r.integers(0, 16, size=(m, k), dtype=np.uint8)
    bc = r.integers(0, 16, size=(n, k), dtype=np.uint8)
    sa = r.integers(66, 180 - d, size=(m, 1)) + r.integers(0, d + 1, size=(m, k // BLOCK))
    sb = r.integers(66, 180 - d, size=(n, 1)) + r.integers(0, d + 1, size=(n, k // BLOCK))
    return Case(ac, sa, bc, sb)


# ---- every e2m1 code at every k position of a K-tile -------------------------------------------------------------

SWEEP_M, SWEEP_N, SWEEP_K = 16 * BK, 256, 2 * BK
SWEEP_E = (-1, 0, 1, 2)  # the powers of two e2m1 holds


def sweep_k_of_row(i: int) -> int:
    """Row ``i = 16 pos + code`` of A holds its code at position ``pos`` of a K-tile; which of the two tiles
    alternates, so that both LDS buffers carry codes."""
    pos, code = divmod(i, 16)
    return pos + BK * ((pos + code) & 1)


@functools.lru_cache(maxsize=None)
def code_sweep() -> Case:
    """4096 x 256 x 512: row ``16 pos + code`` of A holds ``code`` at one k (``sweep_k_of_row``) and +0 elsewhere, so
    every code sits at every position of a K-tile, in both nibbles; row ``j`` of B holds ``(-1)^j 2^e`` at every k,
    ``e = SWEEP_E[(j // 2) % 4]``.  ``C[i][j]`` is one product times the two block scales (small functions of the row
    and the block): exact in bf16."""
    ac = np.zeros((SWEEP_M, SWEEP_K), dtype=np.uint8)
    for i in range(SWEEP_M):
        ac[i, sweep_k_of_row(i)] = i % 16
    pow_code = {-1: 1, 0: 2, 1: 4, 2: 6}
    col = np.array([pow_code[SWEEP_E[(j // 2) % 4]] | (8 if j & 1 else 0) for j in range(SWEEP_N)], dtype=np.uint8)
    bc = np.repeat(col[:, None], SWEEP_K, axis=1)
    g = np.arange(SWEEP_K // BLOCK)[None, :]
    sa = 120 + (np.arange(SWEEP_M)[:, None] // 16 + 3 * g) % 13
    sb = 124 + (np.arange(SWEEP_N)[:, None] + 5 * g) % 7
    return Case(ac, sa, bc, sb)


# ---- k positions: A's and B's operand paths must agree ------------------------------------------------------------

SLOT_M = SLOT_N = 512
SLOT_K = 256


@functools.lru_cache(maxsize=None)
def k_slot_case() -> Case:
    """512 x 512 x 256: ``A[i][k] = u_i`` where ``k = i mod 256`` and ``B[j][k] = v_j`` where ``k = j mod 256``, +0
    elsewhere, u and v positive e2m1 values with periods 7 and 5.  ``C[i][j]`` is nonzero only where ``i = j (mod
    256)``: a k position that the two operand paths place differently moves or removes the entry of a named row and
    column."""
    ac = np.zeros((SLOT_M, SLOT_K), dtype=np.uint8)
    bc = np.zeros((SLOT_N, SLOT_K), dtype=np.uint8)
    i = np.arange(SLOT_M)
    ac[i, i % SLOT_K] = 1 + (3 * i) % 7
    bc[i, i % SLOT_K] = 1 + (2 * i) % 5
    g = np.arange(SLOT_K // BLOCK)[None, :]
    sa = 125 + (i[:, None] + g) % 3
    sb = 126 + (i[:, None] // 2 + 2 * g) % 5
    return Case(ac, sa, bc, sb)


# ---- which scale byte a (row, block) really gets --------------------------------------------------------------------

SCALE_SLOT_M = SCALE_SLOT_N = 512


def slot_scale_a(i, g):
    return 112 + (7 * i + 3 * g) % 16


def slot_scale_b(j, g):
    return 131 + (5 * j + 11 * g) % 13


@functools.lru_cache(maxsize=None)
def scale_slot_case(k: int) -> Case:
    """512 x 512 x k: A is all ones; row ``j`` of B is ones in block ``g_j = j mod (k / 32)`` and +0 elsewhere.  So
    ``C[i][j] = 32 * 2^(sa[i][g_j] + sb[j][g_j] - 254)``: a power of two that names the scale bytes the block of row i
    and of column j really got.  ``sa`` and ``sb`` differ between neighbouring rows, neighbouring blocks, the two
    halves of a K-tile and consecutive K-tiles, and between A and B (their ranges do not overlap)."""
    nb = k // BLOCK
    ac = np.full((SCALE_SLOT_M, k), 2, dtype=np.uint8)
    bc = np.zeros((SCALE_SLOT_N, k), dtype=np.uint8)
    for j in range(SCALE_SLOT_N):
        g = j % nb
        bc[j, BLOCK * g:BLOCK * (g + 1)] = 2
    g = np.arange(nb)[None, :]
    sa = slot_scale_a(np.arange(SCALE_SLOT_M)[:, None], g)
    sb = slot_scale_b(np.arange(SCALE_SLOT_N)[:, None], g)
    return Case(ac, sa, bc, sb)


# ---- every e8m0 code ---------------------------------------------------------------------------------------------

E8_M = E8_N = 256
E8_K = 8192  # 256 blocks: one for each code and three more


@functools.lru_cache(maxsize=None)
def e8m0_sweep() -> Case:
    """256 x 256 x 8192, random codes: ``sa[i][g] = s(g) + (i & 1)`` and ``sb[j][g] = 255 - s(g) - (j & 1)`` with
    ``s(g) = 1 + g mod 253``.  Both arrays hold every code 1 .. 254, and the combined exponent of (i, j) is
    ``1 + (i & 1) - (j & 1)`` in every block: one unit per dot product."""
    r = _rng(8, 8, 8)
    ac = r.integers(0, 16, size=(E8_M, E8_K), dtype=np.uint8)
    bc = r.integers(0, 16, size=(E8_N, E8_K), dtype=np.uint8)
    s = 1 + np.arange(E8_K // BLOCK)[None, :] % 253
    sa = s + (np.arange(E8_M)[:, None] & 1)
    sb = 255 - s - (np.arange(E8_N)[:, None] & 1)
    return Case(ac, sa, bc, sb)


# ---- guard bands -----------------------------------------------------------------------------------------------

def banded(payload: np.ndarray, fill: int, device) -> tuple[torch.Tensor, torch.Tensor]:
    """``(whole, view)``: the uint8 ``payload`` inside an allocation whose other bytes hold ``fill``, ``BAND + 16``
    bytes in, so 16-B aligned and no more."""
    t = torch.from_numpy(np.ascontiguousarray(payload))
    n, lead = t.numel(), gc.BAND + 16
    whole = torch.full((lead + n + gc.BAND,), fill, dtype=torch.uint8, device=device)
    assert whole.data_ptr() % 32 == 0
    view = whole[lead:lead + n].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 32 == 16
    return whole, view


# ---- the quantiser's twin ------------------------------------------------------------------------------------------

def bf16_values(xbits: np.ndarray) -> np.ndarray:
    """fp64 values of raw bf16 words."""
    return (np.asarray(xbits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def quant_twin(xbits: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """The definition of ``gsx_quant_mxfp4``: raw bf16 words ``[R][K]`` -> ``(q [R][K / 2], s [R][K / 32])``.  Per
    block, ``e = floor(log2(max|x|)) - 2`` and the code is ``clamp(e + 127, 1, 254)``; elements are ``x / 2^(code -
    127)`` rounded to the nearest e2m1 value, a tie to the even code, saturated to +-6, the sign kept (of a zero
    too).  An all-zero block gets 127; a block with an inf or a NaN gets 255, and its elements are not defined (here:
    zeros with the sign)."""
    xbits = np.asarray(xbits, dtype=np.uint16)
    r, k = xbits.shape
    assert k % BLOCK == 0
    x = bf16_values(xbits).reshape(r, k // BLOCK, BLOCK)
    bad = ~np.isfinite(x).all(axis=2)
    mx = np.where(bad, 0.0, np.abs(np.where(np.isfinite(x), x, 0.0)).max(axis=2))
    floor_log2 = np.frexp(mx)[1] - 1  # exact; meaningless where mx == 0
    s = np.clip(floor_log2 - 2 + 127, 1, 254)
    s = np.where(mx == 0, 127, s)
    y = np.abs(np.where(np.isfinite(x), x, 0.0)) * np.ldexp(1.0, 127 - s)[:, :, None]  # exact in fp64
    code = np.searchsorted(MIDPOINTS, y, side="left")  # the midpoints below y: the lower neighbour on a tie
    tie = np.isin(y, MIDPOINTS)
    code = code + (tie & (code & 1 == 1))  # a tie goes to the even code
    code = np.where(bad[:, :, None], 0, code)
    code = code.astype(np.uint8) | ((xbits.reshape(x.shape) >> 12) & 8).astype(np.uint8)
    s = np.where(bad, 255, s).astype(np.uint8)
    return pack(code.reshape(r, k)), s


def bf16_bits(x: np.ndarray) -> np.ndarray:
    """Raw bf16 words of fp64 values that bf16 holds exactly."""
    f = np.asarray(x, dtype=np.float32)
    assert (f.astype(np.float64) == np.asarray(x, dtype=np.float64)).all()
    w = f.view(np.uint32)
    assert not (w & 0xFFFF).any()
    return (w >> 16).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def lossless_inputs(rows: int, k: int, seed: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(xbits, codes, s)``: bf16 inputs that quantise without loss.  Every block holds e2m1 grid values times
    2^e, with at least one element of magnitude 4 or 6 so that the quantiser picks exactly ``e`` (``floor(log2(4 or
    6)) = 2``); ``e`` is a per-row base plus 0 or 1 per block, as in ``exact_case``."""
    r = _rng(rows, k, seed)
    codes = r.integers(0, 16, size=(rows, k), dtype=np.uint8)
    nb = k // BLOCK
    top = r.integers(0, BLOCK, size=(rows, nb))
    idx = (np.arange(nb)[None, :] * BLOCK + top)
    rr = np.repeat(np.arange(rows)[:, None], nb, axis=1)
    codes[rr, idx] = r.choice(np.array([6, 7, 14, 15], dtype=np.uint8), size=(rows, nb))
    s = (r.integers(100, 150, size=(rows, 1)) + r.integers(0, 2, size=(rows, nb))).astype(np.uint8)
    return bf16_bits(dequant(codes, s)), codes, s
