"""Operand builders, the reference and the bit-level comparison for the bf16 GEMM tests (native/kernels/gemm.hip).

Plain Python on torch and NumPy, no GPU: ``tests/test_gemm_cases.py`` checks on the CPU that the operands built here
have the properties the GPU tests rely on, ``tests/test_gpu_gemm_edges.py`` feeds them to the kernels.

Every case is built so that the fp64 product of its operands is an fp32 value and every partial sum of the fp32
accumulation, in any order, is exact.  The kernel then has to equal the reference bit for bit: the only rounding
left is the epilogue's one conversion from fp32 to bf16.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np
import torch

BF16_QNAN = 0x7FC0  # what the guard bands of A and B hold
C_BAND = 0xC3C3  # what the guard bands of C hold
BAND = 64 * 1024  # bytes of guard band on either side of an operand


# ---- reference and comparison ----------------------------------------------------------------------------------

def reference(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """``C = A * B^T`` as the fp64 product rounded once to fp32 and once to bf16, on the CPU."""
    return (a.cpu().double() @ b.cpu().double().t()).float().bfloat16()


def bits(t: torch.Tensor) -> torch.Tensor:
    """The raw 16 bits of a bf16 tensor, as int32 in 0..0xFFFF."""
    assert t.dtype == torch.bfloat16
    return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def mismatches(got: torch.Tensor, want: torch.Tensor, zero_by_value_cols=()) -> torch.Tensor:
    """``[row, col]`` of every element of ``got`` that is not what ``want`` asks for.

    Where ``want`` is NaN, ``got`` has to be a NaN with the quiet bit set, of any sign and payload.  Everywhere else
    the 16 bits have to be equal; in the columns listed in ``zero_by_value_cols`` a zero of either sign is accepted
    where ``want`` is a zero.  No element is left out and there is no tolerance."""
    g, w = bits(got.cpu()), bits(want.cpu())
    assert g.shape == w.shape and g.dim() == 2, (g.shape, w.shape)
    w_nan = (w & 0x7FFF) > 0x7F80
    g_qnan = ((g & 0x7FFF) > 0x7F80) & ((g & 0x0040) != 0)
    ok = torch.where(w_nan, g_qnan, g == w)
    for col in zero_by_value_cols:
        ok[:, col] |= ((w[:, col] & 0x7FFF) == 0) & ((g[:, col] & 0x7FFF) == 0)
    return (~ok).nonzero()


def assert_bits_equal(got: torch.Tensor, want: torch.Tensor, what: str = "", zero_by_value_cols=()) -> None:
    bad = mismatches(got, want, zero_by_value_cols)
    if len(bad):
        g, w = bits(got.cpu()), bits(want.cpu())
        first = [f"[{r},{c}] got {int(g[r, c]):#06x} want {int(w[r, c]):#06x}" for r, c in bad[:8].tolist()]
        raise AssertionError(f"{what}: {len(bad)} of {g.numel()} elements differ: " + "; ".join(first))


# ---- the exact generator ---------------------------------------------------------------------------------------

def exact_operands(m: int, n: int, k: int) -> tuple[torch.Tensor, torch.Tensor]:
    """``A[m][k]``, ``B[n][k]`` in bf16 whose product has no rounding before the final conversion: every input is
    q/16 with |q| <= 15, every product a multiple of 2^-8 below 1, and every partial sum stays below ``k`` in
    multiples of 2^-8, which fp32 holds exactly while ``k <= 2^16``.  Periods 31 and 29 along the rows and the
    coprime steps along k put different data under every tile."""
    assert k <= 1 << 16
    i, j = torch.arange(m).unsqueeze(1), torch.arange(k).unsqueeze(0)
    a = ((7 * i + 13 * j) % 31 - 15).double() / 16
    i = torch.arange(n).unsqueeze(1)
    b = ((11 * i + 5 * j) % 29 - 14).double() / 16
    assert torch.equal(a.bfloat16().double(), a) and torch.equal(b.bfloat16().double(), b)
    return a.bfloat16(), b.bfloat16()


@functools.lru_cache(maxsize=None)
def exact_case(m: int, n: int, k: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(a, b, want)`` of the exact generator, built once per shape; the tensors are shared and must not be
    written to."""
    a, b = exact_operands(m, n, k)
    return a, b, reference(a, b)


# ---- guard bands -----------------------------------------------------------------------------------------------

def banded(payload: torch.Tensor, fill: int, device) -> tuple[torch.Tensor, torch.Tensor]:
    """``payload`` (bf16, 2-D) inside a larger allocation on ``device``: ``(whole, view)``.

    ``whole`` is the allocation as int16; every element outside the operand holds the 16-bit pattern ``fill``.
    ``view`` is the operand, starting ``BAND + 16`` bytes into the allocation, so that it is 16-B aligned and no
    more; at least ``BAND`` bytes of band lie on either side."""
    assert payload.dtype == torch.bfloat16 and payload.dim() == 2
    n, lead = payload.numel(), (BAND + 16) // 2
    whole = torch.full((lead + n + BAND // 2,), fill - 0x10000 if fill & 0x8000 else fill, dtype=torch.int16,
                       device=device)
    assert whole.data_ptr() % 32 == 0
    view = whole[lead:lead + n].view(torch.bfloat16).view(payload.shape)
    view.copy_(payload)
    assert view.data_ptr() % 32 == 16 and view.data_ptr() == whole.data_ptr() + BAND + 16
    return whole, view


def bands_of(whole: torch.Tensor, numel: int) -> tuple[torch.Tensor, torch.Tensor]:
    """The leading and the trailing band of a :func:`banded` allocation whose operand has ``numel`` elements."""
    lead = (BAND + 16) // 2
    return whole[:lead], whole[lead + numel:]


# ---- epilogue rounding: any fp32 value pushed through the accumulator ------------------------------------------

ROUND_M = ROUND_N = 256
ROUND_K = 128
PIECE_K = (0, 32, 64)  # where the three pieces of a row sit: no two in one 16-wide k block
LOW16 = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF, 0x0080, 0x4000, 0xC000)
LOW16_NO_L = (0x0000, 0x0100, 0x4000, 0x7F00, 0x8000, 0x8100, 0xC000, 0xFF00)  # low byte clear: the piece l is 0
SPECIAL_ROWS = ("+inf", "-inf", "inf-inf", "nan", "acc-overflow")
E_MIN, E_MAX = -103, 127  # 2^-23 * 2^-103 = 2^-126: the smallest piece times the smallest scale is still normal


def split3(xbits: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The three truncation pieces of the fp32 values with bit patterns ``xbits``: ``h`` is x with the low 16 bits
    cleared, ``m`` and ``l`` come the same way from the remainder.  Each piece has at most 8 significant bits (a
    bf16), the pieces have x's sign and disjoint bit-fields, and ``h + m + l == x`` exactly."""
    x = xbits.astype(np.uint32).view(np.float32)
    h = (xbits.astype(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    r = x - h
    m = (r.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    return h, m, r - m


def _lcg(seed: int):
    x = seed & 0xFFFFFFFF
    while True:
        x = (x * 1664525 + 1013904223) & 0xFFFFFFFF
        yield x >> 8  # the high 24 bits: the low ones of an LCG have short periods


class RoundingCase:
    """The operands of the rounding test and what is known about them.

    Row ``i`` of A holds the fp32 value ``x_i`` in [1, 2) as its pieces ``h, m, l`` at k = 0, 32, 64 and +0
    elsewhere; row ``j`` of B holds ``s_j = +-2^e_j`` in every k position.  So ``C[i][j] = bf16(x_i * s_j)``, and
    every partial sum of the accumulation, in any order, is a sum of pieces with disjoint bit-fields scaled by a
    power of two: an fp32 value.  Five special rows of A and one all-zero row of B carry the infinities, the NaNs
    and the overflow inside the accumulation; each affects only its own row or column of C.

    Attributes: ``a``, ``b`` (bf16), ``want`` (bf16, the reference), ``xbits`` (uint32 per row, 0 for a special
    row), ``finite_rows``, ``rows16`` (finite rows with ``l == 0``), ``special`` (name -> row), ``e`` and ``sign``
    per column, ``finite_cols``, ``zero_col``, ``one_col`` (``s = +1``), ``minus_one_col``."""

    def __init__(self):
        rng = _lcg(20260)
        mant = [(hi << 16) | lo for hi in (0x2A, 0x2B) for lo in LOW16]  # every pattern under an even and an odd bit 16
        mant += [(0x7F << 16) | lo for lo in LOW16]  # bits 16..22 all ones: rounding up carries into the exponent
        mant += [lo for lo in LOW16]  # and all zeros
        mant += [(hi << 16) | lo for hi in (0x00, 0x01, 0x2A, 0x2B, 0x7E, 0x7F) for lo in LOW16_NO_L]
        mant += [next(rng) & 0x7FFF00 for _ in range(24)]  # random, 16 significant bits
        n_finite = ROUND_M - len(SPECIAL_ROWS)
        mant += [next(rng) & 0x7FFFFF for _ in range(n_finite - len(mant))]  # random, 24 significant bits
        assert len(mant) == n_finite
        # spread the classes over the wave tiles and fragments: entry t of the list goes to row 37 t mod 256
        place = [(37 * t) % ROUND_M for t in range(ROUND_M)]
        assert sorted(place) == list(range(ROUND_M))
        self.xbits = np.zeros(ROUND_M, dtype=np.uint32)
        for t, mt in enumerate(mant):
            self.xbits[place[t]] = 0x3F800000 | mt
        self.special = {name: place[n_finite + t] for t, name in enumerate(SPECIAL_ROWS)}
        self.finite_rows = np.flatnonzero(self.xbits)
        self.rows16 = np.flatnonzero((self.xbits != 0) & ((self.xbits & 0xFF) == 0))

        a = np.zeros((ROUND_M, ROUND_K), dtype=np.float32)
        h, m, l = split3(self.xbits[self.finite_rows])
        for k, piece in zip(PIECE_K, (h, m, l)):
            a[self.finite_rows, k] = piece
        big = np.array([0x7F7F0000], dtype=np.uint32).view(np.float32)[0]  # the largest finite bf16
        sp = self.special
        a[sp["+inf"], 0] = np.inf
        a[sp["-inf"], 0] = -np.inf
        a[sp["inf-inf"], 0], a[sp["inf-inf"], 32] = np.inf, -np.inf
        a[sp["nan"], 0] = np.nan
        a[sp["acc-overflow"], 0] = a[sp["acc-overflow"], 32] = big
        abits = a.view(np.uint32)
        assert not (abits & 0xFFFF).any()  # every entry is a bf16: take its high half as it is (the NaN is 0x7FC0)
        self.a = torch.from_numpy((abits >> 16).astype(np.uint16).view(np.int16)).view(torch.bfloat16)
        assert int(bits(self.a)[sp["nan"], 0]) == BF16_QNAN

        # columns: the ends of the exponent range several times over and with both signs, the rest spread evenly
        es = [E_MAX] * 6 + [E_MAX - 1] * 2 + [E_MIN] * 2 + [0] * 2
        rest = ROUND_N - 1 - len(es)
        es += [E_MIN + round(t * (E_MAX - E_MIN) / (rest - 1)) for t in range(rest)]
        place = [(91 * t) % ROUND_N for t in range(ROUND_N)]
        assert sorted(place) == list(range(ROUND_N))
        self.e = np.zeros(ROUND_N, dtype=np.int64)
        self.sign = np.ones(ROUND_N, dtype=np.float64)
        for t, e in enumerate(es):
            self.e[place[t]] = e
            self.sign[place[t]] = -1.0 if t & 1 else 1.0
        self.zero_col = place[ROUND_N - 1]
        self.finite_cols = np.array(sorted(place[:ROUND_N - 1]))
        self.one_col, self.minus_one_col = place[10], place[11]
        s = self.sign * np.exp2(self.e.astype(np.float64))
        s[self.zero_col] = 0.0
        self.s = s  # fp64; every entry a bf16
        b = torch.from_numpy(np.repeat(s[:, None], ROUND_K, axis=1))
        self.b = b.bfloat16()
        assert torch.equal(self.b.double(), b)
        self.want = reference(self.a, self.b)

    def pieces(self) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``h, m, l`` of the finite rows, as fp32."""
        return split3(self.xbits[self.finite_rows])

    def x(self) -> np.ndarray:
        """``x_i`` of the finite rows, as fp32."""
        return self.xbits[self.finite_rows].view(np.float32)


@functools.lru_cache(maxsize=None)
def rounding_case() -> RoundingCase:
    """The one rounding case, built once; its tensors are shared and must not be written to."""
    return RoundingCase()


def f2bf_twin(u: np.ndarray) -> np.ndarray:
    """NumPy transcription of the kernel's ``f2bf`` on fp32 bit patterns: round to nearest even, NaN kept a NaN."""
    u = u.astype(np.uint32)
    special = (u & np.uint32(0x7F800000)) == np.uint32(0x7F800000)
    nanbit = np.where((u & np.uint32(0xFFFF)) != 0, np.uint32(0x40), np.uint32(0))
    rounded = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)
    return np.where(special, (u >> np.uint32(16)) | nanbit, rounded).astype(np.uint16)


ORDERS = tuple(itertools.permutations(range(3)))
