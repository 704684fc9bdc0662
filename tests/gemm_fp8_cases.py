"""Operand builders and the reference for the fp8 GEMM tests (native/kernels/gemm_fp8.hip).

Plain Python on torch and NumPy, no GPU: ``tests/test_gemm_fp8_cases.py`` checks on the CPU that the operands built
here have the properties the GPU tests rely on, ``tests/test_gpu_gemm_fp8.py`` feeds them to the kernels.  The
comparison is ``tests/gemm_cases.py``'s: the raw 16 bits of every element, a quiet NaN of any payload where the
reference is NaN.

Operands are OCP e4m3 (``torch.float8_e4m3fn``).  Every case is built so that the fp64 product of its operands is an
fp32 value and every partial sum of the fp32 accumulation, in any order, is exact.  The reference is that product
rounded to fp32, then the two fp32 multiplies of the epilogue, ``(acc * sa[row]) * sb[col]``, then one rounding to
bf16: what the kernel has to produce bit for bit.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests import gemm_cases as gc

FP8 = torch.float8_e4m3fn
FP8_NAN = 0x7F  # what the guard bands of A and B hold; the other NaN code is 0xFF
NAN_CODES = (0x7F, 0xFF)
SCALE_NONE, SCALE_TENSOR, SCALE_ROW = 0, 1, 2  # gsx_kernels.h


# ---- reference and comparison ----------------------------------------------------------------------------------

def accumulator(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """``A * B^T`` as the fp64 product rounded once to fp32, on the CPU."""
    return (a.cpu().double() @ b.cpu().double().t()).float()


def scaled(acc: torch.Tensor, sa=None, sb=None) -> torch.Tensor:
    """The epilogue on an fp32 accumulator: ``bf16((acc * sa[row]) * sb[col])``, two fp32 multiplies in that order.
    ``sa`` and ``sb`` are fp32 tensors of one element (per tensor) or of ``M`` and ``N`` (per row); None: no
    multiply."""
    assert acc.dtype == torch.float32 and (sa is None) == (sb is None)
    if sa is not None:
        assert sa.dtype == torch.float32 and sb.dtype == torch.float32
        acc = (acc * sa.reshape(-1, 1)) * sb.reshape(1, -1)
        assert acc.dtype == torch.float32
    return acc.bfloat16()


def reference(a: torch.Tensor, b: torch.Tensor, sa=None, sb=None) -> torch.Tensor:
    return scaled(accumulator(a, b), sa, sb)


def assert_bits_equal(got: torch.Tensor, want: torch.Tensor, what: str = "", zeros_by_value: bool = False) -> None:
    """``gemm_cases.assert_bits_equal``; with ``zeros_by_value`` a zero of either sign is accepted wherever ``want``
    is a zero."""
    got = got.cpu()
    if zeros_by_value:
        both_zero = ((gc.bits(got) & 0x7FFF) == 0) & ((gc.bits(want) & 0x7FFF) == 0)
        got = torch.where(both_zero, want, got)
    gc.assert_bits_equal(got, want, what)


def codes(t: torch.Tensor) -> torch.Tensor:
    """The raw bytes of an fp8 tensor, as int32 in 0..255."""
    assert t.dtype == FP8
    return t.contiguous().view(torch.uint8).to(torch.int32)


def from_codes(c) -> torch.Tensor:
    return torch.as_tensor(np.asarray(c, dtype=np.uint8)).view(FP8)


# ---- the exact generator ---------------------------------------------------------------------------------------

def exact_operands(m: int, n: int, k: int) -> tuple[torch.Tensor, torch.Tensor]:
    """``gemm_cases.exact_operands`` in e4m3: every input is q/16 with |q| <= 15, which e4m3 holds exactly."""
    a, b = gc.exact_operands(m, n, k)
    a8, b8 = a.to(FP8), b.to(FP8)
    assert torch.equal(a8.double(), a.double()) and torch.equal(b8.double(), b.double())
    return a8, b8


@functools.lru_cache(maxsize=None)
def exact_case(m: int, n: int, k: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(a, b, acc)`` of the exact generator, ``acc`` the fp32 accumulator; built once per shape, shared, and not to
    be written to."""
    a, b = exact_operands(m, n, k)
    return a, b, accumulator(a, b)


# ---- every e4m3 code ---------------------------------------------------------------------------------------------

SWEEP_M = SWEEP_N = SWEEP_K = 256
SWEEP_E = tuple(range(-9, 9))  # 2^-9, 2^-8 and 2^-7 are e4m3 subnormals; 2^8 is the largest power of two


def sweep_k_of_row(i: int) -> int:
    """Where row ``i`` of A holds its code: a bijection onto 0..255, so both K-tiles and all 128 positions inside a
    tile are used, each by one row per tile."""
    return (37 * i) % SWEEP_K


@functools.lru_cache(maxsize=None)
def code_sweep() -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(a, b, want)``, 256 x 256 x 256: row ``i`` of A holds e4m3 code ``i`` at k = ``sweep_k_of_row(i)`` and +0
    elsewhere; column ``j`` of B holds ``(-1)^j 2^e`` at every k, ``e = SWEEP_E[(j // 2) % 18]``.  So ``C[i][j]`` is
    the value of code ``i`` times a signed power of two: exact in bf16, NaN in the rows of the two NaN codes.  A
    kernel that read the codes as fnuz (bias 8, 0x80 = NaN), selected another format, or applied a hardware scale
    other than 1 gets almost every element wrong."""
    a = np.zeros((SWEEP_M, SWEEP_K), dtype=np.uint8)
    for i in range(SWEEP_M):
        a[i, sweep_k_of_row(i)] = i
    s = np.array([(-1.0) ** j * 2.0 ** SWEEP_E[(j // 2) % len(SWEEP_E)] for j in range(SWEEP_N)])
    b = torch.from_numpy(np.repeat(s[:, None], SWEEP_K, axis=1))
    b8 = b.to(FP8)
    assert torch.equal(b8.double(), b)
    a8 = from_codes(a)
    return a8, b8, reference(a8, b8)


# ---- k positions: A's and B's operand paths must agree ------------------------------------------------------------

SLOT_M = SLOT_N = 512
SLOT_K = 256


def slot_values(count: int, mul: int, period: int) -> torch.Tensor:
    """``count`` positive values q/16, q in 1..``period`` (at most 15), as fp64, with that period."""
    return (1 + (mul * torch.arange(count)) % period).double() / 16


@functools.lru_cache(maxsize=None)
def k_slot_case() -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(a, b, want)``, 512 x 512 x 256: ``A[i][k] = u_i`` where ``k = i mod 256`` and ``B[j][k] = v_j`` where
    ``k = j mod 256``, +0 elsewhere.  ``C[i][j] = u_i v_j`` where ``i = j (mod 256)`` and +0 otherwise: a k
    position that the two operand paths place differently moves or removes the entry of a named row and column.
    Two K-tiles, so both LDS buffers."""
    u, v = slot_values(SLOT_M, 7, 15), slot_values(SLOT_N, 5, 13)
    a = torch.zeros(SLOT_M, SLOT_K, dtype=torch.float64)
    b = torch.zeros(SLOT_N, SLOT_K, dtype=torch.float64)
    a[torch.arange(SLOT_M), torch.arange(SLOT_M) % SLOT_K] = u
    b[torch.arange(SLOT_N), torch.arange(SLOT_N) % SLOT_K] = v
    a8, b8 = a.to(FP8), b.to(FP8)
    assert torch.equal(a8.double(), a) and torch.equal(b8.double(), b)
    return a8, b8, reference(a8, b8)


# ---- scales ----------------------------------------------------------------------------------------------------

def row_scales(count: int, seed: int) -> torch.Tensor:
    """``count`` fp32 values with random 23-bit mantissa fields (24 significant bits), both signs and magnitudes in
    [2^-4, 2^4)."""
    rng = np.random.default_rng(seed)
    mant = rng.integers(0, 1 << 23, size=count, dtype=np.uint32)
    exp = rng.integers(127 - 4, 127 + 4, size=count, dtype=np.uint32)
    sign = rng.integers(0, 2, size=count, dtype=np.uint32)
    return torch.from_numpy(((sign << np.uint32(31)) | (exp << np.uint32(23)) | mant).view(np.float32).copy())


# ---- guard bands -----------------------------------------------------------------------------------------------

def banded(payload: torch.Tensor, device) -> tuple[torch.Tensor, torch.Tensor]:
    """``gemm_cases.banded`` for an fp8 operand: ``(whole, view)``, ``whole`` the allocation as uint8 with the NaN
    code 0x7F everywhere outside the operand, ``view`` the operand ``BAND + 16`` bytes in (16-B aligned and no
    more)."""
    assert payload.dtype == FP8 and payload.dim() == 2
    n, lead = payload.numel(), gc.BAND + 16
    whole = torch.full((lead + n + gc.BAND,), FP8_NAN, dtype=torch.uint8, device=device)
    assert whole.data_ptr() % 32 == 0
    view = whole[lead:lead + n].view(FP8).view(payload.shape)
    view.copy_(payload)
    assert view.data_ptr() % 32 == 16
    return whole, view
