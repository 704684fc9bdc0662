"""Problems for the decode GEMM tests (native/kernels/gemm_decode.hip): ``C[M][N] = A[M][K] * B[N][K]^T``, M <= 16.

Plain Python on torch and NumPy, no GPU.  Nothing is generated here: the operands, the references and the exactness
conditions are those of ``tests/gemm_cases.py`` (bf16), ``tests/gemm_fp8_cases.py`` and ``tests/gemm_mxfp4_cases.py``.
Their conditions do not depend on the order of the summation, so a kernel that splits K among its waves still has to
produce the reference bit for bit.  What this module adds is one form, :class:`Problem`, for the three operand
kinds, and the two ways a large case is cut down to the kernel's shape:

* ``rows(r0, m)``: rows ``r0 .. r0 + m - 1`` of A (with their scales) against all of B.  The 16-row slices of a case
  put together are the case;
* ``transposed()``: the case's B as A and its A as B, scales exchanged.  The wanted result is the transpose of the
  case's.  Its 16-row slices put what the case has in the rows of A (every operand code at every k position, say) on
  the kernel's path for B.

``tests/test_gemm_decode_cases.py`` checks both against the references on the CPU.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from tests import gemm_cases as gc
from tests import gemm_fp8_cases as gf
from tests import gemm_mxfp4_cases as mc

KINDS = ("bf16", "fp8", "mxfp4")
BK = {"bf16": 64, "fp8": 128, "mxfp4": 256}  # elements of a K-tile (128 B of a row)
MAX_M = 16

# the library's table (gsx_decode_gemm_cfg_name / _cfg_shape): name, columns of a strip, waves, K-tiles in flight
CFGS = {0: ("16/4w-f4", 16, 4, 4), 1: ("16/8w-f4", 16, 8, 4), 2: ("16/8w-f8", 16, 8, 8), 3: ("16/16w-f4", 16, 16, 4),
        4: ("32/8w-f4", 32, 8, 4), 5: ("16/8w-f4-nt", 16, 8, 4), 6: ("16/8w-f4-masked", 16, 8, 4)}
ALL = [*CFGS, None]  # None: the dispatching entry point


MAX_K = {"bf16": 65536, "fp8": 65536, "mxfp4": 32768}  # as far as the exact generators' conditions hold


def k_tile_counts(cfg, kind: str) -> list[int]:
    """The K-tile counts that matter to a configuration with W waves that keep F tiles in flight each: waves without
    a tile (1, 2, W - 1), a ragged last round (W + 1, 2 W + 1), the short path with its conditional prologue (up to
    F W + 1 and beyond: a wave with fewer than 2 F tiles), the first counts at which some and then all waves enter
    the steady loop (2 F W - W + 1, 2 F W), and long loops (128, and 4 F W + 3 where the kind's exact generator
    reaches that far).  The dispatching entry point takes every configuration's."""
    if cfg is None:
        return sorted({nk for c in CFGS for nk in k_tile_counts(c, kind)})
    _, _, w, f = CFGS[cfg]
    counts = {1, 2, w - 1, w, w + 1, 2 * w + 1, f * w - 1, f * w, f * w + 1, 2 * f * w - w + 1, 2 * f * w, 128,
              4 * f * w + 3}
    return sorted(nk for nk in counts if nk * BK[kind] <= MAX_K[kind])


@dataclasses.dataclass(frozen=True)
class Problem:
    """One product.  ``a`` and ``b`` are the operands as the kernel takes them (bf16; ``torch.float8_e4m3fn``; uint8
    with two e2m1 codes per byte), ``want`` the bf16 result.  fp8: ``mode`` is the scale mode and ``sa``, ``sb`` fp32
    tensors of one element (TENSOR) or of M and N (ROW); ``acc`` is the fp32 accumulator ``want`` comes from.  mxfp4:
    ``sa`` and ``sb`` are the e8m0 codes, ``[rows][K / 32]`` uint8.  Tensors are shared: not to be written to."""
    kind: str
    a: torch.Tensor
    b: torch.Tensor
    want: torch.Tensor
    sa: torch.Tensor | None = None
    sb: torch.Tensor | None = None
    mode: int = gf.SCALE_NONE
    acc: torch.Tensor | None = None

    @property
    def m(self) -> int:
        return self.a.shape[0]

    @property
    def n(self) -> int:
        return self.b.shape[0]

    @property
    def k(self) -> int:
        return self.a.shape[1] * (2 if self.kind == "mxfp4" else 1)

    def _per_row(self) -> bool:
        return self.kind == "mxfp4" or self.mode == gf.SCALE_ROW

    def rows(self, r0: int, m: int) -> "Problem":
        """Rows ``r0 .. r0 + m - 1`` of A, of its per-row scales and of the result."""
        assert 0 <= r0 and 1 <= m and r0 + m <= self.m
        cut = slice(r0, r0 + m)
        return dataclasses.replace(self, a=self.a[cut], want=self.want[cut],
                                   sa=self.sa[cut] if self._per_row() else self.sa,
                                   acc=None if self.acc is None else self.acc[cut])

    def transposed(self) -> "Problem":
        """B as A and A as B, the scales exchanged, the result transposed.  Where fp8 scales are applied the result
        comes from the accumulator again: ``(acc * sa) * sb`` rounds differently once sa and sb change places."""
        want = self.want.t().contiguous()
        acc = None if self.acc is None else self.acc.t().contiguous()
        if self.kind == "fp8" and self.mode != gf.SCALE_NONE:
            want = gf.scaled(acc, self.sb, self.sa)
        return dataclasses.replace(self, a=self.b, b=self.a, sa=self.sb, sb=self.sa, want=want, acc=acc)

    def reference(self) -> torch.Tensor:
        """The family's reference computed from this problem's own operands."""
        if self.kind == "bf16":
            return gc.reference(self.a, self.b)
        if self.kind == "fp8":
            none = self.mode == gf.SCALE_NONE
            return gf.reference(self.a, self.b, None if none else self.sa, None if none else self.sb)
        return mc.reference(mc.unpack(self.a.numpy()), self.sa.numpy(), mc.unpack(self.b.numpy()), self.sb.numpy())


def bf16_problem(a: torch.Tensor, b: torch.Tensor, want: torch.Tensor) -> Problem:
    """From ``gemm_cases.exact_case`` or the members of its ``rounding_case``."""
    return Problem("bf16", a, b, want)


def fp8_problem(a: torch.Tensor, b: torch.Tensor, acc: torch.Tensor, sa=None, sb=None,
                mode: int = gf.SCALE_NONE) -> Problem:
    """From ``gemm_fp8_cases``: operands and the fp32 accumulator, with the scales of ``mode`` if any."""
    assert (mode == gf.SCALE_NONE) == (sa is None) == (sb is None)
    return Problem("fp8", a, b, gf.scaled(acc, sa, sb), sa, sb, mode, acc)


def mxfp4_problem(case: mc.Case) -> Problem:
    return Problem("mxfp4", torch.from_numpy(case.aq), torch.from_numpy(case.bq), case.want,
                   torch.from_numpy(case.sa), torch.from_numpy(case.sb))


def exact_problem(kind: str, n: int, k: int) -> Problem:
    """The kind's ``exact_case`` with 16 rows of A; ``rows(0, m)`` of it is a problem of M = m."""
    if kind == "bf16":
        return bf16_problem(*gc.exact_case(MAX_M, n, k))
    if kind == "fp8":
        return fp8_problem(*gf.exact_case(MAX_M, n, k))
    return mxfp4_problem(mc.exact_case(MAX_M, n, k))


def exact_b_rows(rows: torch.Tensor, k: int) -> torch.Tensor:
    """Rows ``rows`` (int64 indices) of the B of ``gemm_cases.exact_operands`` for any N, as bf16 on the device of
    ``rows``: the formula itself, so that a B too large for the host can be made on the GPU piece by piece."""
    j = torch.arange(k, device=rows.device, dtype=torch.int64).unsqueeze(0)
    return (((11 * rows.unsqueeze(1) + 5 * j) % 29 - 14).float() / 16).bfloat16()


def error_bound(ref64: torch.Tensor, mag64: torch.Tensor, k: int) -> torch.Tensor:
    """``2^-8 |ref64| + K 2^-23 sum_k |a_k b_k|``, in fp64: how far a result accumulated in fp32 and rounded once to
    bf16 may be from the fp64 product ``ref64``.  The first term is the one rounding to bf16 (half a unit of its 8
    bits).  The second is the accumulation in any order: K additions, each off by at most 2^-24 of a partial sum that
    ``mag64 = sum_k |a_k b_k|`` bounds, and as much again for what that does to the value that is then rounded."""
    return 2.0 ** -8 * ref64.abs() + k * 2.0 ** -23 * mag64


def as_bytes(t: torch.Tensor) -> np.ndarray:
    """The storage of an operand as uint8, for the guard-band helpers."""
    return t.contiguous().view(torch.uint8).numpy()
