"""Host side of the compute pre-flight (native/kernels/cutest.hip): the NumPy twin of every unit's known answer.

A unit ends in one 64-bit signature per wave.  The matrix units multiply operands that are a function of the matrix
coordinates alone -- the twin computes a plain integer ``A @ B`` and knows nothing of lanes or registers -- and every
result is an exact integer whatever the order of summation (:func:`abs_bound`, against :func:`exact_limit`).
``VALU_INT`` and ``LDS`` are twinned step by step in uint64 wrap-around arithmetic.  No GPU and no native library is
needed to import this module.
"""
from __future__ import annotations

import numpy as np

from .memtest import _GOLDEN, _MASK64, RANDOM, _mix64, memtest_words

# name, M, N, K, R (rounds chained into one accumulator), span (operands are integers in [-span/2, span/2 - 1]),
# the unit whose operands it multiplies, integer accumulator
_TABLE = (
    ("MFMA_BF16_16", 16, 16, 32, 64, 16, 0, False),
    ("MFMA_BF16_32", 32, 32, 16, 64, 16, 1, False),
    ("MFMA_F16", 16, 16, 32, 64, 16, 2, False),
    ("MFMA_FP8", 16, 16, 32, 64, 16, 3, False),
    ("MFMA_I8", 16, 16, 64, 64, 256, 4, True),
    ("MFMA_F32", 16, 16, 4, 32, 512, 5, False),
    ("VALU_F32", 16, 16, 4, 32, 512, 5, False),  # the same product as MFMA_F32, by v_fma_f32
)
UNITS = tuple(t[0] for t in _TABLE) + ("VALU_INT", "LDS")
UNIT_IDS = {n: i for i, n in enumerate(UNITS)}
VALU_INT, LDS = UNIT_IDS["VALU_INT"], UNIT_IDS["LDS"]
MATRIX_UNITS = tuple(range(len(_TABLE)))
ROUNDS = {u: _TABLE[u][4] for u in MATRIX_UNITS}
SHAPES = {u: _TABLE[u][1:4] for u in MATRIX_UNITS}
SPANS = {u: _TABLE[u][5] for u in MATRIX_UNITS}

QUICK, FULL = 0, 1
LEVEL_IDS = {"quick": QUICK, "full": FULL}
SEEDS = {"quick": 8, "full": 256}  # launches of a level: seeds 0 .. n - 1
MAX_BAD = 16  # bad-CU entries a report lists
CU_SLOTS = 4096  # xcc << 8 | se << 5 | sh << 4 | cu
EXTRA_LAUNCHES = 8  # what gsx_cutest_run adds at the most to reach coverage

VALU_INT_STEPS = 256
LDS_BYTES = 163840
LDS_QUARTER_DWORDS = LDS_BYTES // 4 // 4

_U = np.uint64


def _key(seed: int) -> int:
    return ((int(seed) & 0xFFFFFFFF) + 1) * _GOLDEN & _MASK64  # never 0: the mixer maps 0 to 0


def _pos(n: np.ndarray) -> np.ndarray:
    """The position term of a signature: ``n`` times an odd constant, mod 2^64."""
    with np.errstate(over="ignore"):
        return n.astype(_U) * _U(_GOLDEN)


def exact_limit(unit: int) -> int:
    """Below this every partial sum is an exact integer in the unit's accumulator (f32: 2^24, i32: 2^31)."""
    return 1 << 31 if _TABLE[unit][7] else 1 << 24


def operands(unit: int, seed: int) -> tuple[np.ndarray, np.ndarray]:
    """``A[R][M][K]`` and ``B[R][K][N]`` of a matrix unit as int64: element ``A[i][k]`` (``which`` 0) or ``B[k][j]``
    (``which`` 1, its coordinate ``j`` in the place of ``i``) of round ``r`` is
    ``(mix64(key(seed) + (u << 32 | r << 24 | which << 16 | i << 8 | k)) >> 32) mod span - span / 2``."""
    _name, m, n, k, rounds, span, gen, _int = _TABLE[unit]
    key = _key(seed)

    def side(which: int, rows: int) -> np.ndarray:
        r, i, kk = np.meshgrid(np.arange(rounds, dtype=_U), np.arange(rows, dtype=_U), np.arange(k, dtype=_U),
                               indexing="ij")
        ctr = (_U(gen) << _U(32)) | (r << _U(24)) | (_U(which) << _U(16)) | (i << _U(8)) | kk
        with np.errstate(over="ignore"):
            z = _mix64(ctr + _U(key))
        return ((z >> _U(32)) & _U(span - 1)).astype(np.int64) - span // 2

    return side(0, m), side(1, n).transpose(0, 2, 1)


def product(unit: int, seed: int) -> np.ndarray:
    """``sum over r of A_r @ B_r`` in int64."""
    a, b = operands(unit, seed)
    return np.einsum("rik,rkj->ij", a, b)


def abs_bound(unit: int, seed: int) -> int:
    """``max over (i, j) of sum |a| |b|`` over the whole chain: no partial sum of any order exceeds it."""
    a, b = operands(unit, seed)
    return int(np.einsum("rik,rkj->ij", np.abs(a), np.abs(b)).max())


def result_bits(unit: int, d: np.ndarray) -> np.ndarray:
    """The raw 32 bits of every result element: an f32 for the f32-accumulating units, an i32 for ``MFMA_I8``."""
    if _TABLE[unit][7]:
        return d.astype(np.int32).view(np.uint32)
    return d.astype(np.float32).view(np.uint32)


def signature(bits: np.ndarray) -> int:
    """``sum over (i, j) of mix64(bits[i][j] ^ (i * N + j + 1) * odd) mod 2^64`` of an ``M x N`` array of uint32."""
    flat = np.ascontiguousarray(bits, dtype=np.uint32).reshape(-1)
    with np.errstate(over="ignore"):
        return int(_mix64(flat.astype(_U) ^ _pos(np.arange(1, flat.size + 1))).sum(dtype=_U))


def valu_int_lanes(seed: int) -> tuple[np.ndarray, np.ndarray]:
    """The 64 lanes' ``(x, y)`` after the integer chain: 32-bit multiply low and high, a 64-bit multiply-add, a
    rotate, xor, popcount and a compare-select per step."""
    m32 = _U(0xFFFFFFFF)
    with np.errstate(over="ignore"):
        y = _mix64(_U(_key(seed)) + (_U(VALU_INT) << _U(32)) + np.arange(64, dtype=_U))
        x = y >> _U(32)
        for _ in range(VALU_INT_STEPS):
            c = (y & m32) | _U(1)
            lo = (x * _U(0x9E3779B1)) & m32
            hi = (x * c) >> _U(32)
            y = y * _U(0xD1342543DE82EF95) + ((hi << _U(32)) | lo)
            rot = y >> _U(59)
            v = lo ^ hi
            r = ((v << rot) | (v >> (_U(32) - rot))) & m32
            p = np.unpackbits(y.view(np.uint8).reshape(64, 8), axis=1).sum(axis=1, dtype=_U)  # popcount
            x = np.where(r > (y >> _U(32)), (r + p) & m32, r ^ (p * _U(0x01010101)))
    return x, y


def _valu_int_signature(seed: int) -> int:
    x, y = valu_int_lanes(seed)
    lane = np.arange(64)
    with np.errstate(over="ignore"):
        return int((_mix64(y ^ _pos(lane + 1)) + _mix64(x ^ _pos(lane + 65))).sum(dtype=_U))


def lds_words(seed: int, which_pass: int) -> np.ndarray:
    """What a wave folds of the quarter it read in pass 0 or 1 (the complement): the memory test's RANDOM words of
    (seed, dword index in the quarter)."""
    return memtest_words(RANDOM, seed, which_pass, 0, 4 * LDS_QUARTER_DWORDS)


def _lds_signature(seed: int) -> int:
    total = 0
    for p in (0, 1):
        w = lds_words(seed, p).astype(_U)
        with np.errstate(over="ignore"):
            total += int(_mix64(w ^ _pos(np.arange(1, w.size + 1) + p * LDS_QUARTER_DWORDS)).sum(dtype=_U))
    return total & _MASK64


def expected_signature(unit: int, seed: int) -> int:
    """The signature every healthy wave reports for ``unit`` in a launch with ``seed``."""
    if unit in MATRIX_UNITS:
        return signature(result_bits(unit, product(unit, seed)))
    if unit == VALU_INT:
        return _valu_int_signature(seed)
    if unit == LDS:
        return _lds_signature(seed)
    raise ValueError(f"unknown unit {unit}")
