"""Host side of the HBM pre-flight memory test (native/kernels/memtest.hip).

:func:`memtest_words` is the NumPy twin of the kernels' pattern generator (uint64 wrap-around arithmetic), and
:data:`LEVELS` is the pass list of each level -- the same sequence ``gsx_memtest_run`` and ``gsx-memtest`` execute --
from which the bytes a run moves follow.  No GPU and no native library is needed to import this module.
"""
from __future__ import annotations

import numpy as np

ADDR, SOLID, WALK, RANDOM = 0, 1, 2, 3
PATTERNS = {"ADDR": ADDR, "SOLID": SOLID, "WALK": WALK, "RANDOM": RANDOM}
QUICK, FULL = 0, 1
LEVEL_IDS = {"quick": QUICK, "full": FULL}
MAX_ERRS = 32

_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)
_GOLDEN = 0x9E3779B97F4A7C15
_MASK64 = (1 << 64) - 1


def _mix64(z: np.ndarray) -> np.ndarray:
    """splitmix64's output function (two multiply-xorshift rounds), element-wise on uint64."""
    z = (z ^ (z >> np.uint64(30))) * _M1
    z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


def memtest_words(pattern: int, seed: int, invert: int, origin: int, nbytes: int) -> np.ndarray:
    """The expected content of ``nbytes`` bytes whose first byte lies ``origin`` bytes into the tested range, as
    ``nbytes // 4`` uint32 dwords.  Word ``W = origin // 16 + k`` holds dwords ``4k .. 4k + 3``."""
    if origin % 16 or nbytes % 16 or origin < 0 or nbytes < 0:
        raise ValueError("origin and nbytes must be non-negative multiples of 16")
    seed &= 0xFFFFFFFF
    n = nbytes // 16
    with np.errstate(over="ignore"):
        w = np.uint64(origin // 16) + np.arange(n, dtype=np.uint64)
        out = np.empty((n, 4), dtype=np.uint32)
        if pattern == ADDR:
            lo, hi = (w & np.uint64(0xFFFFFFFF)).astype(np.uint32), (w >> np.uint64(32)).astype(np.uint32)
            out[:, 0], out[:, 1], out[:, 2], out[:, 3] = lo, hi, ~lo, ~hi
        elif pattern == SOLID:
            out[:] = np.uint32(seed)
        elif pattern == WALK:
            for j in range(4):
                sh = (np.uint64(4) * w + np.uint64(j + seed)) & np.uint64(31)
                out[:, j] = (np.uint64(1) << sh).astype(np.uint32)
        elif pattern == RANDOM:
            key = np.uint64(((seed + 1) * _GOLDEN) & _MASK64)  # never 0: the mixer maps 0 to 0
            for half in range(2):
                z = _mix64(np.uint64(2) * w + np.uint64(half) + key)
                out[:, 2 * half] = (z & np.uint64(0xFFFFFFFF)).astype(np.uint32)
                out[:, 2 * half + 1] = (z >> np.uint64(32)).astype(np.uint32)
        else:
            raise ValueError(f"unknown pattern {pattern}")
    if invert:
        out = ~out
    return out.reshape(-1)


def _triple(pattern: int, seed: int) -> list[tuple[str, int, int, int, int]]:
    """write, check + rewrite (leaves the complement), check the complement: (op, pattern, seed, invert, rewrite)."""
    return [("write", pattern, seed, 0, 0), ("check", pattern, seed, 0, 1), ("check", pattern, seed, 1, 0)]


_QUICK = _triple(ADDR, 0) + _triple(RANDOM, 0)
LEVELS: dict[str, list[tuple[str, int, int, int, int]]] = {
    "quick": _QUICK,
    "full": (_QUICK + [p for s in (0, 0xFFFFFFFF, 0x55555555, 0xAAAAAAAA) for p in _triple(SOLID, s)]
             + [p for s in range(32) for p in _triple(WALK, s)]),
}


def level_passes(level: str) -> int:
    return len(LEVELS[level])


def bytes_moved(level: str, nbytes: int, passes: int | None = None) -> int:
    """HBM traffic of the first ``passes`` passes (default: all) of ``level`` over ``nbytes``: a write or a check
    moves every byte once, a check that rewrites moves it twice."""
    seq = LEVELS[level] if passes is None else LEVELS[level][:passes]
    return sum(nbytes * (2 if rewrite else 1) for _op, _p, _s, _inv, rewrite in seq)
