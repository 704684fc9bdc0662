"""Where the HBM memory test's words go, for its tests (tests/test_gpu_memtest_report.py; checked without a GPU by
tests/test_memtest_cases.py).

Plain Python and NumPy, no GPU and no native library: the launch geometry of ``native/kernels/memtest.hip`` written
out a second time, so that a test can put an error into a chosen wave at a chosen step of its sweep and say which
records an honest report then holds, and in which order.  ``word_of`` and ``owner_of`` take integers or NumPy arrays.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from gpushare_scheduler_extender_amd.ops import memtest as mt

BLOCK = 256  # threads of a workgroup: four waves of 64 lanes, a lane's word is 16 bytes
LANES = 64
WORDS_PER_BLOCK = 1024  # below the cap the grid gives every lane four words
BLOCKS_PER_CU = 8
UNROLL = 4


@dataclass(frozen=True)
class Geometry:
    """One launch over ``n16`` words on ``cus`` CUs.  ``unrolled`` and ``tail`` are the trip structure of block 0's
    wave 0, which makes the most trips of the grid: its iterations of the unrolled loop and its steps of the tail
    loop.  ``wave_trips`` gives any wave's."""
    nbytes: int
    cus: int
    n16: int
    grid: int
    step: int
    unrolled: int
    tail: int

    @property
    def waves(self) -> int:
        return 4 * self.grid

    def wave_trips(self, block: int, wave: int) -> tuple[int, int]:
        """``(iterations of the unrolled loop, steps of the tail loop)`` of wave ``wave`` of block ``block``."""
        base = block * BLOCK + wave * LANES  # lane 0's first word
        last = base + LANES - 1
        u = 0
        while last + (UNROLL - 1) * self.step < self.n16:  # the condition of memtest_kernel's first loop
            last += UNROLL * self.step
            u += 1
        i, t = base + UNROLL * u * self.step, 0
        while i < self.n16:  # lane 0 is the last of a wave to run out: the ballot of the second loop
            i += self.step
            t += 1
        return u, t

    def phase_of(self, block: int, wave: int, trip: int) -> tuple[str, int]:
        """``("unrolled", t)`` when the wave handles its lanes' word ``trip`` in iteration ``t`` of the unrolled loop,
        ``("tail", k)`` when in step ``k`` of the tail loop."""
        u, t = self.wave_trips(block, wave)
        if trip < UNROLL * u:
            return "unrolled", trip // UNROLL
        if trip < UNROLL * u + t:
            return "tail", trip - UNROLL * u
        raise ValueError(f"wave {wave} of block {block} makes {UNROLL * u + t} trips, not {trip + 1}")

    def step_index(self, block: int, wave: int, trip: int) -> int:
        """Which call of ``sweep_step`` of that wave, counted from 0, handles ``trip``."""
        phase, k = self.phase_of(block, wave, trip)
        return k if phase == "unrolled" else self.wave_trips(block, wave)[0] + k


def geometry(nbytes: int, cus: int) -> Geometry:
    """The launch ``gsx_memtest_write`` / ``gsx_memtest_check`` make for ``nbytes`` on a device of ``cus`` CUs.

    Mirrors ``grid_for`` (``grid = clamp(ceil(n16 / 1024), 1, 8 * cus)``) and the two loops of ``memtest_kernel`` in
    native/kernels/memtest.hip: with ``step = 256 * grid``, a wave stays in the unrolled loop, four words per lane
    and iteration, while ``last + 3 * step < n16`` for its last lane's word ``last``, and then in the tail loop, one
    word per lane and step, while any of its lanes has a word below ``n16``."""
    if nbytes <= 0 or nbytes % 16 or cus < 1:
        raise ValueError("nbytes must be a positive multiple of 16 and cus positive")
    n16 = nbytes // 16
    grid = min(max(-(-n16 // WORDS_PER_BLOCK), 1), BLOCKS_PER_CU * cus)
    step = BLOCK * grid
    g = Geometry(nbytes, cus, n16, grid, step, 0, 0)
    u, t = g.wave_trips(0, 0)
    return Geometry(nbytes, cus, n16, grid, step, u, t)


def CAPPED2(cus: int) -> int:
    """Bytes of a range of ``9 * step + 3`` words on the capped grid: every wave makes two iterations of the unrolled
    loop (trips 0-7) and one tail step with every lane live (trip 8); block 0's wave 0 makes a second tail step
    (trip 9) in which only its lanes 0, 1 and 2 are live.  72 MiB + 48 at 256 CUs."""
    step_capped = BLOCKS_PER_CU * cus * BLOCK
    return 16 * (9 * step_capped + 3)


def word_of(block, wave, lane, trip, geo: Geometry):
    """The index of the ``trip``-th word of lane ``lane`` of wave ``wave`` of block ``block``.  Trips ``4t .. 4t + 3``
    are iteration ``t`` of the unrolled loop; the trips after the wave's unrolled range are its tail steps."""
    return block * BLOCK + wave * LANES + lane + trip * geo.step


def owner_of(word, geo: Geometry):
    """``(block, wave, lane, trip)`` of a word index: the inverse of :func:`word_of`."""
    trip, r = word // geo.step, word % geo.step
    return r // BLOCK, (r % BLOCK) // LANES, r % LANES, trip


def expected_dword(pattern: int, seed: int, invert: int, origin: int, byte_off: int) -> int:
    """What the dword at byte ``byte_off`` of a range that starts at ``origin`` holds: the twin of its one word."""
    if byte_off % 4 or byte_off < 0:
        raise ValueError("a dword offset is a non-negative multiple of 4")
    word = mt.memtest_words(pattern, seed, invert, origin + byte_off // 16 * 16, 16)
    return int(word[byte_off % 16 // 4])


@dataclass(frozen=True)
class Plan:
    """``patches``: ``(byte offset in the range, dword to store there)``.  ``ordered``: the records
    ``(origin + offset, expected, actual)`` in the order in which one check reports them while slots last -- the
    host merges waves in index order, a wave's steps fill its slots one after the other, and within a step the bad
    dwords go in lane order, then by word, then by dword.  ``records`` is the same as a set."""
    patches: tuple[tuple[int, int], ...]
    ordered: tuple[tuple[int, int, int], ...]
    flipped_or: int

    @property
    def records(self) -> set[tuple[int, int, int]]:
        return set(self.ordered)

    @property
    def bad_dwords(self) -> int:
        return len(self.ordered)


def flip_plan(flips, geo: Geometry, pattern: int, seed: int = 0, invert: int = 0, origin: int = 0) -> Plan:
    """``flips`` is a list of ``(block, wave, lane, trip, dword, xor_mask)``: XOR ``xor_mask`` into dword ``dword``
    of that lane's ``trip``-th word, in a range that holds ``(pattern, seed, invert)`` at ``origin``."""
    rows, seen = [], set()
    for block, wave, lane, trip, dword, mask in flips:
        if not (0 <= block < geo.grid and 0 <= wave < 4 and 0 <= lane < LANES and 0 <= dword < 4):
            raise ValueError(f"no such place: {(block, wave, lane, trip, dword)}")
        if not 0 < mask <= 0xFFFFFFFF:
            raise ValueError("the mask must change the dword")
        word = word_of(block, wave, lane, trip, geo)
        if not 0 <= word < geo.n16:
            raise ValueError(f"word {word} of {(block, wave, lane, trip)} lies outside the range")
        off = 16 * word + 4 * dword
        if off in seen:
            raise ValueError(f"two flips of the dword at {off}")
        seen.add(off)
        e = expected_dword(pattern, seed, invert, origin, off)
        key = (4 * block + wave, geo.step_index(block, wave, trip), lane, trip, dword)
        rows.append((key, off, e, e ^ mask, mask))
    rows.sort()
    flipped = 0
    for *_, mask in rows:
        flipped |= mask
    return Plan(tuple((off, a) for _k, off, _e, a, _m in rows),
                tuple((origin + off, e, a) for _k, off, e, a, _m in rows), flipped)


def full_level_flips(geo: Geometry, n: int) -> list[tuple[int, int, int, int, int, int]]:
    """``n`` flips ``(block, wave, lane, trip, dword, xor_mask)`` at pairwise different dwords, one per triple of a
    level: the first and the last word of the range, the two lanes on either side of a block's end, words of the
    unrolled loop and words of the tail loop, the rest spread evenly over the range."""
    last = geo.n16 - 1
    words = [0, last]
    blk = geo.grid // 2
    words += [w for w in (word_of(blk, 3, LANES - 1, 1, geo), word_of(min(blk + 1, geo.grid - 1), 0, 0, 1, geo))
              if w <= last]
    _u, t = geo.wave_trips(geo.grid - 1, 3)  # the last wave runs out of the unrolled loop first
    u0, t0 = geo.wave_trips(0, 0)
    if t:
        words.append(word_of(geo.grid - 1, 3, 17, UNROLL * _u, geo))  # a tail step of the last wave
    if t0:
        words.append(word_of(0, 0, 0, UNROLL * u0 + t0 - 1, geo))  # the last tail step of the first wave
    if u0:
        words += [word_of(0, 1, 33, k, geo) for k in range(min(UNROLL * u0, 6))]  # the first wave's unrolled trips
    words = [w for w in dict.fromkeys(words) if 0 <= w <= last]
    k = 0
    while len(words) < n:  # an odd stride: no two of these share a lane and a trip for long
        w = (k * (geo.n16 // max(n, 1) + 37) + 11 * k + 5) % geo.n16
        if w not in words:
            words.append(w)
        k += 1
    out = []
    for j, w in enumerate(words[:n]):
        block, wave, lane, trip = owner_of(w, geo)
        out.append((int(block), int(wave), int(lane), int(trip), j % 4, 1 << (7 * j % 32)))
    return out
