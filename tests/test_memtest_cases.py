"""CPU checks of tests/memtest_cases.py, the geometry that the GPU tests of the memory test's report
(tests/test_gpu_memtest_report.py) place their errors by: a simulation of the kernel's two loops visits every word
exactly once and never one past the range, ``owner_of`` inverts ``word_of``, the sizes have the trip structure the
tests count on, and ``flip_plan`` predicts what a brute-force comparison of a patched twin finds, in report order."""
import numpy as np
import pytest

from gpushare_scheduler_extender_amd.ops import memtest as mt
from tests import memtest_cases as mc
from tests.test_gpu_memtest import CAPPED, SIZES  # the existing GPU tests' sizes; importing them needs no GPU

CUS = (1, 64, 256)


def _sizes(cus):
    return [mc.CAPPED2(cus), *SIZES, CAPPED, (16 << 20) + 48]


def _sweep(geo):
    """The kernel's two loops, all waves at once: ``(visits of every word, sweep_step calls of every wave)``.  Every
    index is asserted to lie inside the range before it counts."""
    visits = np.zeros(geo.n16, dtype=np.int64)
    base = np.arange(geo.waves, dtype=np.int64)[:, None] * mc.LANES
    i = base + np.arange(mc.LANES, dtype=np.int64)[None, :]
    last = i[:, -1].copy()
    unrolled = np.zeros(geo.waves, dtype=np.int64)
    while True:
        go = last + 3 * geo.step < geo.n16
        if not go.any():
            break
        for k in range(4):
            w = (i[go] + k * geo.step).reshape(-1)
            assert w.max() < geo.n16  # every lane of a wave in the unrolled loop is live
            np.add.at(visits, w, 1)
        i[go] += 4 * geo.step
        last[go] += 4 * geo.step
        unrolled[go] += 1
    tail = np.zeros(geo.waves, dtype=np.int64)
    while True:
        live = i < geo.n16
        go = live.any(axis=1)
        if not go.any():
            break
        np.add.at(visits, i[live], 1)
        i[go] += geo.step
        tail[go] += 1
    return visits, unrolled, tail


@pytest.mark.parametrize("cus", CUS)
def test_every_word_has_one_owner_and_owner_of_inverts_word_of(cus):
    for nbytes in _sizes(cus):
        geo = mc.geometry(nbytes, cus)
        n16 = nbytes // 16
        assert geo.n16 == n16 and geo.step == 256 * geo.grid and geo.waves == 4 * geo.grid
        assert geo.grid == min(max((n16 + 1023) // 1024, 1), 8 * cus)
        visits, unrolled, tail = _sweep(geo)
        assert (visits == 1).all(), (cus, nbytes)
        # the per-wave trip counts are the simulation's, for the first, the last and a few waves in between
        for w in sorted({0, 1, geo.waves // 2, geo.waves - 2, geo.waves - 1} & set(range(geo.waves))):
            assert geo.wave_trips(w // 4, w % 4) == (unrolled[w], tail[w]), (cus, nbytes, w)
        assert (geo.unrolled, geo.tail) == (unrolled[0], tail[0])
        assert unrolled[0] == unrolled.max() and (4 * unrolled + tail)[0] == (4 * unrolled + tail).max()
        words = np.arange(n16, dtype=np.int64)
        block, wave, lane, trip = mc.owner_of(words, geo)
        assert (mc.word_of(block, wave, lane, trip, geo) == words).all()
        assert (0 <= block).all() and (block < geo.grid).all() and (wave < 4).all() and (lane < 64).all()
        # an owner is a lane that is live at that trip, and no two words share one
        assert (trip < (4 * unrolled + tail)[4 * block + wave]).all()
        assert len(np.unique(((block * 4 + wave) * 64 + lane) * (trip.max() + 1) + trip)) == n16
        # and the other way round, from places to words and back
        rng = np.random.default_rng(cus)
        b, w, ln = rng.integers(0, geo.grid, 1000), rng.integers(0, 4, 1000), rng.integers(0, 64, 1000)
        t = rng.integers(0, max(1, n16 // geo.step), 1000)
        for got, want in zip(mc.owner_of(mc.word_of(b, w, ln, t, geo), geo), (b, w, ln, t)):
            assert (got == want).all()
    assert mc.owner_of(mc.word_of(3, 2, 63, 9, geo), geo) == (3, 2, 63, 9)  # plain integers too


def test_trip_structure_of_the_capped_sizes():
    assert mc.CAPPED2(256) == (72 << 20) + 48
    for cus in CUS:
        geo = mc.geometry(mc.CAPPED2(cus), cus)
        assert geo.grid == 8 * cus and geo.n16 == 9 * geo.step + 3
        assert (geo.unrolled, geo.tail) == (2, 2) and geo.unrolled >= 2
        _visits, unrolled, tail = _sweep(geo)
        assert (unrolled == 2).all() and tail[0] == 2 and (tail[1:] == 1).all()  # trip 9: block 0's wave 0 alone
        assert [mc.word_of(0, 0, ln, 9, geo) < geo.n16 for ln in range(5)] == [True, True, True, False, False]
        assert mc.word_of(geo.grid - 1, 3, 63, 8, geo) == geo.n16 - 4  # trip 8: every lane of every wave is live
        assert geo.phase_of(0, 0, 0) == ("unrolled", 0) and geo.phase_of(5 % geo.grid, 3, 3) == ("unrolled", 0)
        assert geo.phase_of(geo.grid - 1, 3, 5) == ("unrolled", 1) and geo.phase_of(geo.grid - 1, 3, 8) == ("tail", 0)
        assert geo.phase_of(0, 0, 9) == ("tail", 1) and geo.step_index(0, 0, 9) == 3
        with pytest.raises(ValueError):
            geo.phase_of(0, 1, 9)
    # the existing CAPPED: the grid is capped, but the unrolled loop runs exactly once in every wave at 256 CUs
    geo = mc.geometry(CAPPED, 256)
    _visits, unrolled, tail = _sweep(geo)
    assert geo.grid == 2048 and geo.n16 == 5 * geo.step + 3 and geo.unrolled == 1
    assert (unrolled == 1).all() and tail[0] == 2 and (tail[1:] == 1).all()
    # below the cap some waves never enter the unrolled loop: the level test's 16 MiB + 48 at 256 CUs
    geo = mc.geometry((16 << 20) + 48, 256)
    _visits, unrolled, tail = _sweep(geo)
    assert geo.grid == 1025 and set(unrolled.tolist()) == {0, 1} and {3, 4} <= set(tail[unrolled == 0].tolist())


def test_expected_dword_is_the_twin():
    for pattern in sorted(mt.PATTERNS.values()):
        for invert in (0, 1):
            origin = 2**36 - (1 << 12)  # W crosses 2**32 inside
            want = mt.memtest_words(pattern, 77, invert, origin, 1 << 13)
            for off in (0, 4, 12, 16, (1 << 12) - 4, 1 << 12, (1 << 13) - 4):
                assert mc.expected_dword(pattern, 77, invert, origin, off) == int(want[off // 4])
    with pytest.raises(ValueError):
        mc.expected_dword(mt.ADDR, 0, 0, 0, 6)


def _brute_force(geo, want, got, origin):
    """What the kernel and the host's merge do, one dword at a time: waves in index order, a wave's steps in turn,
    within a step lanes, then the lane's words, then dwords."""
    out = []
    for wv in range(geo.waves):
        u, t = geo.wave_trips(wv // 4, wv % 4)
        steps = [range(4 * k, 4 * k + 4) for k in range(u)] + [range(4 * u + k, 4 * u + k + 1) for k in range(t)]
        for trips in steps:
            for lane in range(64):
                for trip in trips:
                    w = wv * 64 + lane + trip * geo.step
                    if w < geo.n16:
                        out += [(origin + 16 * w + 4 * d, int(want[4 * w + d]), int(got[4 * w + d]))
                                for d in range(4) if want[4 * w + d] != got[4 * w + d]]
    return out


@pytest.mark.parametrize("pattern", sorted(mt.PATTERNS.values()))
def test_flip_plan_is_what_a_comparison_of_a_patched_twin_finds(pattern):
    cus, origin = 1, 2**36 - (1 << 17)
    geo = mc.geometry(mc.CAPPED2(cus), cus)
    last = (geo.grid - 1, 3)
    flips = [(2, 1, 5, 0, 1, 0x10), (2, 1, 5, 0, 3, 0x8000_0000), (2, 1, 40, 0, 0, 1), (2, 1, 5, 2, 2, 0x300),
             (2, 1, 17, 2, 0, 0x4000), *[(2, 1, 9, 5, d, 0xFFFFFFFF) for d in range(4)], (2, 1, 63, 8, 2, 2),
             (*last, 63, 8, 3, 0x20), (*last, 0, 7, 0, 0x40), (0, 0, 2, 9, 1, 0x80), (0, 0, 0, 0, 0, 0x100)]
    for invert in (0, 1):
        plan = mc.flip_plan(flips, geo, pattern, 9, invert, origin)
        want = mt.memtest_words(pattern, 9, invert, origin, geo.nbytes)
        got = want.copy()
        for off, value in plan.patches:
            got[off // 4] = value
        bad = np.flatnonzero(want != got)
        assert plan.bad_dwords == len(bad) == len(flips) and len(plan.records) == len(flips)
        assert plan.records == {(origin + 4 * int(k), int(want[k]), int(got[k])) for k in bad}
        assert plan.flipped_or == int(np.bitwise_or.reduce(want[bad] ^ got[bad]))
        assert list(plan.ordered) == _brute_force(geo, want, got, origin)
    # the first wave's records come first, the last wave's last, and trip 0 before trip 9 in the ragged wave
    offs = [off - origin for off, _e, _a in plan.ordered]
    assert offs[:2] == [0, 16 * mc.word_of(0, 0, 2, 9, geo) + 4]
    assert offs[-2:] == [16 * mc.word_of(*last, 0, 7, geo), 16 * mc.word_of(*last, 63, 8, geo) + 12]
    for wrong in ([(geo.grid, 0, 0, 0, 0, 1)], [(0, 0, 3, 9, 0, 1)], [(0, 0, 0, 0, 0, 0)],
                  [(0, 0, 0, 0, 0, 1), (0, 0, 0, 0, 0, 2)]):
        with pytest.raises(ValueError):
            mc.flip_plan(wrong, geo, pattern)


@pytest.mark.parametrize("cus", CUS)
def test_full_level_flips_are_distinct_and_spread(cus):
    geo = mc.geometry((16 << 20) + 48, cus)
    flips = mc.full_level_flips(geo, 38)
    assert len(flips) == 38
    words = [mc.word_of(b, w, ln, t, geo) for b, w, ln, t, _d, _m in flips]
    assert len(set(words)) == 38 and all(0 <= w < geo.n16 for w in words)
    assert {0, geo.n16 - 1} <= set(words)
    assert all(0 <= d < 4 and 0 < m <= 0xFFFFFFFF for *_, d, m in flips)
    phases = {geo.phase_of(b, w, t)[0] for b, w, _ln, t, _d, _m in flips}
    assert phases == {"unrolled", "tail"}
    assert {(3, 63), (0, 0)} <= {(w, ln) for _b, w, ln, _t, _d, _m in flips}  # both sides of a block's end
    assert len({d for *_, d, _m in flips}) == 4
