"""What the HBM memory test reports, on a real MI355X (native/kernels/memtest.hip, gsx-memtest): errors that one wave
meets at several steps of its sweep, in the unrolled loop and in the tail, keep their own record slots; a word with
several bad dwords is recorded dword by dword; nothing of an earlier launch or of a neighbouring wave is reported;
``invert`` and ``origin`` reach the records; two threads never see each other's report; the FULL level runs all its
114 passes clean and finds one flip per triple; and ``gsx-memtest`` carries its origin from chunk to chunk.

Errors are placed by wave, lane and trip with ``tests/memtest_cases.py`` (checked on the CPU by
``tests/test_memtest_cases.py``), sized from the device's CU count.  Everything is exact: no tolerances."""
import functools
import json
import subprocess
import threading
import time
from pathlib import Path

import numpy as np
import pytest

from gpushare_scheduler_extender_amd.ops import memtest as mt
from tests import memtest_cases as mc

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
TOOL = ROOT / "gpushare_scheduler_extender_amd" / "_native" / "gsx-memtest"
GUARD = 4096
GUARD_PAT = 0xC3C3C3C3
LO = GUARD + 16  # the range starts 16 bytes past a 4 KiB boundary
SMALL = (1 << 20) + 16  # one of test_gpu_memtest.py's SIZES: below the cap, four words per lane
CROSSING = 2**36 - (8 << 20)  # W crosses 2**32 eight MiB into the range
FULL_BYTES = (16 << 20) + 48  # what the FULL level runs over
MAX_ERRS = mt.MAX_ERRS
PATTERNS = sorted(mt.PATTERNS.values())


@pytest.fixture(scope="module")
def hip():
    from gpushare_scheduler_extender_amd.ops import hip as h

    assert h.SO.exists() and h.device_count() > 0, "gpu tests need a GPU and the built kernels"
    return h


@pytest.fixture(scope="module")
def cus(hip):
    return hip.device_info(0)["cu_count"]


@pytest.fixture(scope="module")
def stream(hip):
    s = hip.Stream(0)
    yield s
    s.destroy()


@pytest.fixture(scope="module")
def buf(hip, cus):
    """Guard + the largest range of this file + guard."""
    b = hip.DeviceBuffer(0, LO + max(mc.CAPPED2(cus), FULL_BYTES, 2 * SMALL) + GUARD)
    yield b
    b.free()


@functools.lru_cache(maxsize=3)
def twin(pattern, seed, origin, nbytes):
    """The non-inverted twin of a whole range, computed once and shared read-only."""
    w = mt.memtest_words(pattern, seed, 0, origin, nbytes)
    w.setflags(write=False)
    return w


def words(buf, nbytes, offset=0) -> np.ndarray:
    return np.frombuffer(buf.to_host(nbytes, offset), dtype=np.uint32)


def lay(hip, s, buf, n, origin, pattern, seed, invert=False):
    """Guards around ``n`` bytes of the pattern at ``LO``."""
    hip.hbm_fill(s, buf.addr(0), LO + n + GUARD, GUARD_PAT)
    hip.memtest_write(s, buf.addr(LO), n, origin, pattern, seed, invert)
    s.sync()


def patch(buf, plan):
    for off, value in plan.patches:
        buf.from_host(value.to_bytes(4, "little"), LO + off)


def guards_intact(buf, n):
    return bool((words(buf, LO) == GUARD_PAT).all() and (words(buf, GUARD, LO + n) == GUARD_PAT).all())


def assert_report(rep, plan, ctx=None):
    """The order-free properties of every report."""
    errs = rep.errors()
    assert rep.bad_dwords == plan.bad_dwords, (ctx, rep.bad_dwords, plan.bad_dwords)
    assert rep.flipped_or == plan.flipped_or, (ctx, hex(rep.flipped_or), hex(plan.flipped_or))
    assert rep.n_errs == min(plan.bad_dwords, MAX_ERRS) == len(errs), (ctx, rep.n_errs)
    assert len(set(errs)) == len(errs), (ctx, "a record twice", errs)
    assert set(errs) <= plan.records, (ctx, "records that are no errors", sorted(set(errs) - plan.records))
    if plan.bad_dwords <= MAX_ERRS:
        assert set(errs) == plan.records, (ctx, "missing", sorted(plan.records - set(errs)))


def one_wave_layout(block, wave):
    """10 bad dwords of one wave: 3 at trip 0 and 2 at trip 2 (one unrolled iteration, lane 5 in both and two other
    lanes), a word with all four dwords bad at trip 5 (the second iteration) and 1 at trip 8 (the tail)."""
    return [(block, wave, 5, 0, 1, 0x10), (block, wave, 5, 0, 3, 0x8000_0000), (block, wave, 40, 0, 0, 0x1),
            (block, wave, 5, 2, 2, 0x300), (block, wave, 17, 2, 0, 0x4000),
            *[(block, wave, 9, 5, d, 0x0101_0101 << d) for d in range(4)],
            (block, wave, 63, 8, 2, 0x2)]


# ---------------------------------------------------------------- (a) one wave, several steps

@pytest.mark.parametrize("rewrite", [False, True], ids=["check", "check+rewrite"])
@pytest.mark.parametrize("pattern", [mt.ADDR, mt.RANDOM], ids=["ADDR", "RANDOM"])
def test_errors_of_one_wave_at_several_steps(hip, stream, buf, cus, pattern, rewrite):
    n, origin, seed = mc.CAPPED2(cus), CROSSING, 5
    geo = mc.geometry(n, cus)
    assert (geo.unrolled, geo.tail) == (2, 2)
    flips = [*one_wave_layout(geo.grid // 3, 2), *one_wave_layout(geo.grid - 1, 3),
             (0, 0, 2, 9, 1, 0x0008_0000)]  # and the ragged wave's last live lane in its last step
    plan = mc.flip_plan(flips, geo, pattern, seed, 0, origin)
    assert plan.bad_dwords == 21
    lay(hip, stream, buf, n, origin, pattern, seed)
    patch(buf, plan)
    rep = hip.memtest_check(stream, buf.addr(LO), n, origin, pattern, seed, rewrite=rewrite)
    assert_report(rep, plan, (pattern, rewrite))
    assert rep.errors() == list(plan.ordered)  # and the order: waves by index, a wave's steps one after the other
    if rewrite:
        # the range now holds the complement everywhere, the patched words included; nothing else was touched
        got = words(buf, n, LO)
        want = twin(pattern, seed, origin, n)
        assert (got == ~want).all(), int(np.flatnonzero(got != ~want)[0])
        assert guards_intact(buf, n)
        rep = hip.memtest_check(stream, buf.addr(LO), n, origin, pattern, seed, invert=True)
        assert (rep.bad_dwords, rep.flipped_or, rep.n_errs) == (0, 0, 0)


# ---------------------------------------------------------------- (b) the write path over two unrolled iterations

@pytest.mark.parametrize("pattern", PATTERNS)
def test_write_over_two_unrolled_iterations_equals_the_twin(hip, stream, buf, cus, pattern):
    n, origin, seed = mc.CAPPED2(cus), CROSSING, 0x9E3779B9
    assert origin // 16 < 2**32 < origin // 16 + n // 16
    want = twin(pattern, seed, origin, n)
    for invert in (0, 1):
        lay(hip, stream, buf, n, origin, pattern, seed, bool(invert))
        got = words(buf, n, LO)
        ref = ~want if invert else want
        if not (got == ref).all():
            k = int(np.flatnonzero(got != ref)[0])
            raise AssertionError(f"{(pattern, invert)}: dword {k} is {got[k]:#x}, twin says {ref[k]:#x}")
        assert guards_intact(buf, n), (pattern, invert)


# ---------------------------------------------------------------- (c) the cap, and the neighbouring wave

def test_slots_run_out_inside_a_step_and_the_neighbour_wave_keeps_its_own(hip, stream, buf, cus):
    n, origin, pattern, seed = mc.CAPPED2(cus), 48, mt.RANDOM, 3
    geo = mc.geometry(n, cus)
    block, w = geo.grid // 2, 1
    first = [(block, w, lane, 0, lane // 2 % 4, 1 << (lane % 32)) for lane in range(2, 62, 2)]  # one dword each
    full = [(block, w, lane, trip, d, 0xFFFFFFFF) for lane, trip in ((7, 4), (20, 5), (50, 4)) for d in range(4)]
    other = [(block, w + 1, 3, 6, 0, 0x40), (block, w + 1, 3, 6, 2, 0x80)]
    assert len(first) == 30
    plan = mc.flip_plan(first + full + other, geo, pattern, seed, 0, origin)
    lay(hip, stream, buf, n, origin, pattern, seed)
    patch(buf, plan)
    rep = hip.memtest_check(stream, buf.addr(LO), n, origin, pattern, seed)
    assert_report(rep, plan)
    assert rep.bad_dwords == 44 and rep.n_errs == 32
    # the 30 of trip 0 in lane order, then dwords 0 and 1 of the lowest of the three lanes: the wave's prefix-sum
    # order, its second step starting at slot 30, and the host merging waves in index order
    want = [*mc.flip_plan(first, geo, pattern, seed, 0, origin).ordered,
            *mc.flip_plan(full[:2], geo, pattern, seed, 0, origin).ordered]
    assert [off for off, _e, _a in want[:30]] == [origin + 16 * mc.word_of(block, w, lane, 0, geo) + 4 * (lane // 2 % 4)
                                                  for lane in range(2, 62, 2)]
    assert [off for off, _e, _a in want[30:]] == [origin + 16 * mc.word_of(block, w, 7, 4, geo) + d for d in (0, 4)]
    assert rep.errors() == want == list(plan.ordered[:32])
    # wave w repaired from the host: what is left is wave w + 1's, which no store of wave w has touched
    good = twin(pattern, seed, origin, n)
    for off, _value in mc.flip_plan(first + full, geo, pattern, seed, 0, origin).patches:
        buf.from_host(int(good[off // 4]).to_bytes(4, "little"), LO + off)
    rep = hip.memtest_check(stream, buf.addr(LO), n, origin, pattern, seed)
    rest = mc.flip_plan(other, geo, pattern, seed, 0, origin)
    assert_report(rep, rest)
    assert rep.errors() == list(rest.ordered) and rep.n_errs == 2


# ---------------------------------------------------------------- (d) nothing stale from an earlier launch

@pytest.mark.parametrize("size", ["small", "capped2"])
def test_nothing_of_an_earlier_launch_is_reported(hip, stream, buf, cus, size):
    n = SMALL if size == "small" else mc.CAPPED2(cus)
    geo = mc.geometry(n, cus)
    origin, pattern, seed = 0, mt.RANDOM, 11
    lay(hip, stream, buf, n, origin, pattern, seed)
    rep = hip.memtest_check(stream, buf.addr(LO), n, origin, pattern, seed + 1)  # the wrong seed: bad throughout
    assert rep.n_errs == 32 and rep.flipped_or == 0xFFFFFFFF and n // 4 - 16 <= rep.bad_dwords <= n // 4
    assert len(set(rep.errors())) == 32
    for off, e, a in rep.errors():
        assert e == mc.expected_dword(pattern, seed + 1, 0, origin, off) != a
        assert a == mc.expected_dword(pattern, seed, 0, origin, off)
    rep = hip.memtest_check(stream, buf.addr(LO), n, origin, pattern, seed)
    assert (rep.bad_dwords, rep.flipped_or, rep.n_errs) == (0, 0, 0)
    assert all(e.offset == 0 and e.expected == 0 and e.actual == 0 for e in rep.errs)
    # one flip in a wave whose 32 slots the first launch filled, at its last trip
    block, wave = geo.grid // 2, 2
    u, t = geo.wave_trips(block, wave)
    plan = mc.flip_plan([(block, wave, 21, 4 * u + t - 1, 3, 0x0002_0000)], geo, pattern, seed, 0, origin)
    patch(buf, plan)
    rep = hip.memtest_check(stream, buf.addr(LO), n, origin, pattern, seed)
    assert_report(rep, plan, size)
    assert rep.errors() == list(plan.ordered) and rep.n_errs == 1


# ---------------------------------------------------------------- (e) invert

@pytest.mark.parametrize("pattern", PATTERNS)
def test_records_under_invert_hold_the_complement(hip, stream, buf, cus, pattern):
    n, origin, seed = SMALL, 2**36 - (1 << 19), 0x55555555 if pattern == mt.SOLID else 6
    geo = mc.geometry(n, cus)
    plain = twin(pattern, seed, origin, n)
    places = [(0, 0, 0, 0, 0, 0x1), (geo.grid // 2, 3, 63, 1, 2, 0x8000_0000),
              (*mc.owner_of(geo.n16 - 1, geo), 3, 0x0FF0)]  # the first word, a block's last lane, the last word
    lay(hip, stream, buf, n, origin, pattern, seed, invert=True)
    plan = mc.flip_plan(places, geo, pattern, seed, 1, origin)
    for off, e, _a in plan.ordered:
        assert e == int(~plain[(off - origin) // 4])
    patch(buf, plan)
    rep = hip.memtest_check(stream, buf.addr(LO), n, origin, pattern, seed, invert=True, rewrite=True)
    assert_report(rep, plan, pattern)
    # that pass left the complement of the inverted pattern: the plain one, the patched dwords included
    assert (words(buf, n, LO) == plain).all() and guards_intact(buf, n)
    moved = [(b, w, ln, t, (d + 1) % 4, m) for b, w, ln, t, d, m in places]
    plan = mc.flip_plan(moved, geo, pattern, seed, 0, origin)
    for off, e, _a in plan.ordered:
        assert e == int(plain[(off - origin) // 4])
    patch(buf, plan)
    rep = hip.memtest_check(stream, buf.addr(LO), n, origin, pattern, seed, invert=False)
    assert_report(rep, plan, pattern)


# ---------------------------------------------------------------- (f) accumulation across chunks

def test_two_halves_accumulate_into_one_report_with_their_origins(hip, stream, buf, cus):
    half, pattern, seed = SMALL, mt.ADDR, 0
    geo = mc.geometry(half, cus)
    lay(hip, stream, buf, 2 * half, 0, pattern, seed)
    a = mc.flip_plan([(1, 0, 4, 0, 0, 0x4), (geo.grid - 2, 2, 9, 2, 1, 0x400)], geo, pattern, seed, 0, 0)
    b = mc.flip_plan([(0, 1, 0, 1, 2, 0x8), (1, 3, 60, 3, 3, 0x800)], geo, pattern, seed, 0, half)
    patch(buf, a)
    for off, value in b.patches:
        buf.from_host(value.to_bytes(4, "little"), LO + half + off)
    rep = hip.memtest_check(stream, buf.addr(LO), half, 0, pattern, seed)
    hip.memtest_check(stream, buf.addr(LO + half), half, half, pattern, seed, report=rep)
    assert rep.bad_dwords == 4 and rep.n_errs == 4 and rep.flipped_or == 0xC0C
    assert rep.errors() == [*a.ordered, *b.ordered]
    assert all(off >= half for off, _e, _a in rep.errors()[2:]) and all(off < half for off, _e, _a in rep.errors()[:2])
    # the expected values are those of one range laid in one piece: ADDR words carry the global word index
    whole = twin(pattern, seed, 0, 2 * half)
    assert [e for _off, e, _a in rep.errors()] == [int(whole[off // 4]) for off, _e, _a in rep.errors()]


# ---------------------------------------------------------------- (g) two threads, one device

def test_concurrent_checks_never_mix_their_reports(hip, cus):
    """The pinned report of a device is shared: its reset -> launch -> read-back is serialised, so a thread that
    checks a clean range sees nothing of the thread that checks a bad one (ctypes drops the GIL: the calls overlap).
    A third thread writes and fills throughout; those paths take no lock."""
    n, pattern, seed, calls = SMALL, mt.RANDOM, 21, 200
    geo = mc.geometry(n, cus)
    bufs = [hip.DeviceBuffer(0, n) for _ in range(3)]
    streams = [hip.Stream(0) for _ in range(3)]
    plan = mc.flip_plan([(0, 0, 0, 0, 0, 0x1), (geo.grid // 2, 1, 30, 1, 1, 0x20), (geo.grid // 2, 1, 30, 3, 2, 0x300),
                         (geo.grid // 2, 2, 1, 2, 3, 0x4000), (*mc.owner_of(geo.n16 - 1, geo), 0, 0x8_0000)],
                        geo, pattern, seed, 0, 0)
    errs, done, stop = [], [], threading.Event()
    try:
        for b, s in zip(bufs, streams):
            hip.memtest_write(s, b.addr(0), n, 0, pattern, seed)
            s.sync()
        for off, value in plan.patches:
            bufs[1].from_host(value.to_bytes(4, "little"), off)

        def check(i):
            want = (0, 0, []) if i == 0 else (plan.bad_dwords, plan.flipped_or, list(plan.ordered))
            try:
                for k in range(calls):
                    rep = hip.memtest_check(streams[i], bufs[i].addr(0), n, 0, pattern, seed)
                    got = (rep.bad_dwords, rep.flipped_or, rep.errors())
                    if got != want:
                        errs.append((i, k, got, want))
                        return
                done.append(i)  # a call that raised ends its thread before this line
            finally:
                if i == 1:
                    stop.set()

        def write():
            k = 0
            while not stop.is_set() or k % 2:  # ends after a write, so that the buffer holds the pattern
                if k % 2:
                    hip.memtest_write(streams[2], bufs[2].addr(0), n, 0, pattern, seed)
                else:
                    hip.hbm_fill(streams[2], bufs[2].addr(0), n, 0xDEADBEEF)
                streams[2].sync()
                k += 1
            done.append(2)

        ts = [threading.Thread(target=check, args=(0,)), threading.Thread(target=check, args=(1,)),
              threading.Thread(target=write)]
        for t in ts:
            t.start()
        ts[0].join(), ts[1].join()
        stop.set()  # also when thread 1 ended by an exception
        ts[2].join()
        assert not errs, errs[:3]
        assert sorted(done) == [0, 1, 2], done
        assert (words(bufs[2], n) == twin(pattern, seed, 0, n)).all()
    finally:
        stop.set()
        for b, s in zip(bufs, streams):
            b.free()
            s.destroy()


# ---------------------------------------------------------------- (h) the FULL level

def test_full_level_runs_clean_and_finds_one_flip_per_triple(hip, stream, buf, cus):
    n, origin = FULL_BYTES, CROSSING
    geo = mc.geometry(n, cus)
    hip.hbm_fill(stream, buf.addr(0), LO + n + GUARD, GUARD_PAT)
    t0 = time.perf_counter()
    rep, passes, seconds = hip.memtest_run(stream, buf.addr(LO), n, origin, level="full")
    print(f"memtest full level over 16 MiB: {passes} passes, {seconds:.3f} s ({time.perf_counter() - t0:.3f} s wall)")
    assert passes == mt.level_passes("full") == 114
    assert (rep.bad_dwords, rep.n_errs, rep.flipped_or) == (0, 0, 0) and seconds > 0
    assert (words(buf, 1 << 20, LO + n - (1 << 20))
            == mt.memtest_words(mt.WALK, 31, 1, origin + n - (1 << 20), 1 << 20)).all()
    assert guards_intact(buf, n)
    # the same table by hand into one report, with one dword flipped after every write pass
    table = hip.memtest_pass_table("full")
    assert table == mt.LEVELS["full"] and len(table) == 3 * 38
    flips = mc.full_level_flips(geo, 38)
    rep = hip.MemtestReport()
    want, flipped = [], 0
    for k in range(38):
        (o0, pattern, seed, i0, r0), (o1, _p1, _s1, i1, r1), (o2, _p2, _s2, i2, r2) = table[3 * k:3 * k + 3]
        assert (o0, i0, r0, o1, i1, r1, o2, i2, r2) == ("write", 0, 0, "check", 0, 1, "check", 1, 0)
        hip.memtest_write(stream, buf.addr(LO), n, origin, pattern, seed)
        stream.sync()
        plan = mc.flip_plan([flips[k]], geo, pattern, seed, 0, origin)
        patch(buf, plan)
        want += plan.ordered
        flipped |= plan.flipped_or
        hip.memtest_check(stream, buf.addr(LO), n, origin, pattern, seed, rewrite=True, report=rep)
        assert rep.bad_dwords == k + 1 and rep.n_errs == min(k + 1, 32) and rep.flipped_or == flipped, (k, flips[k])
        hip.memtest_check(stream, buf.addr(LO), n, origin, pattern, seed, invert=True, report=rep)
        assert rep.bad_dwords == k + 1 and rep.n_errs == min(k + 1, 32), (k, "the rewrite did not repair", flips[k])
    assert rep.bad_dwords == 38 and rep.n_errs == 32
    assert rep.errors() == want[:32]  # the first 32 triples' flips, in call order
    assert guards_intact(buf, n)
    # One launch finds one flip above, so no wave wrote a second record.  Below the cap the grid's last waves never
    # enter the unrolled loop: errors at the first, a middle and the last step of such a wave keep their slots too
    block, wave = geo.grid - 1, 3
    u, t = geo.wave_trips(block, wave)
    if cus == 256:
        assert (u, t) == (0, 3)
    trips = sorted({0, (4 * u + t) // 2, 4 * u + t - 1})
    plan = mc.flip_plan([(block, wave, 0 if k else 63, trip, k + 1, 0x11 << k) for k, trip in enumerate(trips)],
                        geo, mt.RANDOM, 1, 0, origin)
    hip.memtest_write(stream, buf.addr(LO), n, origin, mt.RANDOM, 1)
    stream.sync()
    patch(buf, plan)
    rep = hip.memtest_check(stream, buf.addr(LO), n, origin, mt.RANDOM, 1)
    assert_report(rep, plan)
    assert rep.errors() == list(plan.ordered) and rep.n_errs == len(trips)


# ---------------------------------------------------------------- gsx-memtest with more than one chunk

CHUNK = 1 << 30
TOOL_BYTES = CHUNK + (32 << 20) + 16


def run_tool(*argv):
    r = subprocess.run([str(TOOL), *argv], capture_output=True, text=True, timeout=120)
    return r.returncode, json.loads(r.stdout.strip().splitlines()[-1])


def test_tool_carries_the_origin_into_its_second_chunk(hip):
    off, mask = CHUNK + (4 << 20) + 8, 0x100
    rc, out = run_tool("--device", "0", "--bytes", str(TOOL_BYTES), "--chunk", str(CHUNK), "--level", "quick",
                       "--inject", f"{off}:{mask:#010x}")
    assert rc == 1, out
    assert out["chunks"] == 2 and out["bytes_tested"] == TOOL_BYTES and out["error"] is None and not out["truncated"]
    assert out["bytes_moved"] == mt.bytes_moved("quick", TOOL_BYTES) and out["passes"] == 2 * mt.level_passes("quick")
    e = mc.expected_dword(mt.ADDR, 0, 0, 0, off)  # the first write pass of a chunk is ADDR, seed 0
    assert e == int(mt.memtest_words(mt.ADDR, 0, 0, CHUNK, TOOL_BYTES - CHUNK)[(off - CHUNK) // 4])
    assert out["bad_dwords"] == 1 and out["flipped_or"] == mask
    assert out["errors"] == [{"offset": off, "expected": e, "actual": e ^ mask}]


def test_tool_truncated_before_its_first_pass(hip):
    rc, out = run_tool("--device", "0", "--bytes", str(TOOL_BYTES), "--chunk", str(CHUNK), "--level", "quick",
                       "--max-seconds", "0.000001")
    assert rc == 0, out
    assert out["truncated"] is True and out["passes"] == 0 and out["bytes_tested"] == 0 and out["error"] is None
    assert out["chunks"] == 0 and out["bytes_moved"] == 0 and out["bad_dwords"] == 0 and out["errors"] == []


def test_tool_and_library_run_the_same_passes_over_one_range(hip, stream):
    n = 32 << 20
    rc, out = run_tool("--device", "0", "--bytes", str(n), "--level", "quick")
    assert rc == 0 and out["error"] is None and not out["truncated"], out
    b = hip.DeviceBuffer(0, n)
    try:
        rep, passes, _seconds = hip.memtest_run(stream, b.addr(0), n, 0, level="quick")
    finally:
        b.free()
    assert out["passes"] == passes == 6 and out["bytes_moved"] == 8 * n
    assert (out["chunks"], out["bytes_tested"], out["bad_dwords"], rep.bad_dwords) == (1, n, 0, 0)


def test_tool_with_a_reserve_beyond_the_device(hip):
    _free, total = hip.mem_info(0)
    rc, out = run_tool("--device", "0", "--bytes", "all", "--reserve", str(total + (1 << 30)))
    assert rc == 2, out
    assert "no free memory beyond --reserve" in out["error"] and out["bytes_tested"] == 0 and out["passes"] == 0
