"""The HBM pre-flight memory test on a real MI355X (native/kernels/memtest.hip, gsx-memtest): what the kernels write
is the NumPy twin byte for byte, every injected error is counted and reported exactly, the moving-inversions pass
repairs what it reports, byte offsets past 4 GiB work, and the passes run at HBM bandwidth.

Word indices past 2**32 are covered through ``origin`` (the generator's 64-bit W); word indices past 2**32 in the
*addressing* would need a 64 GiB buffer and are covered by review only."""
import json
import subprocess
import time
from pathlib import Path

import numpy as np
import pytest

from gpushare_scheduler_extender_amd.ops import memtest as mt

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
TOOL = ROOT / "gpushare_scheduler_extender_amd" / "_native" / "gsx-memtest"
GUARD = 4096
GUARD_PAT = 0xC3C3C3C3
# one word; under one block; one word past a block; tails on both sides of the unrolled loop (the grid is
# ceil(words / 1024) blocks below 32 MiB, so every lane's four words end right around these sizes)
SIZES = [16, 4080, 4096 + 16, (1 << 20) + 16, (3 << 20) - 16]
# past 32 MiB the grid stops growing (8 blocks per CU): at 256 CUs this is 5 grid steps + 3 words, so every wave
# makes exactly one iteration of the unrolled loop, one tail step with all lanes live and, in block 0's wave 0, a
# second with three (tests/test_memtest_cases.py pins this).  Two unrolled iterations with every dword compared:
# CAPPED2 of tests/memtest_cases.py, in tests/test_gpu_memtest_report.py
CAPPED = (40 << 20) + 48
ORIGINS = [0, 48, 2**36 - (1 << 20)]  # the last crosses W = 2**32 inside the 1 MiB+ buffers
BIG = (4 << 30) + (2 << 20)


@pytest.fixture(scope="module")
def hip():
    from gpushare_scheduler_extender_amd.ops import hip as h

    assert h.SO.exists() and h.device_count() > 0, "gpu tests need a GPU and the built kernels"
    return h


@pytest.fixture(scope="module")
def stream(hip):
    s = hip.Stream(0)
    yield s
    s.destroy()


@pytest.fixture(scope="module")
def small(hip):
    """Guard + range + guard for the largest of SIZES; the range starts 16 bytes past a 4 KiB boundary."""
    buf = hip.DeviceBuffer(0, GUARD + 16 + max(SIZES) + GUARD)
    yield buf
    buf.free()


@pytest.fixture(scope="module")
def big(hip):
    buf = hip.DeviceBuffer(0, BIG)
    yield buf
    buf.free()


def words(buf, nbytes, offset=0) -> np.ndarray:
    return np.frombuffer(buf.to_host(nbytes, offset), dtype=np.uint32)


def write_and_compare(hip, s, buf, pattern, seed, invert, nbytes, origin):
    lo = GUARD + 16  # the range: only 16-B aligned
    total = lo + nbytes + GUARD
    hip.hbm_fill(s, buf.addr(0), total, GUARD_PAT)
    hip.memtest_write(s, buf.addr(lo), nbytes, origin, pattern, seed, bool(invert))
    s.sync()
    got = words(buf, total)
    want = mt.memtest_words(pattern, seed, invert, origin, nbytes)
    ctx = (pattern, seed, invert, nbytes, origin)
    assert (got[:lo // 4] == GUARD_PAT).all(), ("guard before", ctx)
    assert (got[(lo + nbytes) // 4:] == GUARD_PAT).all(), ("guard after", ctx)
    body = got[lo // 4:(lo + nbytes) // 4]
    if not (body == want).all():
        k = int(np.flatnonzero(body != want)[0])
        raise AssertionError(f"{ctx}: dword {k} is {body[k]:#x}, twin says {want[k]:#x}")


def test_hbm_fill_stays_in_its_range(hip, stream):
    """Fill is the SOLID write pass: its tail, a range that is only 16-B aligned, and its bounds.  The guards are laid
    by a host copy, since ``write_and_compare`` lays its own with the fill under test here."""
    lo = GUARD + 16
    for nbytes in [*SIZES, CAPPED]:
        total = lo + nbytes + GUARD
        buf = hip.DeviceBuffer(0, total)
        try:
            buf.from_host(np.full(total // 4, GUARD_PAT, dtype=np.uint32).tobytes())
            hip.hbm_fill(stream, buf.addr(lo), nbytes, 0x1234ABCD)
            stream.sync()
            got = words(buf, total)
        finally:
            buf.free()
        assert (got[:lo // 4] == GUARD_PAT).all(), ("guard before", nbytes)
        assert (got[(lo + nbytes) // 4:] == GUARD_PAT).all(), ("guard after", nbytes)
        assert (got[lo // 4:(lo + nbytes) // 4] == 0x1234ABCD).all(), ("range", nbytes)


@pytest.mark.parametrize("pattern", sorted(mt.PATTERNS.values()))
def test_write_equals_the_numpy_twin(hip, stream, small, pattern):
    for seed in (0, 0x9E3779B9):
        for invert in (0, 1):
            for nbytes in SIZES:
                for origin in ORIGINS:
                    write_and_compare(hip, stream, small, pattern, seed, invert, nbytes, origin)


def test_write_equals_the_twin_where_the_grid_is_capped(hip, stream):
    buf = hip.DeviceBuffer(0, GUARD + 16 + CAPPED + GUARD)
    try:
        for pattern in (mt.ADDR, mt.RANDOM):
            write_and_compare(hip, stream, buf, pattern, 5, 0, CAPPED, ORIGINS[2])
        # and the checks walk the same range: clean, then every error of a sparse set found
        base = buf.addr(GUARD + 16)
        rep = hip.memtest_check(stream, base, CAPPED, ORIGINS[2], mt.RANDOM, 5)
        assert (rep.bad_dwords, rep.flipped_or, rep.n_errs) == (0, 0, 0)
        want = mt.memtest_words(mt.RANDOM, 5, 0, ORIGINS[2], CAPPED)
        at = [0, 4 * 1024 * 1024 + 4, CAPPED // 2 + 8, (36 << 20) + 12, CAPPED - 4]
        for off in at:
            buf.from_host(int(want[off // 4] ^ 0x10).to_bytes(4, "little"), GUARD + 16 + off)
        rep = hip.memtest_check(stream, base, CAPPED, ORIGINS[2], mt.RANDOM, 5)
        assert rep.bad_dwords == len(at) and rep.flipped_or == 0x10
        assert sorted(rep.errors()) == [(ORIGINS[2] + off, int(want[off // 4]), int(want[off // 4]) ^ 0x10)
                                        for off in at]
    finally:
        buf.free()


@pytest.mark.parametrize("pattern", sorted(mt.PATTERNS.values()))
def test_clean_check_reports_nothing(hip, stream, small, pattern):
    for nbytes in SIZES:
        for invert in (False, True):
            base = small.addr(GUARD + 16)
            hip.memtest_write(stream, base, nbytes, 48, pattern, 0xAAAAAAAA, invert)
            rep = hip.memtest_check(stream, base, nbytes, 48, pattern, 0xAAAAAAAA, invert)
            assert (rep.bad_dwords, rep.flipped_or, rep.n_errs) == (0, 0, 0), (pattern, nbytes, invert)
            assert all(e.offset == 0 and e.expected == 0 and e.actual == 0 for e in rep.errs)


def corrupt(buf, lo, want, flips):
    """XOR ``mask`` into the dword at byte ``off`` of the range for every ``(off, mask)``; the expected records."""
    out = []
    for off, mask in flips:
        e = int(want[off // 4])
        buf.from_host((e ^ mask).to_bytes(4, "little"), lo + off)
        out.append((off, e, e ^ mask))
    return out


def test_single_bit_flips_are_reported_exactly(hip, stream, small):
    n, lo, origin = (1 << 20) + 16, GUARD + 16, 48
    for pattern in sorted(mt.PATTERNS.values()):
        hip.memtest_write(stream, small.addr(lo), n, origin, pattern, 3)
        stream.sync()
        want = mt.memtest_words(pattern, 3, 0, origin, n)
        flips = [(0, 1 << 0), (n - 4, 1 << 31), (n // 2 + 4, 1 << 13)]  # first dword, last dword, one in the middle
        recs = corrupt(small, lo, want, flips)
        rep = hip.memtest_check(stream, small.addr(lo), n, origin, pattern, 3)
        assert rep.bad_dwords == 3 and rep.n_errs == 3, (pattern, rep.bad_dwords, rep.n_errs)
        assert sorted(rep.errors()) == sorted((origin + off, e, a) for off, e, a in recs), pattern
        assert rep.flipped_or == (1 << 0) | (1 << 31) | (1 << 13)


def test_check_with_rewrite_reports_and_repairs(hip, stream, small):
    n, lo = (1 << 20) + 16, GUARD + 16
    for pattern in (mt.ADDR, mt.RANDOM, mt.WALK):
        hip.hbm_fill(stream, small.addr(0), lo + n + GUARD, GUARD_PAT)
        hip.memtest_write(stream, small.addr(lo), n, 0, pattern, 1)
        stream.sync()
        want = mt.memtest_words(pattern, 1, 0, 0, n)
        recs = corrupt(small, lo, want, [(16, 0xFF), (n - 16, 0x8000_0001), (4096 * 33 + 8, 0x10)])
        rep = hip.memtest_check(stream, small.addr(lo), n, 0, pattern, 1, rewrite=True)
        assert rep.bad_dwords == 3 and sorted(rep.errors()) == sorted(recs)
        assert rep.flipped_or == 0xFF | 0x8000_0001 | 0x10
        # the whole range now holds the complement, the corrupted words included, and nothing else was touched
        got = words(small, lo + n + GUARD)
        assert (got[lo // 4:(lo + n) // 4] == ~want).all()
        assert (got[:lo // 4] == GUARD_PAT).all() and (got[(lo + n) // 4:] == GUARD_PAT).all()
        rep = hip.memtest_check(stream, small.addr(lo), n, 0, pattern, 1, invert=True)
        assert (rep.bad_dwords, rep.n_errs, rep.flipped_or) == (0, 0, 0)


def test_more_errors_than_slots(hip, stream, small):
    n, lo, origin = (1 << 20) + 16, GUARD + 16, 2**36 - (1 << 20)
    hip.memtest_write(stream, small.addr(lo), n, origin, mt.RANDOM, 9)
    stream.sync()
    want = mt.memtest_words(mt.RANDOM, 9, 0, origin, n)
    at = 300 * 1024 + 16  # 4 KiB of complemented data somewhere inside
    small.from_host((want[at // 4:at // 4 + 1024] ^ np.uint32(0xFFFFFFFF)).tobytes(), lo + at)
    rep = hip.memtest_check(stream, small.addr(lo), n, origin, mt.RANDOM, 9)
    assert rep.bad_dwords == 1024 and rep.n_errs == 32 and rep.flipped_or == 0xFFFFFFFF
    errs = rep.errors()
    assert len({off for off, _, _ in errs}) == 32
    for off, e, a in errs:  # every record truthful
        rel = off - origin
        assert at <= rel < at + 4096 and rel % 4 == 0
        assert e == int(want[rel // 4]) and a == e ^ 0xFFFFFFFF
    # accumulation: a second check into the same report adds its count and keeps the 32 records
    hip.memtest_check(stream, small.addr(lo), n, origin, mt.RANDOM, 9, report=rep)
    assert rep.bad_dwords == 2048 and rep.n_errs == 32


def test_byte_offsets_past_4_gib(hip, stream, big):
    hip.memtest_write(stream, big.addr(0), BIG, 0, mt.ADDR, 0)
    stream.sync()
    tail = words(big, 2 << 20, 4 << 30)
    assert (tail == mt.memtest_words(mt.ADDR, 0, 0, 4 << 30, 2 << 20)).all()
    off = 2**32 + (1 << 20)
    e = int(mt.memtest_words(mt.ADDR, 0, 0, off, 16)[0])
    big.from_host((e ^ 0x40).to_bytes(4, "little"), off)
    rep = hip.memtest_check(stream, big.addr(0), BIG, 0, mt.ADDR, 0)
    assert rep.bad_dwords == 1 and rep.errors() == [(off, e, e ^ 0x40)] and rep.flipped_or == 0x40


def test_run_quick_matches_the_python_table(hip, stream):
    n = 64 << 20
    for level in ("quick", "full"):
        assert hip.memtest_pass_table(level) == mt.LEVELS[level]
    buf = hip.DeviceBuffer(0, n)
    try:
        rep, passes, seconds = hip.memtest_run(stream, buf.addr(0), n, 1 << 30, "quick")
        assert passes == mt.level_passes("quick") == 6
        assert mt.bytes_moved("quick", n, passes) == 8 * n
        assert (rep.bad_dwords, rep.n_errs, rep.flipped_or) == (0, 0, 0) and seconds > 0
        # the last triple leaves the complement of RANDOM, seed 0, at this origin
        assert (words(buf, 1 << 20, n - (1 << 20))
                == mt.memtest_words(mt.RANDOM, 0, 1, (1 << 30) + n - (1 << 20), 1 << 20)).all()
    finally:
        buf.free()


def run_tool(*argv):
    r = subprocess.run([str(TOOL), *argv], capture_output=True, text=True, timeout=120)
    return r.returncode, json.loads(r.stdout.strip().splitlines()[-1])


def test_tool_clean_run(hip):
    rc, out = run_tool("--device", "0", "--bytes", "268435456", "--level", "quick")
    assert rc == 0, out
    assert out["bad_dwords"] == 0 and out["bytes_tested"] == 268435456 and out["error"] is None
    assert out["passes"] == mt.level_passes("quick") and out["bytes_moved"] == mt.bytes_moved("quick", 268435456)
    assert out["errors"] == [] and not out["truncated"] and out["bdf"] and out["gbps"] > 0


def test_tool_finds_an_injected_flip(hip):
    rc, out = run_tool("--device", "0", "--bytes", "268435456", "--level", "quick", "--inject", "4096:0x00000100")
    assert rc == 1, out
    e = int(mt.memtest_words(mt.ADDR, 0, 0, 4096, 16)[0])
    assert out["bad_dwords"] == 1 and out["flipped_or"] == 0x100
    assert out["errors"] == [{"offset": 4096, "expected": e, "actual": e ^ 0x100}]
    assert out["bytes_tested"] == 268435456 and out["error"] is None


def rate(n_bytes, calls, fn, sync):
    """TB/s of ``calls`` runs of ``fn`` by the host clock; the timed work ends in a stream sync."""
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    sync()
    return calls * n_bytes / (time.perf_counter() - t0) / 1e12


def test_bandwidth(hip, stream, big):
    n, base, calls = 4 << 30, big.addr(0), 3
    fill = lambda: hip.hbm_fill(stream, base, n, 7)  # noqa: E731
    write = lambda: hip.memtest_write(stream, base, n, 0, mt.RANDOM, 1)  # noqa: E731
    inv = [False]

    def check():
        rep = hip.memtest_check(stream, base, n, 0, mt.RANDOM, 1, invert=inv[0])
        assert rep.bad_dwords == 0

    def check_rewrite():  # every pass leaves the complement of what it found
        rep = hip.memtest_check(stream, base, n, 0, mt.RANDOM, 1, invert=inv[0], rewrite=True)
        assert rep.bad_dwords == 0
        inv[0] = not inv[0]

    fill(), write(), check(), check_rewrite(), check_rewrite()  # warm-up: every kernel loaded, the report allocated
    stream.sync()
    rows = {"fill": [], "write": [], "check": [], "check+rewrite": []}
    for _ in range(3):  # interleaved: every repeat measures all four
        rows["fill"].append(rate(n, calls, fill, stream.sync))
        rows["write"].append(rate(n, calls, write, stream.sync))
        inv[0] = False
        rows["check"].append(rate(n, calls, check, stream.sync))
        rows["check+rewrite"].append(rate(2 * n, calls + 1, check_rewrite, stream.sync))  # an even count
    for name, r in rows.items():
        print(f"memtest bandwidth {name}: {' '.join(f'{x:.2f}' for x in r)} TB/s "
              f"(median {sorted(r)[1]:.2f}, spread {max(r) - min(r):.2f})")
    for name in ("write", "check", "check+rewrite"):
        assert sorted(rows[name])[1] > 2.0, (name, rows[name])  # the floor fill is held to; a broken kernel is far below


def test_a_completely_bad_range_costs_what_a_clean_one_costs(hip, stream, big):
    """A dead stack is the case the test exists for.  On top of a clean pass every wave makes one read of the claim
    counter, at most one claim and its one end-of-launch update: a few host round trips per wave, overlapped across
    the 8192 waves of a launch, against a millisecond of HBM traffic -- so the clean pass's floor holds here too."""
    n, base = 4 << 30, big.addr(0)
    hip.memtest_write(stream, base, n, 0, mt.RANDOM, 1)
    clean = lambda: hip.memtest_check(stream, base, n, 0, mt.RANDOM, 1)  # noqa: E731
    reps = []
    bad = lambda: reps.append(hip.memtest_check(stream, base, n, 0, mt.RANDOM, 2))  # noqa: E731 - the wrong seed
    clean(), bad()
    r_clean = rate(n, 3, clean, stream.sync)
    r_bad = rate(n, 3, bad, stream.sync)
    print(f"memtest bandwidth clean check {r_clean:.2f} TB/s, completely bad {r_bad:.2f} TB/s")
    want = mt.memtest_words(mt.RANDOM, 2, 0, 0, 1 << 20)
    got = mt.memtest_words(mt.RANDOM, 1, 0, 0, 1 << 20)
    assert (want != got).all()  # every dword of the first MiB differs; the count over 4 GiB is within a few of all
    for rep in reps:
        assert n // 4 - 16 <= rep.bad_dwords <= n // 4 and rep.n_errs == 32 and rep.flipped_or == 0xFFFFFFFF
        for off, e, a in rep.errors():
            assert off < 1 << 20 or (e != a and off % 4 == 0)
            if off < 1 << 20:
                assert e == int(want[off // 4]) and a == int(got[off // 4])
    assert r_bad > 2.0, (r_bad, r_clean)
