"""The compute pre-flight without a GPU: the NumPy twin of every unit's known answer, the native host twin and the
aggregation of per-wave records (pure host code of the library), ``gsx-cutest``'s argument handling, and the device
plugin's compute pre-flight driven through a stub tool, in the pattern of ``tests/test_memtest.py``."""
import asyncio
import json
import os
import stat
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest

from gpushare_scheduler_extender_amd.deviceplugin.plugin import device_tags
from gpushare_scheduler_extender_amd.k8s.objects import make_pod
from gpushare_scheduler_extender_amd.models.profile import SHARED_GPU
from gpushare_scheduler_extender_amd.ops import cutest as ct
from tests.test_memtest import BAD as MEM_BAD
from tests.test_memtest import Node as MemNode
from tests.test_memtest import Stub as MemStub
from tests.test_memtest import _alive, _health_polls

ROOT = Path(__file__).resolve().parents[1]
P = SHARED_GPU
NUNITS = len(ct.UNITS)


# ------------------------------------------------------------------ the NumPy twin

def test_unit_table():
    assert ct.UNITS == ("MFMA_BF16_16", "MFMA_BF16_32", "MFMA_F16", "MFMA_FP8", "MFMA_I8", "MFMA_F32", "VALU_F32",
                        "VALU_INT", "LDS")
    assert ct.SEEDS == {"quick": 8, "full": 256}
    assert ct.SHAPES[ct.UNIT_IDS["MFMA_BF16_32"]] == (32, 32, 16) and ct.SHAPES[ct.UNIT_IDS["MFMA_I8"]] == (16, 16, 64)
    assert ct.ROUNDS[ct.UNIT_IDS["MFMA_F32"]] == 32 and ct.ROUNDS[ct.UNIT_IDS["MFMA_FP8"]] == 64


def test_twin_is_deterministic():
    for u in range(NUNITS):
        assert ct.expected_signature(u, 5) == ct.expected_signature(u, 5)
        assert 0 <= ct.expected_signature(u, 5) < 1 << 64


def test_signatures_differ_across_units_and_seeds_except_valu_f32():
    sigs = {(u, s): ct.expected_signature(u, s) for u in range(NUNITS) for s in range(6)}
    mf, vf = ct.UNIT_IDS["MFMA_F32"], ct.UNIT_IDS["VALU_F32"]
    assert all(sigs[mf, s] == sigs[vf, s] for s in range(6))  # the same product, so the very same signature
    rest = [v for (u, _s), v in sigs.items() if u != vf]
    assert len(set(rest)) == len(rest)


def test_operands_are_in_range_and_depend_on_coordinates():
    for u in ct.MATRIX_UNITS:
        m, n, k = ct.SHAPES[u]
        a, b = ct.operands(u, 3)
        assert a.shape == (ct.ROUNDS[u], m, k) and b.shape == (ct.ROUNDS[u], k, n)
        half = ct.SPANS[u] // 2
        for x in (a, b):
            assert x.min() == -half and x.max() == half - 1  # the whole range is used
        assert not (a[0] == a[1]).all() and not (a[:, 0] == a[:, 1]).all() and not (a[:, :, 0] == a[:, :, 1]).all()
    a, _ = ct.operands(ct.UNIT_IDS["MFMA_I8"], 0)
    assert (a.min(), a.max()) == (-128, 127)  # the full int8 range
    # element (r, i, k) written out with Python integers
    M = (1 << 64) - 1

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    u, seed, r, i, k = ct.UNIT_IDS["MFMA_F16"], 9, 7, 11, 29
    a, b = ct.operands(u, seed)
    key = (seed + 1) * 0x9E3779B97F4A7C15 & M
    assert a[r, i, k] == ((mix((key + (u << 32 | r << 24 | 0 << 16 | i << 8 | k)) & M) >> 32) & 15) - 8
    assert b[r, k, i] == ((mix((key + (u << 32 | r << 24 | 1 << 16 | i << 8 | k)) & M) >> 32) & 15) - 8


def test_flipping_one_bit_or_swapping_two_elements_changes_the_signature():
    for u in ct.MATRIX_UNITS:
        bits = ct.result_bits(u, ct.product(u, 1))
        base = ct.signature(bits)
        assert base == ct.expected_signature(u, 1)
        for (i, j), bit in (((0, 0), 0), ((3, 5), 31), ((bits.shape[0] - 1, bits.shape[1] - 1), 13)):
            flipped = bits.copy()
            flipped[i, j] ^= np.uint32(1 << bit)
            assert ct.signature(flipped) != base
        flat = bits.reshape(-1)
        p, q = 0, next(x for x in range(1, flat.size) if flat[x] != flat[0])
        swapped = flat.copy()
        swapped[p], swapped[q] = flat[q], flat[p]
        assert ct.signature(swapped.reshape(bits.shape)) != base
        assert ct.signature(bits.T.copy()) != base  # transposed: every row and column exchanged


def test_every_result_is_exact_whatever_the_summation_order():
    for u in ct.MATRIX_UNITS:
        m, n, k = ct.SHAPES[u]
        half = ct.SPANS[u] // 2
        # the bound by construction: rounds * K * (span / 2)^2 ...
        assert ct.ROUNDS[u] * k * half * half < ct.exact_limit(u), ct.UNITS[u]
        # ... and of the operands the twin really generates, over the seeds a quick run uses
        for seed in range(ct.SEEDS["quick"]):
            assert ct.abs_bound(u, seed) < ct.exact_limit(u)
        d = ct.product(u, 0)
        if ct.exact_limit(u) == 1 << 24:
            assert (d.astype(np.float32).astype(np.int64) == d).all()


def test_valu_int_and_lds_twins():
    x, y = ct.valu_int_lanes(4)
    assert x.shape == y.shape == (64,) and len(set(y.tolist())) == 64 and int(x.max()) < 1 << 32
    x2, y2 = ct.valu_int_lanes(5)
    assert (y2 != y).all()
    w0, w1 = ct.lds_words(2, 0), ct.lds_words(2, 1)
    assert w0.size == ct.LDS_QUARTER_DWORDS == 10240 and (w1 == ~w0).all()
    assert 4 * 4 * ct.LDS_QUARTER_DWORDS == ct.LDS_BYTES == 160 << 10


# ------------------------------------------------------------------ the library's host code (no GPU is opened)

@pytest.fixture(scope="module")
def hip():
    from gpushare_scheduler_extender_amd.ops import hip as h

    h.lib()
    return h


def test_native_table_is_the_python_table(hip):
    table = hip.cutest_unit_table()
    assert tuple(t[0] for t in table) == ct.UNITS
    for u in ct.MATRIX_UNITS:
        assert table[u][1:] == (*ct.SHAPES[u], ct.ROUNDS[u], ct.SPANS[u])
    assert all(len(table[u]) == 1 for u in (ct.VALU_INT, ct.LDS))
    assert {lv: hip.cutest_seeds(lv) for lv in ("quick", "full")} == ct.SEEDS


def test_native_expected_equals_the_twin_over_the_seeds_of_full(hip):
    for seed in range(ct.SEEDS["full"]):
        for u in range(NUNITS):
            assert hip.cutest_expected(u, seed) == ct.expected_signature(u, seed), (ct.UNITS[u], seed)
    with pytest.raises(hip.HipError):
        hip.cutest_expected(NUNITS, 0)


def _rec(hip, xcc, se, sh, cu, simd, fail=0, seed=0, sig=None):
    r = hip.CutestRecord()
    r.hw_id = simd << 4 | cu << 8 | sh << 12 | se << 13 | 3  # a wave slot in the low bits, as the hardware has
    r.xcc_id = xcc
    r.fail_mask = fail
    r.seed = seed
    for u in range(NUNITS):
        r.sig[u] = ct.expected_signature(u, seed) if sig is None else sig[u]
    return r


def test_aggregate_attributes_by_physical_cu_and_simd(hip):
    want = [ct.expected_signature(u, 7) for u in range(NUNITS)]
    got = list(want)
    got[4] ^= 0x10
    got[8] ^= 0x1
    recs = [_rec(hip, 0, 1, 0, 2, s, seed=7) for s in range(4)]  # one CU, all four SIMDs
    recs += [_rec(hip, 1, 1, 0, 2, 0, seed=7), _rec(hip, 1, 1, 0, 2, 0, seed=7)]  # same se/sh/cu, another XCC
    recs += [_rec(hip, 7, 3, 1, 9, 1, seed=7), _rec(hip, 7, 3, 1, 9, 2, fail=1 << 4 | 1 << 8, seed=7, sig=got),
             _rec(hip, 7, 3, 1, 9, 2, fail=1 << 8, seed=7, sig=got)]
    rep = hip.cutest_aggregate(recs)
    assert (rep.waves, rep.bad_waves, rep.cus_seen, rep.simds_seen, rep.cus_covered) == (9, 2, 3, 7, 1)
    assert (rep.bad_cus, rep.n_bad) == (1, 1)
    cus = rep.cus()
    assert set(cus) == {(0, 1, 0, 2), (1, 1, 0, 2), (7, 3, 1, 9)}
    assert (cus[0, 1, 0, 2].waves, cus[0, 1, 0, 2].simds, cus[0, 1, 0, 2].fail_mask) == (4, 0xF, 0)
    assert (cus[1, 1, 0, 2].waves, cus[1, 1, 0, 2].simds) == (2, 0x1)
    c = cus[7, 3, 1, 9]
    assert (c.waves, c.bad_waves, c.simds, c.bad_simds, c.fail_mask) == (3, 2, 0x6, 0x4, 1 << 4 | 1 << 8)
    (b,) = rep.bad_entries()
    assert (b.xcc, b.se, b.sh, b.cu, b.simds, b.units, b.unit, b.seed) == (7, 3, 1, 9, 0x4, 1 << 4 | 1 << 8, 4, 7)
    assert b.expected == want[4] and b.got == got[4]
    # reports accumulate: the same CU bad again, on another SIMD, stays one entry
    hip.cutest_aggregate([_rec(hip, 7, 3, 1, 9, 0, fail=1, seed=7, sig=got)], rep)
    assert (rep.waves, rep.bad_waves, rep.bad_cus, rep.n_bad, rep.simds_seen) == (10, 3, 1, 1, 8)
    assert rep.bad_entries()[0].simds == 0x5 and rep.bad_entries()[0].units == 1 | 1 << 4 | 1 << 8
    assert rep.bad_entries()[0].unit == 4  # the first bad unit of the first bad wave
    # the decode and the slot, exhaustively: every (xcc, se, sh, cu) there is a slot for, on every SIMD
    where = [(x, se, sh, cu, simd) for x in range(16) for se in range(8) for sh in range(2) for cu in range(16)
             for simd in range(4)]
    arr = (hip.CutestRecord * len(where))()
    for r, (x, se, sh, cu, simd) in zip(arr, where):
        r.hw_id, r.xcc_id, r.seed = simd << 4 | cu << 8 | sh << 12 | se << 13 | 0xB, x, 7  # wave bits set
        assert (*r.where(), r.simd) == (x, se, sh, cu, simd)
    for fail in (0, 1 << 4):
        for r in arr:
            r.fail_mask = fail
        rep = hip.cutest_aggregate(arr)
        cus = rep.cus()
        assert len(cus) == ct.CU_SLOTS == 4096 and set(cus) == {w[:4] for w in where}
        assert all(c.simds == 0xF and c.waves == 4 for c in cus.values())
        assert (rep.waves, rep.cus_seen, rep.simds_seen, rep.cus_covered) == (16384, 4096, 16384, 4096)
        assert all(hip.slot_cu(hip.cu_slot(*w)) == w and rep.cu[hip.cu_slot(*w)].waves == 4 for w in cus)
        if fail:
            assert (rep.bad_cus, rep.n_bad, rep.bad_waves) == (4096, 16, 16384)
            assert [(b.xcc, b.se, b.sh, b.cu) for b in rep.bad_entries()] == [w[:4] for w in where[:64:4]]
            assert all(c.bad_simds == 0xF and c.fail_mask == fail for c in cus.values())
        else:
            assert (rep.bad_cus, rep.n_bad, rep.bad_waves) == (0, 0, 0)


def test_aggregate_caps_the_entries_and_keeps_the_counts(hip):
    recs = [_rec(hip, x, s, 0, c, 0, fail=2) for x in range(2) for s in range(4) for c in range(5)]  # 40 bad CUs
    recs += [_rec(hip, 3, 0, 0, c, 1) for c in range(6)]
    rep = hip.cutest_aggregate(recs)
    assert (rep.bad_cus, rep.n_bad, rep.bad_waves, rep.waves, rep.cus_seen) == (40, ct.MAX_BAD, 40, 46, 46)
    assert [(b.xcc, b.se, b.cu) for b in rep.bad_entries()] == [(0, s, c) for s in range(4) for c in range(5)][:16]
    assert sum(1 for c in rep.cus().values() if c.fail_mask) == 40
    empty = hip.cutest_aggregate([])
    assert (empty.waves, empty.bad_waves, empty.cus_seen, empty.bad_cus, empty.n_bad) == (0, 0, 0, 0, 0)
    assert empty.cus() == {}


def test_launch_rejects_bad_arguments_before_any_device_call(hip):
    recs = (hip.CutestRecord * 4)()
    L = hip.lib()
    assert L.gsx_cutest_launch(None, 0, 0, None, recs, 4) != 0 and b"block count" in L.gsx_last_error()
    assert L.gsx_cutest_launch(None, 0, 2, None, recs, 4) != 0 and b"4 * blocks" in L.gsx_last_error()
    bad = hip.CutestInject(0, 0, 0, 0, -1, NUNITS, 1)
    assert L.gsx_cutest_launch(None, 0, 1, bad, recs, 4) != 0 and b"unit" in L.gsx_last_error()


# ------------------------------------------------------------------ the tool's argument handling

def test_tool_rejects_bad_arguments_before_any_device_call():
    from gpushare_scheduler_extender_amd.utils.build import build_native

    build_native(["tools"])
    tool = ROOT / "gpushare_scheduler_extender_amd" / "_native" / "gsx-cutest"
    # no device may be opened: with every GPU hidden a device call would fail with another message
    env = {**os.environ, "HIP_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": ""}
    # the whole line, as the tool printed it before its frame was shared with gsx-memtest (seconds is 0 on these paths)
    line = ('{{"device":-1,"bdf":"","level":"{level}","launches":0,"seconds":0.000000,"cus_seen":0,"simds_seen":0,'
            '"cus_covered":0,"cus_expected":0,"covered":false,"waves":0,"bad_waves":0,"bad_cu_count":0,"bad_cus":[],'
            '"units_failed":[],"truncated":false,"error":"{error}"}}\n')
    words = "--cu-mask needs 32-bit words W0,W1,..."
    inject = "--inject needs XCC:SE:SH:CU[:SIMD]:UNIT:XORMASK (a unit's name or number, a non-zero 32-bit mask)"
    for argv, word, error in ((["--level", "bogus"], "--level", "--level needs quick or full"),
                              (["--cu-mask", "0,0"], "--cu-mask", "--cu-mask needs at least one CU"),
                              (["--cu-mask", "0x1ffffffff"], "--cu-mask", words),
                              (["--expect-cus", "0"], "--expect-cus", "--expect-cus needs a CU count"),
                              (["--max-seconds", "-1"], "--max-seconds", "--max-seconds needs a number of seconds"),
                              (["--inject", "0:0:0:0:LDS"], "--inject", inject),
                              (["--inject", "0:0:0:0:NOSUCH:1"], "--inject", inject),
                              (["--inject", "0:0:0:0:4:LDS:1"], "--inject", inject),
                              (["--inject", "0:0:0:0:LDS:0"], "--inject", inject),
                              (["--inject", "0:9:0:0:LDS:1"], "--inject", inject),
                              (["--device", "0", "--bdf", "0000:05:00.0"], "exclude",
                               "--device and --bdf exclude each other"),
                              (["--frobnicate"], "unknown", "unknown argument (see the head of tool_cutest.hip)")):
        r = subprocess.run([str(tool), *argv], capture_output=True, text=True, timeout=60, env=env)
        assert r.returncode == 2, (argv, r.returncode, r.stdout, r.stderr)
        assert r.stdout == line.format(level="quick", error=error), (argv, r.stdout)
        out = json.loads(r.stdout.strip().splitlines()[-1])
        assert word in out["error"] and out["device"] == -1 and out["waves"] == 0, (argv, out)
        assert set(out) >= {"device", "bdf", "level", "launches", "seconds", "cus_seen", "cus_expected", "covered",
                            "waves", "bad_waves", "bad_cus", "units_failed", "truncated", "error"}
        assert out["bad_cus"] == [] and out["units_failed"] == []
    # good arguments get as far as the device, and there is none
    r = subprocess.run([str(tool), "--inject", "1:2:0:3:2:MFMA_FP8:0x80", "--cu-mask", "0xffffffff,0xffffffff"],
                       capture_output=True, text=True, timeout=60, env=env)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 2 and out["error"] == "no HIP device" and out["device"] == -1
    assert r.stdout == line.format(level="quick", error="no HIP device")
    r = subprocess.run([str(tool), "--bdf", "0000:05:00.0", "--level", "full", "--expect-cus", "256",
                        "--max-seconds", "2.5"], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 2 and r.stdout == line.format(level="full", error="no HIP device")


# ------------------------------------------------------------------ the plugin's compute pre-flight

STUB = r'''#!{python}
"""Stand-in for gsx-cutest: per --bdf, what <dir>/<bdf>.cutest.json says ({{"rc", "sleep", "report"}}); logs every
start and end."""
import json, os, sys, time
here = os.path.dirname(os.path.abspath(__file__))
bdf = sys.argv[sys.argv.index("--bdf") + 1]
def note(what):
    with open(os.path.join(here, "events.log"), "a") as f:
        f.write(json.dumps({{"tool": "cutest", "what": what, "bdf": bdf, "t": time.monotonic()}}) + "\n")
with open(os.path.join(here, "cutest-starts.log"), "a") as f:
    f.write(json.dumps({{"pid": os.getpid(), "argv": sys.argv[1:]}}) + "\n")
note("start")
try:
    with open(os.path.join(here, bdf + ".cutest.json")) as f:
        plan = json.load(f)
except OSError:
    plan = {{}}
if plan.get("sleep"):
    time.sleep(plan["sleep"])
rep = {{"device": 0, "bdf": bdf, "level": "quick", "launches": 8, "seconds": 0.125, "cus_seen": 256,
       "simds_seen": 1024, "cus_covered": 256, "cus_expected": 256, "covered": True, "waves": 32768, "bad_waves": 0,
       "bad_cu_count": 0, "bad_cus": [], "units_failed": [], "truncated": False, "error": None}}
rep.update(plan.get("report") or {{}})
note("end")
print(json.dumps(rep))
sys.exit(plan.get("rc", 0))
'''

BAD = {"rc": 1, "report": {"bad_waves": 12, "bad_cu_count": 2, "units_failed": ["MFMA_FP8", "LDS"], "bad_cus": [
    {"xcc": 5, "se": 2, "sh": 1, "cu": 7, "simds": [1], "units": ["MFMA_FP8", "LDS"], "unit": "MFMA_FP8", "seed": 0,
     "expected": 1, "got": 3},
    {"xcc": 6, "se": 0, "sh": 0, "cu": 1, "simds": [0, 1, 2, 3], "units": ["LDS"], "unit": "LDS", "seed": 0,
     "expected": 1, "got": 2}]}}
REASON = "cutest: 2 bad CUs (first xcc 5 se 2 sh 1 cu 7, units MFMA_FP8,LDS)"


class Stub:
    def __init__(self, d: Path):
        self.dir = d
        self.path = d / "cutest-stub"
        self.path.write_text(STUB.format(python=sys.executable))
        self.path.chmod(self.path.stat().st_mode | stat.S_IXUSR)

    def plan(self, bdf: str, **plan):
        (self.dir / f"{bdf}.cutest.json").write_text(json.dumps(plan))

    def starts(self) -> list[dict]:
        try:
            return [json.loads(ln) for ln in (self.dir / "cutest-starts.log").read_text().splitlines()]
        except FileNotFoundError:
            return []


class Node(MemNode):
    async def post(self, query: str, what: str = "cutest"):
        import aiohttp

        async with aiohttp.ClientSession() as s:
            async with s.post(f"http://127.0.0.1:{self.port}/debug/{what}?{query}") as r:
                return r.status, await r.text()


def test_compute_preflight_is_off_by_default_and_independent_of_the_memory_one(sock_dir, tmp_path):
    stub, mem = Stub(tmp_path), MemStub(tmp_path)

    async def go():
        async with Node(sock_dir, preflight="quick", memtest_cmd=[str(mem.path)], cutest_cmd=[str(stub.path)]) as n:
            first = await n.start()
            assert n.plugin.preflight_compute.level == "off"
            assert all(d.health == "Healthy" for d in first.devices)
            await _health_polls(n.plugin, 2)
            assert stub.starts() == []  # --preflight quick alone starts no cutest child ...
            assert sorted(s["argv"][1] for s in mem.starts()) == sorted(d.bdf for d in n.devs)  # ... one memtest each
            assert [d["cutest"] for d in n.plugin.debug_state()["devices"]] == [None, None]
            assert "gpushare_plugin_cutest_errors_total 0" in n.plugin.metrics_text()
    asyncio.run(go())


def test_compute_preflight_all_clean(sock_dir, tmp_path):
    stub, mem = Stub(tmp_path), MemStub(tmp_path)

    async def go():
        async with Node(sock_dir, preflight_compute="quick", memtest_cmd=[str(mem.path)],
                        cutest_cmd=[str(stub.path)]) as n:
            first = await n.start()
            assert len(first.devices) == 128 and all(d.health == "Healthy" for d in first.devices)
            assert mem.starts() == []  # the memory pre-flight stays off
            starts = stub.starts()
            assert sorted(s["argv"][1] for s in starts) == sorted(d.bdf for d in n.devs)  # one child per device
            argv = starts[0]["argv"]
            assert argv[2:4] == ["--level", "quick"] and "--max-seconds" in argv
            cu = {d.bdf: d.cu_count for d in n.devs}[argv[1]]
            assert cu > 0 and argv[argv.index("--expect-cus") + 1] == str(cu)
            m = n.plugin.metrics_text()
            for dev in (0, 1):
                assert f'gpushare_plugin_cutest_bad_cus{{device="{dev}"}} 0' in m
                assert f'gpushare_plugin_cutest_bad_waves{{device="{dev}"}} 0' in m
                assert f'gpushare_plugin_cutest_cus_seen{{device="{dev}"}} 256' in m
                assert f'gpushare_plugin_cutest_seconds{{device="{dev}"}} 0.125' in m
                assert f'gpushare_plugin_cutest_last_run_timestamp{{device="{dev}"}} ' in m
            assert "gpushare_plugin_cutest_errors_total 0" in m
            state = n.plugin.debug_state()
            assert [d["cutest"]["bad_cu_count"] for d in state["devices"]] == [0, 0]
            assert [d["memtest"] for d in state["devices"]] == [None, None]
    asyncio.run(go())


def test_compute_failure_is_unhealthy_at_once_sticky_and_cleared_by_a_clean_run(sock_dir, tmp_path):
    stub = Stub(tmp_path)

    async def go():
        async with Node(sock_dir, preflight_compute="quick", cutest_cmd=[str(stub.path)]) as n:
            stub.plan(n.devs[1].bdf, **BAD)
            first = await n.start()
            tag1 = device_tags(n.devs)[1]
            assert n.unhealthy(first) == {tag1}  # in the FIRST list kubelet sees
            rep = n.plugin.debug_state()["devices"][1]["cutest"]
            assert rep["reason"] == REASON
            m = n.plugin.metrics_text()
            assert 'gpushare_plugin_cutest_bad_cus{device="1"} 2' in m
            assert 'gpushare_plugin_cutest_bad_waves{device="1"} 12' in m
            # fake amdsmi says healthy at every poll; the failed mark holds
            await _health_polls(n.plugin, 6)
            assert n.plugin.health_info[1]["healthy"] and not n.plugin.devices[1].healthy
            assert n.plugin.devices[0].healthy
            assert 'gpushare_plugin_device_healthy{device="1"} 0' in n.plugin.metrics_text()
            # on demand, with a tool that now finds nothing
            stub.plan(n.devs[1].bdf, rc=0)
            status, body = await n.post("device=1&level=full")
            assert status == 200 and json.loads(body)["bad_cu_count"] == 0, (status, body)
            assert stub.starts()[-1]["argv"][2:4] == ["--level", "full"]
            upd = await n.next_list()
            assert n.unhealthy(upd) == set()
            assert n.plugin.devices[1].healthy
            assert (await n.post("device=7"))[0] == 404 and (await n.post("device=1&level=bogus"))[0] == 400
    asyncio.run(go())


def test_compute_preflight_skips_a_device_with_an_allocation_record(sock_dir, tmp_path):
    stub = Stub(tmp_path)

    async def go():
        async with Node(sock_dir, preflight_compute="quick", cutest_cmd=[str(stub.path)]) as n:
            ann = {P.annotation_idx: "0", P.annotation_pod: "8", P.annotation_dev: "64",
                   P.annotation_assigned: "true", P.annotation_assume_time: "1"}
            await n.c.create("pods", make_pod("tenant", 8, node="n", annotations=ann, phase="Running", uid="u-tenant"))
            ids = [f"{device_tags(n.devs)[0]}-_-{k}" for k in range(8)]
            ckpt = sock_dir / "dp" / "gsx-allocations.json"
            ckpt.parent.mkdir(parents=True, exist_ok=True)
            ckpt.write_text(json.dumps({"node": "n", "records": [
                {"aid": "a1", "ids": ids, "uid": "u-tenant", "dev": 0, "units": 8, "cu_mask": "", "owner": "u-tenant",
                 "on_gpu": True}]}))
            stub.plan(n.devs[0].bdf, **BAD)  # would fail -- if it were tested
            first = await n.start()
            assert n.unhealthy(first) == set()
            assert [s["argv"][1] for s in stub.starts()] == [n.devs[1].bdf]  # GPU 0 was never tested
            assert n.plugin.debug_state()["devices"][0]["cutest"]["skipped"] == "in use"
            status, _ = await n.post("device=0")
            assert status == 409 and len(stub.starts()) == 1
            stub.plan(n.devs[0].bdf, rc=0)
            status, body = await n.post("device=0&force=1")
            assert status == 200 and json.loads(body)["bad_cu_count"] == 0
            assert stub.starts()[-1]["argv"][1] == n.devs[0].bdf and n.plugin.devices[0].healthy
    asyncio.run(go())


@pytest.mark.parametrize("how", ["exit2", "timeout", "missing"])
def test_compute_preflight_that_cannot_run_leaves_the_gpu_healthy(sock_dir, tmp_path, how):
    stub = Stub(tmp_path)
    cmd = [str(tmp_path / "no-such-tool")] if how == "missing" else [str(stub.path)]

    async def go():
        async with Node(sock_dir, preflight_compute="quick", preflight_timeout=0.5 if how == "timeout" else 30,
                        cutest_cmd=cmd) as n:
            if how == "exit2":  # coverage stayed short of --expect-cus: reported, never a compute error
                stub.plan(n.devs[1].bdf, rc=2, report={"error": "coverage stayed short of --expect-cus",
                                                       "covered": False, "cus_covered": 250})
            elif how == "timeout":
                stub.plan(n.devs[1].bdf, sleep=60)
            t0 = time.monotonic()
            first = await n.start()
            assert time.monotonic() - t0 < 20
            assert len(first.devices) == 128 and n.unhealthy(first) == set()
            m = n.plugin.metrics_text()
            want = 2 if how == "missing" else 1  # no device can be tested without the tool
            assert f"gpushare_plugin_cutest_errors_total {want}" in m
            assert "gpushare_plugin_memtest_errors_total 0" in m
            assert 'gpushare_plugin_cutest_bad_cus{device="1"}' not in m
            rep = n.plugin.debug_state()["devices"][1]["cutest"]
            assert rep["error"] and n.plugin.devices[1].healthy
            if how == "exit2":
                assert rep["error"].startswith("coverage stayed short") and rep["exit"] == 2 and not rep["covered"]
            if how == "timeout":
                assert "timed out" in rep["error"]
                (pid,) = [s["pid"] for s in stub.starts() if s["argv"][1] == n.devs[1].bdf]
                assert not _alive(pid)  # terminated, not left sleeping
            if how == "missing":
                assert "cannot start" in rep["error"]
            await _health_polls(n.plugin, 2)
            assert n.plugin.devices[1].healthy
    asyncio.run(go())


MEM_STUB_LOGGING = r'''#!{python}
"""gsx-memtest stand-in that also logs its start and end to events.log and stays a little while."""
import json, os, sys, time
here = os.path.dirname(os.path.abspath(__file__))
bdf = sys.argv[sys.argv.index("--bdf") + 1]
def note(what):
    with open(os.path.join(here, "events.log"), "a") as f:
        f.write(json.dumps({{"tool": "memtest", "what": what, "bdf": bdf, "t": time.monotonic()}}) + "\n")
note("start")
try:
    with open(os.path.join(here, bdf + ".json")) as f:
        plan = json.load(f)
except OSError:
    plan = {{}}
time.sleep(0.2)
rep = {{"device": 0, "bdf": bdf, "level": "quick", "bytes_tested": 1 << 30, "bytes_moved": 8 << 30, "passes": 6,
       "seconds": 0.25, "gbps": 34.4, "bad_dwords": 0, "flipped_or": 0, "errors": [], "truncated": False,
       "error": None}}
rep.update(plan.get("report") or {{}})
note("end")
print(json.dumps(rep))
sys.exit(plan.get("rc", 0))
'''


def test_memory_and_compute_failures_each_need_their_own_clean_run(sock_dir, tmp_path):
    stub = Stub(tmp_path)
    mem = tmp_path / "memtest-logging-stub"
    mem.write_text(MEM_STUB_LOGGING.format(python=sys.executable))
    mem.chmod(mem.stat().st_mode | stat.S_IXUSR)

    async def go():
        async with Node(sock_dir, preflight="quick", preflight_compute="quick", memtest_cmd=[str(mem)],
                        cutest_cmd=[str(stub.path)]) as n:
            bdf1 = n.devs[1].bdf
            stub.plan(bdf1, sleep=0.2, **BAD)
            stub.plan(n.devs[0].bdf, sleep=0.2)
            (tmp_path / f"{bdf1}.json").write_text(json.dumps(MEM_BAD))
            first = await n.start()
            tag1 = device_tags(n.devs)[1]
            assert n.unhealthy(first) == {tag1}
            # both tools ran on both GPUs, and a GPU's two children took turns
            events = [json.loads(ln) for ln in (tmp_path / "events.log").read_text().splitlines()]
            for d in n.devs:
                mine = sorted((e for e in events if e["bdf"] == d.bdf), key=lambda e: e["t"])
                assert sorted(e["tool"] for e in mine if e["what"] == "start") == ["cutest", "memtest"]
                assert [e["what"] for e in mine] == ["start", "end", "start", "end"], mine
                assert mine[0]["tool"] == mine[1]["tool"] and mine[2]["tool"] == mine[3]["tool"]
            state = n.plugin.debug_state()["devices"][1]
            assert state["memtest"]["bad_dwords"] == 3 and state["cutest"]["reason"] == REASON
            # a clean compute run alone does not lift the memory test's mark ...
            stub.plan(bdf1, rc=0)
            status, _ = await n.post("device=1")
            assert status == 200 and not n.plugin.devices[1].healthy
            await _health_polls(n.plugin, 2)
            assert not n.plugin.devices[1].healthy
            # ... nor does a clean memory run lift a compute mark: fail compute again, then clean the memory
            stub.plan(bdf1, **BAD)
            assert (await n.post("device=1"))[0] == 200
            (tmp_path / f"{bdf1}.json").write_text(json.dumps({"rc": 0}))
            status, _ = await n.post("device=1", what="memtest")
            assert status == 200 and not n.plugin.devices[1].healthy
            await _health_polls(n.plugin, 2)
            assert not n.plugin.devices[1].healthy
            # both clean: Healthy again
            stub.plan(bdf1, rc=0)
            assert (await n.post("device=1"))[0] == 200
            assert n.plugin.devices[1].healthy and n.plugin.devices[0].healthy
    asyncio.run(go())


def test_entry_point_has_the_compute_preflight_flag():
    r = subprocess.run([sys.executable, "-m", "gpushare_scheduler_extender_amd.deviceplugin", "--help"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120, env={**os.environ, "PYTHONPATH": str(ROOT)})
    assert r.returncode == 0
    assert "--preflight-compute {off,quick,full}" in r.stdout and "--preflight {off,quick,full}" in r.stdout
    bad = subprocess.run([sys.executable, "-m", "gpushare_scheduler_extender_amd.deviceplugin", "--node", "n",
                          "--preflight-compute", "sometimes"], cwd=ROOT, capture_output=True, text=True, timeout=120,
                         env={**os.environ, "PYTHONPATH": str(ROOT)})
    assert bad.returncode == 2 and "--preflight-compute" in bad.stderr
