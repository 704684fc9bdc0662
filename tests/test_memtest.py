"""The HBM pre-flight memory test without a GPU: the NumPy twin of the kernels' pattern generator, the pass table,
``gsx-memtest``'s argument handling, and the device plugin's pre-flight driven through a stub tool against the fake
amdsmi backend -- failures are sticky across health polls, a tool that cannot run never costs capacity, GPUs with
tenants are left alone."""
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

from gpushare_scheduler_extender_amd.deviceplugin.devices import Device, apply_memory_pools
from gpushare_scheduler_extender_amd.deviceplugin.plugin import GpuSharePlugin, device_tags
from gpushare_scheduler_extender_amd.k8s.client import KubeClient
from gpushare_scheduler_extender_amd.k8s.objects import make_node, make_pod
from gpushare_scheduler_extender_amd.models.profile import SHARED_GPU
from gpushare_scheduler_extender_amd.ops import memtest as mt
from gpushare_scheduler_extender_amd.ops import mxdev
from gsxtools.kubeletapi import PluginClient
from tests.fixtures.fakeapi import FakeApiServerRunner

ROOT = Path(__file__).resolve().parents[1]
P = SHARED_GPU
BACKEND = "fake:2x64GiB"


# ------------------------------------------------------------------ the NumPy twin

@pytest.mark.parametrize("pattern", sorted(mt.PATTERNS.values()))
def test_twin_is_deterministic_and_invert_is_the_complement(pattern):
    a = mt.memtest_words(pattern, 0x1234, 0, 4096, 1 << 16)
    b = mt.memtest_words(pattern, 0x1234, 0, 4096, 1 << 16)
    assert a.dtype == np.uint32 and a.shape == ((1 << 16) // 4,) and (a == b).all()
    inv = mt.memtest_words(pattern, 0x1234, 1, 4096, 1 << 16)
    assert (inv == ~a).all()
    # a range generated in two pieces, the second with its origin advanced, is the range generated at once
    two = np.concatenate([mt.memtest_words(pattern, 0x1234, 0, 4096, 1 << 15),
                          mt.memtest_words(pattern, 0x1234, 0, 4096 + (1 << 15), 1 << 15)])
    assert (two == a).all()


def test_twin_known_words():
    # ADDR: {lo32(W), hi32(W), ~lo32(W), ~hi32(W)} of W = origin / 16 + k
    w = mt.memtest_words(mt.ADDR, 99, 0, 48, 32)
    assert w.tolist() == [3, 0, 0xFFFFFFFC, 0xFFFFFFFF, 4, 0, 0xFFFFFFFB, 0xFFFFFFFF]
    assert set(mt.memtest_words(mt.SOLID, 0x55555555, 0, 0, 64).tolist()) == {0x55555555}
    # WALK: dword j of word W is 1 << ((4 W + j + seed) & 31)
    w = mt.memtest_words(mt.WALK, 30, 0, 16, 32)
    assert w.tolist() == [1 << ((4 * W + j + 30) & 31) for W in (1, 2) for j in range(4)]
    # RANDOM: splitmix64's output function of 2 W + half + (seed + 1) * golden, written out with Python integers
    M = (1 << 64) - 1

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    want = []
    for W in (5, 6):
        for half in (0, 1):
            z = mix((2 * W + half + (7 + 1) * 0x9E3779B97F4A7C15) & M)
            want += [z & 0xFFFFFFFF, z >> 32]
    assert mt.memtest_words(mt.RANDOM, 7, 0, 80, 32).tolist() == want
    r = mt.memtest_words(mt.RANDOM, 0, 0, 0, 1 << 20)
    assert abs(float(np.unpackbits(r.view(np.uint8)).mean()) - 0.5) < 0.001  # half the bits set
    assert (mt.memtest_words(mt.RANDOM, 1, 0, 0, 4096) != r[:1024]).mean() > 0.99  # the seed matters


def test_twin_addr_words_are_unique_across_a_chunk_boundary():
    chunk = 1 << 16
    a = mt.memtest_words(mt.ADDR, 0, 0, 0, chunk).reshape(-1, 4)
    b = mt.memtest_words(mt.ADDR, 0, 0, chunk, chunk).reshape(-1, 4)  # the next chunk: its origin advanced
    both = np.concatenate([a, b])
    assert len({tuple(x) for x in both.tolist()}) == len(both)
    restart = mt.memtest_words(mt.ADDR, 0, 0, 0, chunk).reshape(-1, 4)  # what a chunk without origin would hold
    assert (restart == a).all() and not (b == a).all(axis=1).any()


def test_twin_walk_visits_all_32_bit_positions_within_8_consecutive_words():
    for seed in (0, 5, 31):
        for origin in (0, 48, 16 * 1001):
            w = mt.memtest_words(mt.WALK, seed, 0, origin, 8 * 16)
            assert sorted(w.tolist()) == [1 << k for k in range(32)]


def test_twin_word_index_wraps_correctly_at_2_pow_32():
    origin = 16 * ((1 << 32) - 2)  # words 2^32 - 2 .. 2^32 + 1
    w = mt.memtest_words(mt.ADDR, 0, 0, origin, 64).reshape(4, 4)
    assert w[:, 0].tolist() == [0xFFFFFFFE, 0xFFFFFFFF, 0, 1] and w[:, 1].tolist() == [0, 0, 1, 1]
    assert (w[:, 2] == ~w[:, 0]).all() and (w[:, 3] == ~w[:, 1]).all()
    r = mt.memtest_words(mt.RANDOM, 0, 0, origin, 64).reshape(4, 4)
    assert len({tuple(x) for x in r.tolist()}) == 4  # no repeat where lo32(W) starts over
    low = mt.memtest_words(mt.RANDOM, 0, 0, 0, 32).reshape(2, 4)
    assert not (r[2:] == low).all()  # W = 2^32 is not W = 0
    walk = mt.memtest_words(mt.WALK, 0, 0, origin, 64)
    assert walk.tolist() == [1 << ((4 * W + j) & 31) for W in range((1 << 32) - 2, (1 << 32) + 2) for j in range(4)]


def test_level_table_and_bytes_moved():
    quick, full = mt.LEVELS["quick"], mt.LEVELS["full"]
    assert [(op, p) for op, p, *_ in quick] == [("write", mt.ADDR), ("check", mt.ADDR), ("check", mt.ADDR),
                                                ("write", mt.RANDOM), ("check", mt.RANDOM), ("check", mt.RANDOM)]
    assert mt.bytes_moved("quick", 1000) == 8000  # write, check + rewrite (2 x), check: 4 x bytes per pattern
    assert full[:6] == quick and mt.level_passes("full") == 3 * (2 + 4 + 32)
    assert [s for op, p, s, *_ in full if p == mt.SOLID and op == "write"] == [0, 0xFFFFFFFF, 0x55555555, 0xAAAAAAAA]
    assert [s for op, p, s, *_ in full if p == mt.WALK and op == "write"] == list(range(32))
    for seq in (quick, full):
        for k in range(0, len(seq), 3):  # triples: write, check + rewrite, check the complement
            (o0, p0, s0, i0, r0), (o1, p1, s1, i1, r1), (o2, p2, s2, i2, r2) = seq[k:k + 3]
            assert (o0, i0, r0, o1, i1, r1, o2, i2, r2) == ("write", 0, 0, "check", 0, 1, "check", 1, 0)
            assert p0 == p1 == p2 and s0 == s1 == s2
    assert mt.bytes_moved("full", 16) == 4 * 16 * 38 and mt.bytes_moved("quick", 16, passes=2) == 48


def test_native_pass_table_is_the_python_table():
    """``gsx_memtest_run`` and ``gsx-memtest`` execute the sequence the Python table describes (the library loads
    without a GPU; no device call is made)."""
    from gpushare_scheduler_extender_amd.ops import hip

    for level in ("quick", "full"):
        assert hip.memtest_pass_table(level) == mt.LEVELS[level]


# ------------------------------------------------------------------ the tool's argument handling

def test_tool_rejects_bad_arguments_before_any_device_call():
    from gpushare_scheduler_extender_amd.utils.build import build_native

    build_native(["tools"])
    tool = ROOT / "gpushare_scheduler_extender_amd" / "_native" / "gsx-memtest"
    # no device may be opened: with every GPU hidden a device call would fail with another message
    env = {**os.environ, "HIP_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": ""}
    # the whole line, as the tool printed it before its frame was shared with gsx-cutest (seconds is 0 on these paths)
    line = ('{{"device":-1,"bdf":"","level":"{level}","bytes_tested":0,"bytes_moved":0,"passes":0,"chunks":0,'
            '"seconds":0.000000,"gbps":0.0,"bad_dwords":0,"flipped_or":0,"errors":[],"truncated":false,'
            '"error":"{error}"}}\n')
    for argv, word, level, error in (
            (["--level", "bogus"], "--level", "quick", "--level needs quick or full"),
            (["--chunk", "4096"], "--chunk", "quick", "--chunk needs a multiple of 16 of at least 1 GiB"),
            (["--bytes", "100"], "--bytes", "quick", "--bytes needs a positive multiple of 16, or all"),
            (["--inject", "4096"], "--inject", "quick",
             "--inject needs OFFSET:XORMASK (a dword offset, a non-zero 32-bit mask)"),
            (["--device", "0", "--bdf", "0000:05:00.0"], "exclude", "quick", "--device and --bdf exclude each other"),
            (["--frobnicate"], "unknown", "quick", "unknown argument (see the head of tool_memtest.hip)"),
            # good arguments get as far as the device, and there is none
            (["--bdf", "0000:05:00.0", "--bytes", "33554432", "--level", "full", "--max-seconds", "2.5"], "no HIP",
             "full", "no HIP device"),
            (["--device", "1", "--reserve", "0x40000000", "--chunk", "2147483648", "--inject", "4096:0x10"], "no HIP",
             "quick", "no HIP device")):
        r = subprocess.run([str(tool), *argv], capture_output=True, text=True, timeout=60, env=env)
        assert r.returncode == 2, (argv, r.returncode, r.stdout, r.stderr)
        assert r.stdout == line.format(level=level, error=error), (argv, r.stdout)
        out = json.loads(r.stdout.strip().splitlines()[-1])
        assert word in out["error"] and out["device"] == -1 and out["bytes_tested"] == 0, (argv, out)
        assert set(out) >= {"device", "bdf", "level", "bytes_tested", "bytes_moved", "passes", "seconds", "gbps",
                            "bad_dwords", "flipped_or", "errors", "truncated", "error"}


# ------------------------------------------------------------------ the plugin's pre-flight

STUB = r'''#!{python}
"""Stand-in for gsx-memtest: per --bdf, what <dir>/<bdf>.json says ({{"rc", "sleep", "report"}}); logs every start."""
import json, os, sys, time
here = os.path.dirname(os.path.abspath(__file__))
bdf = sys.argv[sys.argv.index("--bdf") + 1]
with open(os.path.join(here, "starts.log"), "a") as f:
    f.write(json.dumps({{"pid": os.getpid(), "argv": sys.argv[1:]}}) + "\n")
try:
    with open(os.path.join(here, bdf + ".json")) as f:
        plan = json.load(f)
except OSError:
    plan = {{}}
if plan.get("sleep"):
    time.sleep(plan["sleep"])
rep = {{"device": 0, "bdf": bdf, "level": "quick", "bytes_tested": 1 << 30, "bytes_moved": 8 << 30, "passes": 6,
       "seconds": 0.25, "gbps": 34.4, "bad_dwords": 0, "flipped_or": 0, "errors": [], "truncated": False,
       "error": None}}
rep.update(plan.get("report") or {{}})
print(json.dumps(rep))
sys.exit(plan.get("rc", 0))
'''

BAD = {"rc": 1, "report": {"bad_dwords": 3, "flipped_or": 0x104,
                           "errors": [{"offset": 0x1000, "expected": 0, "actual": 0x100}]}}


class Stub:
    def __init__(self, d: Path):
        self.dir = d
        self.path = d / "memtest-stub"
        self.path.write_text(STUB.format(python=sys.executable))
        self.path.chmod(self.path.stat().st_mode | stat.S_IXUSR)

    def plan(self, bdf: str, **plan):
        (self.dir / f"{bdf}.json").write_text(json.dumps(plan))

    def starts(self) -> list[dict]:
        try:
            return [json.loads(ln) for ln in (self.dir / "starts.log").read_text().splitlines()]
        except FileNotFoundError:
            return []


def _devices():
    return apply_memory_pools([Device(**d) for d in mxdev.enumerate_devices(BACKEND)])


class Node:
    """A fake apiserver, a plugin on node ``n`` with two fake 64 GiB GPUs, and a ListAndWatch stream."""

    def __init__(self, sock_dir, **plugin_kw):
        self.sock_dir, self.kw = sock_dir, plugin_kw

    async def __aenter__(self):
        mxdev._sessions.pop(BACKEND, None)  # a fake backend of our own: other tests inject faults into theirs
        self.api = await FakeApiServerRunner().start()
        self.c = KubeClient(self.api.url)
        await self.c.create("nodes", make_node("n", 128, 2))
        self.devs = _devices()
        return self

    async def start(self):
        self.plugin = GpuSharePlugin(KubeClient(self.api.url), "n", self.devs, SHARED_GPU,
                                     socket_dir=str(self.sock_dir / "dp"), health_backend=BACKEND,
                                     health_interval=0.05, **self.kw)
        self.port = await self.plugin.serve_debug("127.0.0.1", 0)
        await self.plugin.start(register=False)
        self.cl = PluginClient(self.plugin.socket_path)
        self.stream = self.cl.list_and_watch()
        return await self.next_list()

    async def next_list(self):
        return await asyncio.wait_for(self.stream.read(), 5)

    async def post(self, query: str):
        import aiohttp

        async with aiohttp.ClientSession() as s:
            async with s.post(f"http://127.0.0.1:{self.port}/debug/memtest?{query}") as r:
                return r.status, await r.text()

    def unhealthy(self, resp) -> set:
        return {d.ID.split("-_-")[0] for d in resp.devices if d.health == "Unhealthy"}

    async def __aexit__(self, *exc):
        if hasattr(self, "stream"):
            self.stream.cancel()
            await self.cl.close()
        if hasattr(self, "plugin"):
            await self.plugin.stop()
            await self.plugin.client.close()
        await self.c.close()
        await self.api.stop()
        mxdev._sessions.pop(BACKEND, None)


async def _health_polls(plugin, n: int):
    """Wait until the amdsmi health loop has polled ``n`` more times (it replaces ``health_info[0]`` every poll)."""
    for _ in range(n):
        seen = plugin.health_info.get(0)
        for _ in range(200):
            await asyncio.sleep(0.01)
            if plugin.health_info.get(0) is not seen:
                break
        else:
            raise AssertionError("the health loop does not poll")


def test_preflight_all_clean(sock_dir, tmp_path):
    stub = Stub(tmp_path)

    async def go():
        async with Node(sock_dir, preflight="quick", preflight_gib=1, memtest_cmd=[str(stub.path)]) as n:
            first = await n.start()
            assert len(first.devices) == 128 and all(d.health == "Healthy" for d in first.devices)
            starts = stub.starts()
            assert sorted(s["argv"][1] for s in starts) == sorted(d.bdf for d in n.devs)  # one child per GPU
            argv = starts[0]["argv"]
            assert argv[2:6] == ["--level", "quick", "--bytes", str(1 << 30)] and "--max-seconds" in argv
            m = n.plugin.metrics_text()
            for dev in (0, 1):
                assert f'gpushare_plugin_memtest_bad_dwords{{device="{dev}"}} 0' in m
                assert f'gpushare_plugin_memtest_bytes_tested{{device="{dev}"}} {1 << 30}' in m
                assert f'gpushare_plugin_memtest_seconds{{device="{dev}"}} 0.25' in m
                assert f'gpushare_plugin_memtest_last_run_timestamp{{device="{dev}"}} ' in m
            assert "gpushare_plugin_memtest_errors_total 0" in m
            state = n.plugin.debug_state()
            assert [d["memtest"]["bad_dwords"] for d in state["devices"]] == [0, 0]
    asyncio.run(go())


def test_preflight_failure_is_unhealthy_at_once_sticky_and_cleared_by_a_clean_run(sock_dir, tmp_path):
    stub = Stub(tmp_path)

    async def go():
        async with Node(sock_dir, preflight="quick", memtest_cmd=[str(stub.path)]) as n:
            stub.plan(n.devs[1].bdf, **BAD)
            first = await n.start()
            tag1 = device_tags(n.devs)[1]
            assert n.unhealthy(first) == {tag1}  # in the FIRST list kubelet sees
            assert stub.starts()[0]["argv"][5] == "all"
            rep = n.plugin.debug_state()["devices"][1]["memtest"]
            assert rep["reason"] == "memtest: 3 bad dwords, first at offset 0x1000, bits 0x104"
            assert 'gpushare_plugin_memtest_bad_dwords{device="1"} 3' in n.plugin.metrics_text()
            # fake amdsmi says healthy at every poll; the failed mark holds
            await _health_polls(n.plugin, 6)
            assert n.plugin.health_info[1]["healthy"] and not n.plugin.devices[1].healthy
            assert n.plugin.devices[0].healthy
            assert 'gpushare_plugin_device_healthy{device="1"} 0' in n.plugin.metrics_text()
            # so does a reset: the post-reset path obeys the same rule
            mxdev.inject(1, "event=GPU_POST_RESET", BACKEND)
            await _health_polls(n.plugin, 3)
            assert not n.plugin.devices[1].healthy
            # on demand, with a tool that now finds nothing
            stub.plan(n.devs[1].bdf, rc=0)
            status, body = await n.post("device=1")
            assert status == 200 and json.loads(body)["bad_dwords"] == 0, (status, body)
            upd = await n.next_list()
            assert n.unhealthy(upd) == set()
            assert n.plugin.devices[1].healthy
            assert (await n.post("device=7"))[0] == 404 and (await n.post("device=1&level=bogus"))[0] == 400
    asyncio.run(go())


def test_preflight_skips_a_gpu_with_an_allocation_record(sock_dir, tmp_path):
    stub = Stub(tmp_path)

    async def go():
        async with Node(sock_dir, preflight="quick", memtest_cmd=[str(stub.path)]) as n:
            ann = {P.annotation_idx: "0", P.annotation_pod: "8", P.annotation_dev: "64",
                   P.annotation_assigned: "true", P.annotation_assume_time: "1"}
            pod = make_pod("tenant", 8, node="n", annotations=ann, phase="Running", uid="u-tenant")
            await n.c.create("pods", pod)
            ids = [f"{device_tags(n.devs)[0]}-_-{k}" for k in range(8)]
            ckpt = sock_dir / "dp" / "gsx-allocations.json"
            ckpt.parent.mkdir(parents=True, exist_ok=True)
            ckpt.write_text(json.dumps({"node": "n", "records": [
                {"aid": "a1", "ids": ids, "uid": "u-tenant", "dev": 0, "units": 8, "cu_mask": "", "owner": "u-tenant",
                 "on_gpu": True}]}))
            stub.plan(n.devs[0].bdf, **BAD)  # would fail -- if it were tested
            first = await n.start()
            assert [r.dev for r in n.plugin.state.records.values()] == [0]
            assert n.unhealthy(first) == set()
            assert [s["argv"][1] for s in stub.starts()] == [n.devs[1].bdf]  # GPU 0 was never tested
            assert n.plugin.debug_state()["devices"][0]["memtest"]["skipped"] == "in use"
            status, _ = await n.post("device=0")
            assert status == 409 and len(stub.starts()) == 1
            # force=1: what is free now, minus a reserve
            stub.plan(n.devs[0].bdf, rc=0)
            status, body = await n.post("device=0&force=1")
            assert status == 200 and json.loads(body)["bad_dwords"] == 0
            forced = stub.starts()[-1]["argv"]
            assert forced[1] == n.devs[0].bdf and "--reserve" in forced and forced[forced.index("--bytes") + 1] == "all"
            assert n.plugin.devices[0].healthy
    asyncio.run(go())


def _alive(pid: int) -> bool:
    try:
        os.kill(pid, 0)
    except ProcessLookupError:
        return False
    try:  # a zombie is gone as far as the GPU is concerned, but the plugin reaps its children anyway
        return Path(f"/proc/{pid}/stat").read_text().split(")")[-1].split()[0] != "Z"
    except OSError:
        return False


@pytest.mark.parametrize("how", ["exit2", "timeout", "missing"])
def test_preflight_that_cannot_run_leaves_the_gpu_healthy(sock_dir, tmp_path, how):
    stub = Stub(tmp_path)
    cmd = [str(tmp_path / "no-such-tool")] if how == "missing" else [str(stub.path)]

    async def go():
        async with Node(sock_dir, preflight="quick", preflight_timeout=0.5 if how == "timeout" else 30,
                        memtest_cmd=cmd) as n:
            if how == "exit2":
                stub.plan(n.devs[1].bdf, rc=2, report={"error": "device allocation failed", "bytes_tested": 0})
            elif how == "timeout":
                stub.plan(n.devs[1].bdf, sleep=60)
            t0 = time.monotonic()
            first = await n.start()
            assert time.monotonic() - t0 < 20
            assert len(first.devices) == 128 and n.unhealthy(first) == set()
            m = n.plugin.metrics_text()
            want = 2 if how == "missing" else 1  # no GPU can be tested without the tool
            assert f"gpushare_plugin_memtest_errors_total {want}" in m
            assert 'gpushare_plugin_memtest_bad_dwords{device="1"}' not in m
            rep = n.plugin.debug_state()["devices"][1]["memtest"]
            assert rep["error"] and n.plugin.devices[1].healthy
            if how == "exit2":
                assert rep["error"] == "device allocation failed" and rep["exit"] == 2
            if how == "timeout":
                assert "timed out" in rep["error"]
                (pid,) = [s["pid"] for s in stub.starts() if s["argv"][1] == n.devs[1].bdf]
                assert not _alive(pid)  # terminated, not left sleeping
            if how == "missing":
                assert "cannot start" in rep["error"]
            await _health_polls(n.plugin, 2)
            assert n.plugin.devices[1].healthy
    asyncio.run(go())


def test_preflight_is_off_by_default(sock_dir, tmp_path):
    stub = Stub(tmp_path)

    async def go():
        async with Node(sock_dir, memtest_cmd=[str(stub.path)]) as n:
            first = await n.start()
            assert n.plugin.preflight.level == "off"
            assert all(d.health == "Healthy" for d in first.devices)
            await _health_polls(n.plugin, 2)
            assert stub.starts() == []  # never started
            assert n.plugin.debug_state()["devices"][0]["memtest"] is None
            assert "gpushare_plugin_memtest_errors_total 0" in n.plugin.metrics_text()
    asyncio.run(go())


def test_entry_point_has_the_preflight_flags():
    r = subprocess.run([sys.executable, "-m", "gpushare_scheduler_extender_amd.deviceplugin", "--help"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120, env={**os.environ, "PYTHONPATH": str(ROOT)})
    assert r.returncode == 0
    for flag in ("--preflight {off,quick,full}", "--preflight-gib", "--preflight-timeout"):
        assert flag in r.stdout
    bad = subprocess.run([sys.executable, "-m", "gpushare_scheduler_extender_amd.deviceplugin", "--node", "n",
                          "--preflight", "sometimes"], cwd=ROOT, capture_output=True, text=True, timeout=120,
                         env={**os.environ, "PYTHONPATH": str(ROOT)})
    assert bad.returncode == 2 and "--preflight" in bad.stderr
