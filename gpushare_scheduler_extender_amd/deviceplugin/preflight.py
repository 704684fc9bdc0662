"""Pre-flight: run ``gsx-memtest`` (HBM) and ``gsx-cutest`` (compute) on the GPUs nobody uses yet and keep what fails
out of ListAndWatch.

The plugin never opens HIP itself: every GPU is tested by a child process of its own (at most
:data:`MAX_CHILDREN` at a time), whose JSON line and exit code are the result:

* exit 0 -- clean: a failed mark from an earlier run is cleared;
* exit 1 -- memory errors: the GPU's IDs turn ``Unhealthy`` and stay so (the amdsmi health poll cannot flip them
  back) until a later run is clean;
* exit 2, a timeout (the child is terminated, then killed) or a missing tool -- the test could not run: the GPU stays
  as it was, the outcome is recorded and counted in ``gpushare_plugin_memtest_errors_total``.  A broken tool must
  not take a node's capacity away.

A GPU with an allocation record, or a pod of this node annotated onto it, is skipped (``"skipped": "in use"``): the
test never takes memory from a tenant.  Compute partitions of one GPU share its HBM, so one child tests the pool
and its result holds for every partition; the pool counts as in use when any of them is.

:class:`ComputePreflight` is the same child-runner for ``gsx-cutest`` (``--preflight-compute``): exit 1 means CUs that
computed wrong answers.  It runs per device, not per pool -- compute partitions of one GPU have CUs of their own --
with ``--expect-cus`` set to the device's CU count, shares the memory test's cap on children, and never runs while
the memory test of the same GPU does.  A device is healthy only if neither pre-flight holds it down.
"""
from __future__ import annotations

import asyncio
import json
import logging
import time
from pathlib import Path

log = logging.getLogger("gsx.preflight")

LEVELS = ("off", "quick", "full")
MAX_CHILDREN = 8
KILL_GRACE_S = 2.0  # between SIGTERM and SIGKILL of a child past its timeout
# what a forced on-demand run leaves free next to the tenants' memory, as the tool's own default does
FORCE_RESERVE = 1 << 30
TOOL = Path(__file__).resolve().parents[1] / "_native" / "gsx-memtest"
CUTEST_TOOL = TOOL.with_name("gsx-cutest")


class InUse(Exception):
    """The GPU has tenants: an on-demand test needs ``force``."""


class Preflight:
    NAME = "memtest"  # in log lines, reasons and metric names
    BAD = "bad_dwords"  # the report key that counts what exit 1 found
    METRICS = (("bad_dwords", "bad_dwords"), ("bytes_tested", "bytes_tested"), ("seconds", "seconds"),
               ("last_run_timestamp", "timestamp"))

    def __init__(self, plugin, level: str = "off", gib: float = 0.0, timeout: float = 120.0,
                 cmd: list[str] | None = None):
        if level not in LEVELS:
            raise ValueError(f"preflight level {level!r}: one of {', '.join(LEVELS)}")
        self.plugin = plugin
        self.level = level
        self.gib = gib
        self.timeout = timeout
        self.cmd = list(cmd) if cmd else [str(TOOL)]
        # by HBM pool (a physical GPU: the key outlives a re-partitioning, which renumbers the devices)
        self.failed: set[str] = set()  # pools whose last completed test found memory errors
        self.reports: dict[str, dict] = {}  # the last outcome per pool
        self.errors_total = 0  # tests that could not run
        self._sem: asyncio.Semaphore | None = None
        self._gpu_locks: dict[str, asyncio.Lock] = {}  # one child per physical GPU at a time, whichever tool

    def _slot(self) -> asyncio.Semaphore:
        """The cap on children, shared by every pre-flight of the plugin."""
        if self._sem is None:
            self._sem = asyncio.Semaphore(MAX_CHILDREN)
        return self._sem

    def _gpu_lock(self, idx: int) -> asyncio.Lock:
        return self._gpu_locks.setdefault(Preflight._key(self, idx), asyncio.Lock())

    # ------------------------------------------------------------ which GPUs
    def _key(self, idx: int) -> str:
        d = self.plugin.devices.get(idx)
        return f"#{idx}" if d is None else d.pool or d.bdf or f"#{idx}"

    def is_failed(self, idx: int) -> bool:
        return bool(self.failed) and self._key(idx) in self.failed

    def report(self, idx: int) -> dict | None:
        """The last outcome of the memory test that covered device ``idx``."""
        return self.reports.get(self._key(idx))

    def _pool(self, idx: int) -> list[int]:
        """The indices of the devices that share ``idx``'s HBM (itself included)."""
        d = self.plugin.devices[idx]
        if not d.pool:
            return [idx]
        return sorted(i for i, o in self.plugin.devices.items() if o.pool == d.pool)

    def _device_in_use(self, idx: int) -> bool:
        st = self.plugin.state
        return (any(r.dev == idx for r in st.records.values())
                or any(p.dev == idx and not p.complete for p in st.pods.values())
                or st.core.lingering(idx) > 0 or st.core.terminating_used(idx) > 0)

    def in_use(self, idx: int) -> bool:
        return any(self._device_in_use(i) for i in self._pool(idx))

    # ------------------------------------------------------------ one child
    def _argv(self, idx: int, level: str, force: bool) -> list[str]:
        d = self.plugin.devices[idx]
        argv = [*self.cmd, "--bdf", d.bdf] if d.bdf else [*self.cmd, "--device", str(idx)]
        argv += ["--level", level, "--bytes", str(int(self.gib * (1 << 30)) // 16 * 16) if self.gib > 0 else "all"]
        if force:
            argv += ["--reserve", str(FORCE_RESERVE)]
        # the tool ends itself between passes before the plugin has to kill it ("truncated", not a failure)
        return [*argv, "--max-seconds", f"{0.8 * self.timeout:.3f}"]

    async def _child(self, idx: int, level: str, force: bool) -> dict:
        """Run the tool on one GPU: its JSON line plus ``exit``, or ``{"error": ...}`` when it could not run."""
        argv = self._argv(idx, level, force)
        try:
            proc = await asyncio.create_subprocess_exec(*argv, stdin=asyncio.subprocess.DEVNULL,
                                                        stdout=asyncio.subprocess.PIPE,
                                                        stderr=asyncio.subprocess.DEVNULL)
        except OSError as e:
            return {"error": f"cannot start {argv[0]}: {e.strerror or e}"}
        try:
            out, _ = await asyncio.wait_for(proc.communicate(), self.timeout)
        except asyncio.TimeoutError:
            await self._reap(proc)
            return {"error": f"timed out after {self.timeout:g}s"}
        except asyncio.CancelledError:
            await asyncio.shield(self._reap(proc))
            raise
        rep: dict = {}
        for line in reversed(out.decode(errors="replace").splitlines()):
            try:
                got = json.loads(line)
            except ValueError:
                continue
            if isinstance(got, dict):
                rep = got
                break
        rep["exit"] = proc.returncode
        if proc.returncode not in (0, 1):
            rep["error"] = rep.get("error") or f"exit status {proc.returncode}"
        elif self.BAD not in rep:
            rep["error"] = "no report on stdout"
        elif proc.returncode == 1 and not rep[self.BAD]:
            rep["error"] = f"exit 1 without {self.BAD.replace('_', ' ')}"
        return rep

    @staticmethod
    async def _reap(proc) -> None:
        """Terminate, then kill: no child outlives its test."""
        for sig in (proc.terminate, proc.kill):
            try:
                sig()
            except ProcessLookupError:
                return
            try:
                await asyncio.wait_for(proc.wait(), KILL_GRACE_S)
                return
            except asyncio.TimeoutError:
                continue
        await proc.wait()

    # ------------------------------------------------------------ results
    @staticmethod
    def reason(rep: dict) -> str:
        first = (rep.get("errors") or [{}])[0]
        return (f"memtest: {rep.get('bad_dwords', 0)} bad dwords, first at offset {first.get('offset', 0):#x}, "
                f"bits {rep.get('flipped_or', 0):#x}")

    def _apply(self, idx: int, rep: dict) -> None:
        """Record a pool's outcome for each of its devices and set their health."""
        rep["timestamp"] = time.time()
        key = self._key(idx)
        self.reports[key] = rep
        if rep.get("error"):  # could not run: the GPU stays as it was
            self.errors_total += 1
            log.warning("%s of GPU %d could not run: %s", self.NAME, idx, rep["error"])
            return
        if rep.get(self.BAD):
            rep["reason"] = self.reason(rep)
            self.failed.add(key)
        else:
            self.failed.discard(key)
        for i in self._pool(idx):
            if rep.get(self.BAD):
                self.plugin.set_health(i, False, f"({rep['reason']})")
            elif (self.plugin.health_info.get(i) or {}).get("healthy", True):
                # unless amdsmi, or the other pre-flight, holds it down
                self.plugin.set_health(i, True, f"({self.NAME} clean)")

    async def _one(self, idx: int, level: str, force: bool) -> dict:
        async with self._gpu_lock(idx), self._slot():
            rep = await self._child(idx, level, force)
        if idx in self.plugin.devices:  # not re-shaped meanwhile
            self._apply(idx, rep)
        return rep

    async def run_all(self) -> dict[int, dict]:
        """The pre-flight proper: every idle pool, one child each, in parallel."""
        todo = []
        for idx in sorted(self.plugin.devices):
            pool = self._pool(idx)
            if idx != pool[0]:
                continue
            if self.in_use(idx):
                self.reports[self._key(idx)] = {"skipped": "in use", "timestamp": time.time()}
                continue
            todo.append(idx)
        if todo:
            t0 = time.monotonic()
            await asyncio.gather(*(self._one(i, self.level, False) for i in todo))
            log.info("pre-flight %s (%s) of GPUs %s took %.1fs; failed: %s", self.NAME, self.level, todo,
                     time.monotonic() - t0, sorted(self.failed) or "none")
        return {i: self.report(i) for i in sorted(self.plugin.devices) if self.report(i) is not None}

    async def run_device(self, idx: int, level: str | None = None, force: bool = False) -> dict:
        """On demand (``POST /debug/memtest``): the same routine for one GPU.  With tenants on it only ``force``
        runs it, on what is free now minus a reserve."""
        level = level or (self.level if self.level != "off" else "quick")
        if level not in LEVELS[1:]:
            raise ValueError(f"level {level!r}: quick or full")
        if idx not in self.plugin.devices:
            raise KeyError(idx)
        busy = self.in_use(idx)
        if busy and not force:
            raise InUse(idx)
        return await self._one(self._pool(idx)[0], level, busy)

    # ------------------------------------------------------------ exposed state
    def metrics(self) -> list[str]:
        lines = []
        for name, key in self.METRICS:
            lines.append(f"# TYPE gpushare_plugin_{self.NAME}_{name} gauge")
            for i in sorted(self.plugin.devices):
                rep = self.report(i)
                if rep is None or "skipped" in rep or (rep.get("error") and key != "timestamp"):
                    continue
                lines.append(f'gpushare_plugin_{self.NAME}_{name}{{device="{i}"}} {rep.get(key, 0)}')
        lines += [f"# TYPE gpushare_plugin_{self.NAME}_errors_total counter",
                  f"gpushare_plugin_{self.NAME}_errors_total {self.errors_total}"]
        return lines


class ComputePreflight(Preflight):
    """``gsx-cutest`` through the same child-runner: per device, and never next to ``memory``'s child on one GPU."""
    NAME = "cutest"
    BAD = "bad_cu_count"
    METRICS = (("bad_cus", "bad_cu_count"), ("bad_waves", "bad_waves"), ("cus_seen", "cus_seen"),
               ("seconds", "seconds"), ("last_run_timestamp", "timestamp"))

    def __init__(self, plugin, level: str = "off", timeout: float = 120.0, cmd: list[str] | None = None,
                 memory: Preflight | None = None):
        super().__init__(plugin, level, 0.0, timeout, cmd or [str(CUTEST_TOOL)])
        self.memory = memory

    def _slot(self) -> asyncio.Semaphore:
        return self.memory._slot() if self.memory is not None else super()._slot()

    def _gpu_lock(self, idx: int) -> asyncio.Lock:
        return self.memory._gpu_lock(idx) if self.memory is not None else super()._gpu_lock(idx)

    def _key(self, idx: int) -> str:
        """By device: a partition's CUs are its own (the BDF tells physical GPUs apart, the index partitions)."""
        d = self.plugin.devices.get(idx)
        return f"#{idx}" if d is None else f"{d.bdf}#{idx}"

    def _pool(self, idx: int) -> list[int]:
        return [idx]

    def _argv(self, idx: int, level: str, force: bool) -> list[str]:
        d = self.plugin.devices[idx]
        argv = [*self.cmd, "--bdf", d.bdf] if d.bdf else [*self.cmd, "--device", str(idx)]
        argv += ["--level", level]
        if d.cu_count > 0:
            argv += ["--expect-cus", str(d.cu_count)]
        return [*argv, "--max-seconds", f"{0.8 * self.timeout:.3f}"]

    @staticmethod
    def reason(rep: dict) -> str:
        first = (rep.get("bad_cus") or [{}])[0]
        where = " ".join(f"{k} {first.get(k, 0)}" for k in ("xcc", "se", "sh", "cu"))
        return (f"cutest: {rep.get('bad_cu_count', 0)} bad CUs (first {where}, "
                f"units {','.join(first.get('units') or []) or '?'})")

