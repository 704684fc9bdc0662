"""Warm p50 of the single-range entry points (hbm_stamp + sync, hbm_verify): the rows bench_kernels.py takes cold."""
import json
import time

from gpushare_scheduler_extender_amd.ops import hip

GiB, MiB = 1 << 30, 1 << 20


def p50(f, n=200):
    for _ in range(20):
        f()
    ts = []
    for _ in range(n):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    ts.sort()
    return round(ts[len(ts) // 2] * 1e6, 1)


s = hip.Stream(0)
big = hip.DeviceBuffer(0, 64 * GiB)
small = hip.DeviceBuffer(0, 64 * MiB)


def stamp(buf, n, st):
    hip.hbm_stamp(s, buf.addr(), n, st, 42)
    s.sync()


out = {
    "stamp 64 GiB @1 MiB + sync, p50 us": p50(lambda: stamp(big, 64 * GiB, MiB)),
    "verify 64 GiB @1 MiB, p50 us": p50(lambda: hip.hbm_verify(s, big.addr(), 64 * GiB, MiB, 42)),
    "stamp 64 MiB @16 B (4 Mi stamps) + sync, p50 us": p50(lambda: stamp(small, 64 * MiB, 16)),
    "verify 64 MiB @16 B (4 Mi stamps), p50 us": p50(lambda: hip.hbm_verify(s, small.addr(), 64 * MiB, 16, 42)),
}
assert hip.hbm_verify(s, small.addr(), 64 * MiB, 16, 42) == 0
big.free()
small.free()
s.destroy()
print(json.dumps(out))
