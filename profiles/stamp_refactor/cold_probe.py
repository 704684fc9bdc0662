"""First-call cost of a stamp: after a fill (as scripts/bench_kernels.py takes it) and as the process's first kernel."""
import json
import sys
import time

from gpushare_scheduler_extender_amd.ops import hip

GiB, MiB = 1 << 30, 1 << 20
s = hip.Stream(0)
buf = hip.DeviceBuffer(0, 4 * GiB)
s.sync()


def timed(f):
    t = time.perf_counter()
    f()
    s.sync()
    return round((time.perf_counter() - t) * 1e6, 1)


def stamp():
    hip.hbm_stamp(s, buf.addr(), 4 * GiB, MiB, 42)


def fill():
    hip.hbm_fill(s, buf.addr(), 16 * MiB, 1)


order = sys.argv[1]
out = {"order": order}
for i, name in enumerate(order.split(",")):
    out[f"{i}:{name}_us"] = timed(stamp if name == "stamp" else fill)
buf.free()
s.destroy()
print(json.dumps(out))
