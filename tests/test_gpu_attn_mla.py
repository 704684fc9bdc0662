"""The MLA decode attention (native/kernels/attn_mla.hip) on a real MI355X: one latent row of 576 elements per token,
K (all 576) and V (the first 512) for all heads.

The library's table is 0 "4w-f1" and 1 "4w-f2" (4 waves, 1 or 2 tiles of 32 tokens in flight).  Every O lies between
guard rows of poison that have to stay poison, and starts as NaN, so a row that is not written shows.  No index is out
of range: a wrong kernel fails a comparison and reads nothing outside an allocation.
"""
import json
import math
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import attn_decode_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
DK, DV = 576, 512
CFGS = {0: ("4w-f1", 4, 1), 1: ("4w-f2", 4, 2)}
GUARD = 4  # guard rows on either side of O
POISON8 = 0xA5
SPLITS = (1, 2, 5)
HOWS = [None] + [(cfg, splits) for cfg in CFGS for splits in SPLITS]  # None: the dispatching entry point
kinds = pytest.mark.parametrize("kind", dc.KINDS)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    from gpushare_scheduler_extender_amd.ops import hip as h

    assert hasattr(h, "mla_decode_attn"), "the bindings have no MLA decode attention"
    return h


@pytest.fixture(scope="module")
def stream(hip):
    s = hip.Stream(0)
    yield s
    s.destroy()


def problem(kind, hq, page, lens, select, seed=0):
    """``dict(kind, q, cache, table, lens, scale, kv_scale, want)`` on the host; pages are handed out scattered, and
    slots past a sequence's end, three spare pages and the table entries past the end (which name them) hold NaN.
    ``select``: token t's 64 RoPE elements are the +-1 code of t (element i is bit i % 11 of t: two tokens differ in 5
    elements or more), head h's query is 32 times its target's code and zeros over the latent, and scale * kv_scale is
    1: the target's x is 32 * 64 * log2 e and every other token's lower by 32 * 10 * log2 e = 461 or more, so p is
    exactly 1 or 0.  The latent holds integers 1..15 that spell (page, slot, d); ``want`` is the target's latent times
    kv_scale (a power of two), exact.  Otherwise N(0, 1) data, and ``want`` is None."""
    gen = torch.Generator().manual_seed(seed)
    kv_scale = 1.0 if kind == "bf16" else (2.0 if select else 0.5)
    npages = [-(-n // page) for n in lens]
    total = sum(npages) + dc.POISON_PAGES
    order = dc._page_order(total, "scattered")
    stride = max(npages + [1])
    table = np.empty((len(lens), stride), dtype=np.int32)
    cache = torch.full((total, page, DK), float("nan"))
    q = torch.zeros(len(lens), hq, DK) if select else torch.randn(len(lens), hq, DK, generator=gen)
    want = torch.zeros(len(lens), hq, DV)
    bit = np.arange(64) % 11
    at = 0
    for b, n in enumerate(lens):
        table[b] = order[sum(npages) + (b + np.arange(stride)) % dc.POISON_PAGES]
        table[b, :npages[b]] = order[at:at + npages[b]]
        at += npages[b]
        if n == 0:
            continue
        t = np.arange(n)
        pp, slot = table[b][t // page].astype(np.int64), t % page
        if not select:
            cache[pp, slot] = torch.randn(n, DK, generator=gen) / kv_scale
            continue
        code = torch.from_numpy((2.0 * ((t[:, None] >> bit[None]) & 1) - 1).astype(np.float32))
        d = np.arange(DV)
        lat = 1 + ((((pp * page + slot)[:, None] >> (3 * (d % 7))) & 7) + d % 8)
        cache[pp, slot] = torch.cat([torch.from_numpy(lat.astype(np.float32)), code], dim=1)
        cuts = sorted({c for s in SPLITS for c in dc.split_cuts(n, s)})
        for h, tok in enumerate(dc.pick_targets(n, page, cuts, hq, b)):
            q[b, h, DV:] = 32 * code[tok]
            want[b, h] = cache[pp[tok], slot[tok], :DV] * kv_scale
    cache = cache.bfloat16() if kind == "bf16" else cache.to(dc.FP8)
    return dict(kind=kind, q=q.bfloat16(), cache=cache, table=torch.from_numpy(table),
                lens=torch.tensor(lens, dtype=torch.int32), scale=(1.0 if select else 192 ** -0.5) / kv_scale,
                kv_scale=kv_scale, want=want.bfloat16() if select else None)


class Launch:
    """A problem's operands on the device, a workspace for 5 splits (and for the dispatching entry point), and one
    guarded O per launch: the rows of NaN between GUARD rows of poison bytes on either side."""

    def __init__(self, hip, p):
        self.p, self.b, self.hq = p, *p["q"].shape[:2]
        self.page, self.max_len = p["cache"].shape[1], max(int(p["lens"].max()), 1)
        self.dev = tuple(p[x].cuda() for x in ("q", "cache", "table", "lens"))
        need = max(self.b * self.hq * 5 * 2056,
                   hip.mla_decode_attn_workspace_bytes(self.b, self.hq, self.page, self.max_len), 16)
        self.ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        self.front, self.body = GUARD * self.hq * DV * 2, self.b * self.hq * DV * 2
        self.outs = []

    def args(self, o) -> dict:
        p = self.p
        q, c, bt, sl = (x.data_ptr() for x in self.dev)
        return dict(kind=p["kind"], q=q, kv_cache=c, block_table=bt, seq_lens=sl, o=o.data_ptr() + self.front,
                    b=self.b, hq=self.hq, page=self.page, num_pages=p["cache"].shape[0],
                    table_stride=p["table"].shape[1], max_seq_len=self.max_len, scale=p["scale"],
                    kv_scale=p["kv_scale"], workspace=self.ws.data_ptr(), workspace_bytes=self.ws.numel())

    def fresh(self):
        o = torch.full((2 * self.front + self.body,), POISON8, dtype=torch.uint8, device="cuda")
        o[self.front:self.front + self.body] = 0xFF
        torch.cuda.synchronize()  # the fill is torch's: the test's stream does not wait for torch's
        self.outs.append(o)
        return o

    def run(self, hip, s, how):
        """One launch into a fresh O, not synchronised; the launches share the workspace and are ordered on ``s``."""
        a = self.args(self.fresh())
        if how is None:
            hip.mla_decode_attn(s, **a)
        elif how == "timed":
            assert hip.time_mla_decode_attn(s, iters=2, **a) > 0.0
        else:
            hip.mla_decode_attn_launch_cfg(s, cfg=how[0], splits=how[1], **a)

    def read(self, i: int, what: str):
        raw = self.outs[i].cpu()
        assert bool((raw[:self.front] == POISON8).all()) and bool((raw[self.front + self.body:] == POISON8).all()), \
            f"{what}: a guard row of O was written"
        return raw[self.front:self.front + self.body].view(torch.bfloat16).reshape(self.b, self.hq, DV)


# ---- 1. selection, bit for bit -----------------------------------------------------------------------------------------

@kinds
@pytest.mark.parametrize("hq", (1, 16, 17, 64, 65, 128))
@pytest.mark.parametrize("page", (16, 64))
def test_selection_returns_each_heads_target(hip, stream, kind, hq, page):
    p = problem(kind, hq, page, (0, 1, 31, 32, 33, 63, 64, 65, 200, 1100), select=True)
    run = Launch(hip, p)
    for how in HOWS:
        run.run(hip, stream, how)
    stream.sync()
    for i, how in enumerate(HOWS):
        dc.assert_bits_equal(run.read(i, f"{how}"), p["want"], f"{kind}, Hq {hq}, page {page}, (cfg, splits) {how}")


# ---- 2. bounded ----------------------------------------------------------------------------------------------------------

@kinds
@pytest.mark.parametrize("hq", (16, 128))
def test_random_data_stays_inside_the_bound(hip, stream, kind, hq):
    lens = (599, 31, 0, 256)
    p = problem(kind, hq, 16, lens, select=False, seed=7)
    q = p["q"].double().numpy()
    ref, vmax, s_max = np.zeros((len(lens), hq, DV)), np.zeros((len(lens), 1, DV)), 0.0
    for b, n in enumerate(lens):
        if n:
            t = np.arange(n)
            k = dc._float64(p["cache"][p["table"][b].numpy()[t // 16].astype(np.int64), t % 16]) * p["kv_scale"]
            x = q[b] @ k.T * p["scale"]
            w = np.exp(x - x.max(axis=1, keepdims=True))
            ref[b] = (w / w.sum(axis=1, keepdims=True)) @ k[:, :DV]
            vmax[b, 0] = np.abs(k[:, :DV]).max(axis=0)
            s_max = max(s_max, float((np.abs(q[b]) @ np.abs(k).T).max()))
    c = p["scale"] * dc.LOG2E  # k is dequantised: kv_scale is in S
    rel = 2 * math.log(2) * ((DK + 4) * dc.EPS * s_max * c + (max(lens) + 4) * dc.EPS / math.log(2))
    bound = dc.U * vmax + dc.U * np.abs(ref) + rel * vmax
    run = Launch(hip, p)
    for how in HOWS:
        run.run(hip, stream, how)
    stream.sync()
    for i, how in enumerate(HOWS):
        err = np.abs(run.read(i, f"{how}").double().numpy() - ref)
        print(f"{kind}, Hq {hq}, {how}: worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert not np.isnan(err).any(), f"{how}: NaN in O"
        assert (err <= bound).all(), f"{how}: {int((err > bound).sum())} of {err.size} elements outside the bound"


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------

WS_2_SPLITS = 2 * 16 * 2 * 2056  # B * Hq * splits * (512 + 2) * 4 of the problem below


@pytest.mark.parametrize("change,text", [
    (dict(hq=0), "need 1 <= Hq <= 128"),
    (dict(hq=129), "need 1 <= Hq <= 128"),
    (dict(page=24), "need page % 16 == 0 and 16 <= page <= 256"),
    (dict(kv_scale=0.5), "kv_scale must be 1.0"),
    (dict(cfg=0, splits=65), "need 1 <= splits <= 64"),
    (dict(cfg=1, splits=2, workspace_bytes=WS_2_SPLITS - 1), f"workspace too small: 2 splits need {WS_2_SPLITS} bytes"),
    (dict(o="q"), "O must not overlap Q"),
])
def test_refusals_launch_nothing(hip, stream, change, text):
    p = problem("bf16", 16, 16, (5, 40), select=True)
    run = Launch(hip, p)
    a = {**run.args(run.fresh()), **change}
    if a["o"] == "q":
        a["o"] = a["q"]
    with pytest.raises(hip.HipError, match=re.escape(text)):
        (hip.mla_decode_attn_launch_cfg if "cfg" in a else hip.mla_decode_attn)(stream, **a)
    stream.sync()
    raw = run.outs[0].cpu()
    assert bool((raw[run.front:run.front + run.body] == 0xFF).all()), "a refused call wrote to O"
    assert torch.equal(run.dev[0].cpu().view(torch.int16), p["q"].view(torch.int16)), "a refused call wrote to Q"


# ---- 4. the table and the timed call -------------------------------------------------------------------------------------

def test_the_library_has_the_table_the_docstring_lists(hip):
    assert {i: (hip.mla_decode_attn_cfg_name(i), *hip.mla_decode_attn_cfg_shape(i)) for i in CFGS} == CFGS
    assert hip.mla_decode_attn_cfg_name(len(CFGS)) is None and hip.mla_decode_attn_cfg_name(-1) is None
    with pytest.raises(hip.HipError):
        hip.mla_decode_attn_cfg_shape(len(CFGS))


@kinds
def test_the_timed_call_computes_what_the_plain_call_does(hip, stream, kind):
    run = Launch(hip, problem(kind, 17, 16, (70, 0, 33), select=False, seed=3))
    run.run(hip, stream, None)
    run.run(hip, stream, "timed")
    stream.sync()
    dc.assert_bits_equal(run.read(1, "timed"), run.read(0, "plain"), f"{kind}: the timed call")


# ---- 5. workload ---------------------------------------------------------------------------------------------------------

def test_the_attn_workload_runs_mla(hip):
    r = subprocess.run([sys.executable, str(ROOT / "samples" / "workload" / "main.py"), "--workload", "attn", "--mla",
                        "--kernel", "gsx", "--heads", "16", "--batch", "2", "--context", "1000", "--kv-gib", "0.05",
                        "--iters", "10", "--json"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["workload"] == "attn" and out["mla"] is True and out["kernel"] == "gsx", out
    assert np.isfinite(out["tbps"]) and out["tbps"] > 0 and np.isfinite(out["tflops"]) and out["tflops"] > 0
