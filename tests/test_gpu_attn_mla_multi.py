"""The multi-token MLA decode attention (native/kernels/attn_mla_multi.hip) on a real MI355X: T = 1..16 new tokens per
sequence, causal among themselves, over the paged latent cache.  Q and O are [B * T][Hq][..]; ``seq_lens`` holds the
lengths before the chunk, whose rows are already in the cache.

Every O lies between guard rows of poison that have to stay poison, and starts as NaN, so a row that is not written
shows.  No index is out of range: a wrong kernel fails a comparison and reads nothing outside an allocation.
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
FIXED = [(cfg, splits) for cfg in CFGS for splits in SPLITS]
HOWS = [None, *FIXED]  # None: the dispatching entry point
BASES = (0, 1, 15, 30, 31, 32, 33, 63, 200, 1090)
kinds = pytest.mark.parametrize("kind", dc.KINDS)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    from gpushare_scheduler_extender_amd.ops import hip as h

    assert hasattr(h, "mla_decode_attn_multi"), "the bindings have no multi-token MLA decode attention"
    return h


@pytest.fixture(scope="module")
def stream(hip):
    s = hip.Stream(0)
    yield s
    s.destroy()


def problem(kind, hq, t, page, bases, family, max_len=None, seed=0):
    """``dict(kind, t, q, cache, table, lens, max_len, scale, kv_scale, want)`` on the host, in the shape of
    ``problem()`` of tests/test_gpu_attn_mla.py: sequence b has ``end = min(bases[b] + t, max_len)`` rows in the cache,
    pages are handed out scattered, and slots at or past ``end``, three spare pages and the table entries past the end
    hold NaN.  The selection families give a token's 64 RoPE elements the +-1 code of a number below 2048, a column's
    query 32 times the code it asks for and zeros over the latent, so p is exactly 1 or 0; the latent holds integers
    1..15 that spell (page, slot, d).
      "own": token i has code i.  Column (new token j, head h) asks for its own token ``base + j`` when h is even and
             for an old token of ``dc.pick_targets`` (tile, page and split borders) when h is odd; ``want`` is that
             token's latent times kv_scale.
      0, 1:  (the shift s) new token j has code ``base + (j + s) // 2``, which it shares with its pair alone, and every
             column asks for its own token's code: the first of a pair wants its own latent, the second the pair's
             mean (l = 2: exact).
    A row at or past ``max_len`` wants zeros.  ``family`` None: N(0, 1) data, and ``want`` is None."""
    gen = torch.Generator().manual_seed(seed)
    select = family is not None
    kv_scale = 1.0 if kind == "bf16" else (2.0 if select else 0.5)
    max_len = max_len or max(bases) + t
    ends = [min(n + t, max_len) for n in bases]
    npages = [-(-n // page) for n in ends]
    total = sum(npages) + dc.POISON_PAGES
    order = dc._page_order(total, "scattered")
    stride = max(npages + [-(-max_len // page)])
    table = np.empty((len(bases), stride), dtype=np.int32)
    cache = torch.full((total, page, DK), float("nan"))
    q = torch.randn(len(bases), t, hq, DK, generator=gen) if not select else torch.zeros(len(bases), t, hq, DK)
    want = torch.zeros(len(bases), t, hq, DV)
    bit, d, at = np.arange(64) % 11, np.arange(DV), 0

    def code(i):
        return torch.from_numpy((2.0 * ((np.asarray(i)[..., None] >> bit) & 1) - 1).astype(np.float32))

    for b, (base, n) in enumerate(zip(bases, ends)):
        table[b] = order[sum(npages) + (b + np.arange(stride)) % dc.POISON_PAGES]
        table[b, :npages[b]] = order[at:at + npages[b]]
        at += npages[b]
        tok = np.arange(n)
        pp, slot = table[b][tok // page].astype(np.int64), tok % page
        if not select:
            cache[pp, slot] = torch.randn(n, DK, generator=gen) / kv_scale
            continue
        new = np.arange(t)
        number = tok.copy() if family == "own" else np.where(tok < base, tok, base + (tok - base + family) // 2)
        lat = torch.from_numpy((1 + ((((pp * page + slot)[:, None] >> (3 * (d % 7))) & 7) + d % 8)).astype(np.float32))
        cache[pp, slot] = torch.cat([lat, code(number)], dim=1)
        lat = torch.cat([lat, torch.zeros(base + t - n, DV)]) * kv_scale  # rows that are not live want zeros
        if family == "own":
            tgt = np.repeat(base + new[:, None], hq, axis=1)
            if base:
                cuts = sorted({c for s in SPLITS for c in dc.split_cuts(n, s)})
                old = np.array(dc.pick_targets(base, page, cuts, t * (hq // 2), b)).reshape(t, hq // 2)
                tgt[:, 1::2] = np.where(base + new[:, None] < max_len, old, tgt[:, 1::2])
            q[b, :, :, DV:] = 32 * code(tgt)
            want[b] = lat[tgt]
        else:
            q[b, :, :, DV:] = 32 * code(base + (new + family) // 2)[:, None]
            second = (new > 0) & ((new + family) % 2 == 1) & (base + new < max_len)
            mine = lat[base + new]
            mine[second] = (mine[second] + lat[base + new[second] - 1]) / 2
            want[b] = mine[:, None]
    cache = cache.bfloat16() if kind == "bf16" else cache.to(dc.FP8)
    return dict(kind=kind, t=t, q=q.bfloat16().reshape(-1, hq, DK), cache=cache, table=torch.from_numpy(table),
                lens=torch.tensor(bases, dtype=torch.int32), max_len=max_len,
                scale=(1.0 if select else 192 ** -0.5) / kv_scale, kv_scale=kv_scale,
                want=want.bfloat16().reshape(-1, hq, DV) if select else None)


class Launch:
    """A problem's operands on the device, a workspace for 5 splits (and for the dispatching entry point), and one
    guarded O per launch: the rows of NaN between GUARD rows of poison bytes on either side."""

    def __init__(self, hip, p):
        self.p, self.t, self.hq, self.b = p, p["t"], p["q"].shape[1], len(p["lens"])
        self.page = p["cache"].shape[1]
        self.dev = tuple(p[x].cuda() for x in ("q", "cache", "table", "lens"))
        need = max(self.b * self.t * self.hq * 5 * 2056,
                   hip.mla_decode_attn_multi_workspace_bytes(self.b, self.t, self.hq, self.page, p["max_len"]), 16)
        self.ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        self.front, self.body = GUARD * self.hq * DV * 2, self.b * self.t * self.hq * DV * 2
        self.outs = []

    def args(self, o) -> dict:
        p = self.p
        q, c, bt, sl = (x.data_ptr() for x in self.dev)
        return dict(kind=p["kind"], q=q, kv_cache=c, block_table=bt, seq_lens=sl, o=o.data_ptr() + self.front,
                    b=self.b, t=self.t, hq=self.hq, page=self.page, num_pages=p["cache"].shape[0],
                    table_stride=p["table"].shape[1], max_seq_len=p["max_len"], scale=p["scale"],
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
            hip.mla_decode_attn_multi(s, **a)
        elif how == "timed":
            assert hip.time_mla_decode_attn_multi(s, iters=2, **a) > 0.0
        elif how[0] == "single":  # gsx_mla_decode_attn on the lengths after the one new token
            del a["t"]
            a["seq_lens"] = self.lens1.data_ptr()
            hip.mla_decode_attn_launch_cfg(s, cfg=how[1], splits=how[2], **a)
        else:
            hip.mla_decode_attn_multi_launch_cfg(s, cfg=how[0], splits=how[1], **a)

    def read(self, i: int, what: str):
        raw = self.outs[i].cpu()
        assert bool((raw[:self.front] == POISON8).all()) and bool((raw[self.front + self.body:] == POISON8).all()), \
            f"{what}: a guard row of O was written"
        return raw[self.front:self.front + self.body].view(torch.bfloat16).reshape(-1, self.hq, DV)

    def check_all(self, hip, s, want, what):
        for how in HOWS:
            self.run(hip, s, how)
        s.sync()
        for i, how in enumerate(HOWS):
            dc.assert_bits_equal(self.read(i, f"{how}"), want, f"{what}, (cfg, splits) {how}")


# ---- 1, 2. selection, bit for bit -----------------------------------------------------------------------------------------

@kinds
@pytest.mark.parametrize("family", ("own", 0, 1))
@pytest.mark.parametrize("hq,t", ((1, 2), (3, 16), (16, 4), (17, 3), (48, 2), (64, 2), (128, 3)))
@pytest.mark.parametrize("page", (16, 64))
def test_selection_returns_each_columns_target(hip, stream, kind, family, hq, t, page):
    p = problem(kind, hq, t, page, BASES, family)
    Launch(hip, p).check_all(hip, stream, p["want"], f"{kind}, family {family}, Hq {hq}, T {t}, page {page}")


@kinds
@pytest.mark.parametrize("family", ("own", 1))
def test_rows_past_max_seq_len_are_zeros(hip, stream, kind, family):
    """Sequence 0 has one live row, sequence 1 none; their neighbours' rows are those of a launch without them."""
    p = problem(kind, 17, 4, 16, (69, 70, 20, 66), family, max_len=70)
    assert bool((p["want"][1:8] == 0).all()) and bool((p["want"][0] != 0).all())  # rows b * T + t
    Launch(hip, p).check_all(hip, stream, p["want"], f"{kind}, family {family}, max_seq_len 70")


# ---- 3. T == 1 ------------------------------------------------------------------------------------------------------------

@kinds
@pytest.mark.parametrize("hq", (16, 65))
def test_one_new_token_gives_the_bits_of_the_single_token_kernel(hip, stream, kind, hq):
    run = Launch(hip, problem(kind, hq, 1, 16, (70, 0, 33, 599), None, seed=5))
    run.lens1 = (run.p["lens"] + 1).cuda()
    for how in FIXED:
        run.run(hip, stream, how)
        run.run(hip, stream, ("single", *how))
    stream.sync()
    for i, how in enumerate(FIXED):
        dc.assert_bits_equal(run.read(2 * i, f"{how}"), run.read(2 * i + 1, "single").cpu(), f"{kind}, Hq {hq}, {how}")


# ---- 4. bounded -----------------------------------------------------------------------------------------------------------

@kinds
@pytest.mark.parametrize("hq,t", ((16, 4), (128, 2)))
def test_random_data_stays_inside_the_bound(hip, stream, kind, hq, t):
    """The bound of tests/test_gpu_attn_mla.py, its sequence-length term taken at the longest ``end``."""
    bases = (599, 31, 0, 256)
    p = problem(kind, hq, t, 16, bases, None, seed=7)
    q = p["q"].double().numpy().reshape(len(bases), t, hq, DK)
    ref, vmax, s_max = np.zeros((len(bases), t, hq, DV)), np.zeros((len(bases), t, 1, DV)), 0.0
    for b, base in enumerate(bases):
        tok = np.arange(base + t)
        k = dc._float64(p["cache"][p["table"][b].numpy()[tok // 16].astype(np.int64), tok % 16]) * p["kv_scale"]
        for j in range(t):
            x = q[b, j] @ k[:base + j + 1].T * p["scale"]
            w = np.exp(x - x.max(axis=1, keepdims=True))
            ref[b, j] = (w / w.sum(axis=1, keepdims=True)) @ k[:base + j + 1, :DV]
            s_max = max(s_max, float((np.abs(q[b, j]) @ np.abs(k[:base + j + 1]).T).max()))
            vmax[b, j, 0] = np.abs(k[:base + j + 1, :DV]).max(axis=0)
    c = p["scale"] * dc.LOG2E  # k is dequantised: kv_scale is in S
    rel = 2 * math.log(2) * ((DK + 4) * dc.EPS * s_max * c + (max(bases) + t + 4) * dc.EPS / math.log(2))
    bound = (dc.U * vmax + dc.U * np.abs(ref) + rel * vmax).reshape(-1, hq, DV)
    ref = ref.reshape(-1, hq, DV)
    run = Launch(hip, p)
    for how in HOWS:
        run.run(hip, stream, how)
    stream.sync()
    for i, how in enumerate(HOWS):
        err = np.abs(run.read(i, f"{how}").double().numpy() - ref)
        print(f"{kind}, Hq {hq}, T {t}, {how}: worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert not np.isnan(err).any(), f"{how}: NaN in O"
        assert (err <= bound).all(), f"{how}: {int((err > bound).sum())} of {err.size} elements outside the bound"


# ---- 5. refusals and the table ------------------------------------------------------------------------------------------

WS_2_SPLITS = 2 * 3 * 16 * 2 * 2056  # B * T * Hq * splits * (512 + 2) * 4 of the problem below


@pytest.mark.parametrize("change,text", [
    (dict(t=0), "need 1 <= T <= 16"),
    (dict(t=17), "need 1 <= T <= 16"),
    (dict(hq=129), "need 1 <= Hq <= 128"),
    (dict(page=24), "need page % 16 == 0 and 16 <= page <= 256"),
    (dict(q=0), "Q, KV_cache, O, block_table and seq_lens must not be NULL"),
    (dict(o="q"), "O must not overlap Q"),
    (dict(cfg=1, splits=2, workspace_bytes=WS_2_SPLITS - 1), f"workspace too small: 2 splits need {WS_2_SPLITS} bytes"),
])
def test_refusals_launch_nothing(hip, stream, change, text):
    p = problem("bf16", 16, 3, 16, (5, 40), "own")
    run = Launch(hip, p)
    a = {**run.args(run.fresh()), **change}
    if a["o"] == "q":
        a["o"] = a["q"]
    with pytest.raises(hip.HipError, match=re.escape(text)):
        (hip.mla_decode_attn_multi_launch_cfg if "cfg" in a else hip.mla_decode_attn_multi)(stream, **a)
    stream.sync()
    raw = run.outs[0].cpu()
    assert bool((raw[run.front:run.front + run.body] == 0xFF).all()), "a refused call wrote to O"
    assert torch.equal(run.dev[0].cpu().view(torch.int16), p["q"].view(torch.int16)), "a refused call wrote to Q"


def test_the_library_has_the_table_the_docstring_lists(hip):
    doc = " ".join(hip.mla_decode_attn_multi_cfg_shape.__doc__.split())
    for i, (name, waves, inflight) in CFGS.items():
        assert (hip.mla_decode_attn_multi_cfg_name(i), *hip.mla_decode_attn_multi_cfg_shape(i)) == CFGS[i]
        assert f'{i} "{name}": ({waves}, {inflight})' in doc
    assert hip.mla_decode_attn_multi_cfg_name(len(CFGS)) is None and hip.mla_decode_attn_multi_cfg_name(-1) is None
    with pytest.raises(hip.HipError):
        hip.mla_decode_attn_multi_cfg_shape(len(CFGS))


# ---- 6, 7. the timed call and the workload --------------------------------------------------------------------------------

@kinds
def test_the_timed_call_computes_what_the_plain_call_does(hip, stream, kind):
    run = Launch(hip, problem(kind, 17, 3, 16, (70, 0, 33), None, seed=3))
    run.run(hip, stream, None)
    run.run(hip, stream, "timed")
    stream.sync()
    dc.assert_bits_equal(run.read(1, "timed"), run.read(0, "plain"), f"{kind}: the timed call")


def test_the_attn_workload_runs_multi_token_mla(hip):
    r = subprocess.run([sys.executable, str(ROOT / "samples" / "workload" / "main.py"), "--workload", "attn", "--mla",
                        "--new-tokens", "4", "--kernel", "gsx", "--heads", "16", "--batch", "2", "--context", "1000",
                        "--kv-gib", "0.05", "--iters", "10", "--json"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["workload"] == "attn" and out["mla"] is True and out["new_tokens"] == 4, out
    assert all(np.isfinite(out[k]) and out[k] > 0 for k in ("tokens_per_s", "tbps", "tflops")), out
