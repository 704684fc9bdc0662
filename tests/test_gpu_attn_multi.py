"""The multi-token decode attention (native/kernels/attn_decode_multi.hip) on a real MI355X.

Problems, the fp64 reference and the error bound are those of ``tests/attn_prefill_cases.py``: the entry point has the
semantics of ``gsx_prefill_attn``.  The library's table is 0 "4w-f1" (4 waves, 1 tile in flight) and 1 "4w-f2" (4 waves,
2 tiles).  Every O lies between guard rows of poison that have to stay poison, and starts as NaN, so a row that is not
written shows.  No index is out of range: a wrong kernel fails a comparison and reads nothing outside an allocation.
"""
import json
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import attn_prefill_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
CFGS = {0: ("4w-f1", 4, 1), 1: ("4w-f2", 4, 2)}
GUARD = 4  # guard rows on either side of O
POISON8 = 0xA5
# (G, T): one, two and four fragments of 16 columns, a fragment border inside one token's group of heads, G not a power
# of two, both limits of G * T
SHAPES = ((1, 2), (4, 4), (4, 5), (3, 7), (16, 4), (8, 8), (4, 16))
# the causal edge inside a tile of 32, on its border and across two tiles, across a page, and a sequence that starts empty
BASES = (0, 1, 30, 31, 32, 33, 200)
HOWS = [None] + [(cfg, splits) for cfg in CFGS for splits in (1, 2, 5)]  # None: the dispatching entry point
kinds = pytest.mark.parametrize("kind", pc.KINDS)
shapes = pytest.mark.parametrize("g,t", SHAPES)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    from gpushare_scheduler_extender_amd.ops import hip as h

    assert hasattr(h, "decode_attn_multi"), "the bindings have no multi-token decode attention"
    return h


@pytest.fixture(scope="module")
def stream(hip):
    s = hip.Stream(0)
    yield s
    s.destroy()


class Launch:
    """A problem's operands on the device, a workspace for 5 splits (and for the dispatching entry point), and one
    guarded O per launch: ``rows`` rows of NaN between GUARD rows of poison bytes on either side."""

    def __init__(self, hip, p: pc.Problem):
        self.p = p
        self.dev = tuple(x.cuda() for x in (p.q, p.k_cache, p.v_cache, p.block_table, p.seq_lens))
        need = max(p.b * p.t * p.hq * 5 * 520, hip.decode_attn_multi_workspace_bytes(p.b, p.t, p.hq, pc.D, p.page,
                                                                                     p.max_seq_len), 16)
        self.ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        self.front, self.body = GUARD * p.hq * pc.D * 2, p.b * p.t * p.hq * pc.D * 2
        self.outs = []

    def args(self, o: torch.Tensor) -> dict:
        p = self.p
        q, k, v, bt, sl = (x.data_ptr() for x in self.dev)
        return dict(kind=p.kind, q=q, k_cache=k, v_cache=v, block_table=bt, seq_lens=sl, o=o.data_ptr() + self.front,
                    b=p.b, t=p.t, hq=p.hq, hkv=p.hkv, d=pc.D, page=p.page, num_pages=p.num_pages,
                    table_stride=p.table_stride, max_seq_len=p.max_seq_len, scale=p.scale, k_scale=p.k_scale,
                    v_scale=p.v_scale, workspace=self.ws.data_ptr(), workspace_bytes=self.ws.numel())

    def fresh(self) -> torch.Tensor:
        o = torch.full((2 * self.front + self.body,), POISON8, dtype=torch.uint8, device="cuda")
        o[self.front:self.front + self.body] = 0xFF
        torch.cuda.synchronize()  # the fill is torch's: the test's stream does not wait for torch's
        self.outs.append(o)
        return o

    def run(self, hip, s, how):
        """One launch into a fresh O, not synchronised.  The launches of one Launch share the workspace: they are
        ordered on the stream."""
        a = self.args(self.fresh())
        if how is None:
            hip.decode_attn_multi(s, **a)
        elif how == "timed":
            assert hip.time_decode_attn_multi(s, iters=2, **a) > 0.0
        else:
            hip.decode_attn_multi_launch_cfg(s, cfg=how[0], splits=how[1], **a)

    def read(self, i: int, what: str) -> torch.Tensor:
        raw = self.outs[i].cpu()
        assert bool((raw[:self.front] == POISON8).all()) and bool((raw[self.front + self.body:] == POISON8).all()), \
            f"{what}: a guard row of O was written"
        return raw[self.front:self.front + self.body].view(torch.bfloat16).reshape(-1, self.p.hq, pc.D)


def _bits(x: torch.Tensor) -> torch.Tensor:
    return x.contiguous().view(torch.int16)


def _all_hows_return(hip, stream, p: pc.Problem, what: str):
    run = Launch(hip, p)
    for how in HOWS:
        run.run(hip, stream, how)
    stream.sync()
    for i, how in enumerate(HOWS):
        got = run.read(i, f"{what}, {how}")
        assert torch.equal(_bits(got), _bits(p.want)), f"{what}, (cfg, splits) {how}: O is not each row's own token"


# ---- 1. bit for bit ------------------------------------------------------------------------------------------------------

@kinds
@shapes
@pytest.mark.parametrize("page", (16, 64))
def test_staircase_returns_each_rows_own_token(hip, stream, kind, g, t, page):
    p = pc.staircase_problem(kind, g, page, t, BASES, **pc.fp8_scales(kind))
    _all_hows_return(hip, stream, p, f"{kind}, G {g}, T {t}, page {page}")


# ---- 2. bounded ----------------------------------------------------------------------------------------------------------

@kinds
@pytest.mark.parametrize("g,t", ((8, 8), (16, 4), (1, 16)))
def test_random_data_stays_inside_the_bound(hip, stream, kind, g, t):
    p = pc.random_problem(kind, 7, g, 16, t, (599, 31, 0, 256))
    bound, ref, _ = pc.error_bound(p)
    run = Launch(hip, p)
    hows = [None, (0, 3), (1, 3)]
    for how in hows:
        run.run(hip, stream, how)
    stream.sync()
    for i, how in enumerate(hows):
        err = np.abs(run.read(i, f"{how}").double().numpy() - ref)
        print(f"{kind}, G {g}, T {t}, {how}: worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert not np.isnan(err).any(), f"{how}: NaN in O"
        assert (err <= bound).all(), f"{how}: {int((err > bound).sum())} of {err.size} elements outside the bound"


# ---- 3. dead rows --------------------------------------------------------------------------------------------------------

@kinds
@shapes
def test_a_row_past_max_seq_len_is_zeros(hip, stream, kind, g, t):
    p = pc.staircase_problem(kind, g, 16, t, (40,), max_seq_len=40 + t - 1, **pc.fp8_scales(kind))
    assert p.live() == [t - 1] and not bool(p.want[-1].float().abs().sum())
    _all_hows_return(hip, stream, p, f"{kind}, G {g}, T {t}, the last row dead")


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------

WS_2_SPLITS = 2 * 4 * 8 * 2 * 520  # B * T * Hq * splits * 520 of the problem below


@pytest.mark.parametrize("change,text", [
    (dict(t=0), "need 1 <= T <= 16"),
    (dict(t=17), "need 1 <= T <= 16"),
    (dict(hq=26, hkv=2, t=5), "need (Hq / Hkv) * T <= 64"),
    (dict(cfg=0, splits=65), "need 1 <= splits <= 64"),
    (dict(cfg=1, splits=2, workspace_bytes=WS_2_SPLITS - 1), f"workspace too small: 2 splits need {WS_2_SPLITS} bytes"),
    (dict(o="q"), "O must not overlap Q"),
])
def test_refusals_launch_nothing(hip, stream, change, text):
    p = pc.staircase_problem("bf16", 4, 16, 4, (5, 40))
    run = Launch(hip, p)
    a = {**run.args(run.fresh()), **change}
    if a["o"] == "q":
        a["o"] = a["q"]
    with pytest.raises(hip.HipError, match=re.escape(text)):
        (hip.decode_attn_multi_launch_cfg if "cfg" in a else hip.decode_attn_multi)(stream, **a)
    stream.sync()
    raw = run.outs[0].cpu()
    assert bool((raw[run.front:run.front + run.body] == 0xFF).all()), "a refused call wrote to O"
    assert torch.equal(run.dev[0].cpu(), p.q), "a refused call wrote to Q"


# ---- 5. tables and timing ------------------------------------------------------------------------------------------------

def test_the_library_has_the_table_the_docstring_lists(hip):
    assert {i: (hip.decode_attn_multi_cfg_name(i), *hip.decode_attn_multi_cfg_shape(i)) for i in CFGS} == CFGS
    assert hip.decode_attn_multi_cfg_name(len(CFGS)) is None and hip.decode_attn_multi_cfg_name(-1) is None
    with pytest.raises(hip.HipError):
        hip.decode_attn_multi_cfg_shape(len(CFGS))


@kinds
def test_the_timed_call_computes_what_the_plain_call_does(hip, stream, kind):
    p = pc.random_problem(kind, 3, 4, 16, 5, (70, 0, 33))
    run = Launch(hip, p)
    run.run(hip, stream, None)
    run.run(hip, stream, "timed")
    stream.sync()
    assert torch.equal(_bits(run.read(0, "plain")), _bits(run.read(1, "timed")))


# ---- 6. workload ---------------------------------------------------------------------------------------------------------

def test_the_attn_workload_runs_several_new_tokens(hip):
    r = subprocess.run([sys.executable, str(ROOT / "samples" / "workload" / "main.py"), "--workload", "attn", "--kernel",
                        "gsx", "--new-tokens", "4", "--batch", "2", "--context", "1000", "--kv-gib", "0.05", "--iters",
                        "10", "--json"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["workload"] == "attn" and out["new_tokens"] == 4 and out["kernel"] == "gsx", out
    assert np.isfinite(out["tbps"]) and out["tbps"] > 0 and np.isfinite(out["tokens_per_s"]) and out["tokens_per_s"] > 0
