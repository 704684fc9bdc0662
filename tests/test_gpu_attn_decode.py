"""The decode attention (native/kernels/attn_decode.hip) on a real MI355X.

Problems, the fp64 reference and the error bound are those of ``tests/attn_decode_cases.py``, which
``tests/test_attn_decode_cases.py`` checks on the CPU.  The selection cases are compared on the raw 16 bits of every
element: they test addressing (block tables, pages, splits, waves, masking) and need no tolerance.  The window cases,
compared in the same way, test that every token is counted exactly once.  The random cases are compared with the
derived bound.  One case holds a page index above ``num_pages - 1`` (``attn_decode_cases.page_clamp_problem``), and
its caches reach three pages further than ``num_pages`` says; no other index is out of range and none is negative, so
a wrong kernel fails a comparison and reads nothing outside an allocation.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import attn_decode_cases as ac  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
ROOT = Path(__file__).resolve().parents[1]
WS_BYTES = 16 << 20
KIND_CFG = [(kind, cfg) for kind in ac.KINDS for cfg in ac.ALL]
kind_cfg = pytest.mark.parametrize("kind,cfg", KIND_CFG,
                                   ids=[f"{k}-{'dispatch' if c is None else c}" for k, c in KIND_CFG])


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    from gpushare_scheduler_extender_amd.ops import hip as h

    assert h.SO.exists()
    assert hasattr(h, "decode_attn_cfgs"), "the bindings have no decode attention"
    assert h.decode_attn_cfgs() == ac.CFGS
    return h


@pytest.fixture(scope="module")
def stream(hip):
    s = hip.Stream(0)
    yield s
    s.destroy()


@pytest.fixture(scope="module")
def ws():
    """The workspace of every test.  ``Dev.run`` sets the part a launch may use to fp32 NaN first (a few KiB for
    most cases, a few MiB at 64 splits): a partial the kernel fails to write is then merged as NaN, never as an earlier
    problem's."""
    return torch.full((WS_BYTES // 4,), NAN, device="cuda", dtype=torch.float32)


class Dev:
    """A problem's operands on the device; ``run`` launches into a fresh NaN ``O`` and returns it (not synchronised)."""

    def __init__(self, p: ac.Problem, tensors=None):
        self.p = p
        self.t = tensors or tuple(t.cuda() for t in (p.q, p.k_cache, p.v_cache, p.block_table, p.seq_lens))

    def run(self, hip, s, ws, cfg, splits=None, o=None):
        p = self.p
        q, k, v, bt, sl = self.t
        o = torch.full((p.b, p.hq, ac.D), NAN, device="cuda", dtype=torch.bfloat16) if o is None else o
        if cfg is None:
            assert splits is None
            used = hip.decode_attn_workspace_bytes(p.b, p.hq, ac.D, p.page, p.max_seq_len)
        else:
            used = p.b * p.hq * splits * ac.PARTIAL_BYTES if splits > 1 else 0
        assert used <= ws.numel() * 4
        # ``s`` does not wait for torch's stream, nor torch's for it: an earlier launch, on any stream, has to have
        # merged its partials before they are overwritten, and the fill has to be done before this launch
        torch.cuda.synchronize()
        ws[:used // 4].fill_(NAN)
        torch.cuda.synchronize()
        args = (s, p.kind, q.data_ptr(), k.data_ptr(), v.data_ptr(), bt.data_ptr(), sl.data_ptr(), o.data_ptr(), p.b,
                p.hq, p.hkv, ac.D, p.page, p.num_pages, p.table_stride, p.max_seq_len, p.scale)
        tail = (p.k_scale, p.v_scale, ws.data_ptr(), ws.numel() * 4)
        if cfg is None:
            hip.decode_attn(*args, *tail)
        else:
            hip.decode_attn_cfg(*args, cfg, splits, *tail)
        return o


def _splits_of(cfg):
    return (None,) if cfg is None else ac.SPLITS


def _check(hip, stream, ws, problems, cfg, what):
    """Every problem on the configuration with each of its split counts, launched first and compared afterwards."""
    runs = []
    for name, p in problems:
        d = Dev(p)
        runs += [(f"{what}, {name}, splits {s}", p, d.run(hip, stream, ws, cfg, s)) for s in _splits_of(cfg)]
    stream.sync()
    for name, p, o in runs:
        ac.assert_bits_equal(o, p.want, name)


# ---- 1. selection: groups, short lengths, page sizes ------------------------------------------------------------------

@kind_cfg
def test_attn_selects_across_groups_and_short_lengths(hip, stream, ws, kind, cfg):
    """G in 1, 2, 4, 8, 16 with Hkv = 2, pages of 16 and 64, and the lengths 0 .. 33 around the 16-token half and the
    32-token tile (the length is below G for some), five and four sequences to a batch, with every split count: most
    splits and most waves then have no token at all.  Poison around: past the lengths, in the unused table entries."""
    _check(hip, stream, ws, ac.short_cases(kind), cfg, f"{kind} cfg {cfg}")


# ---- 2. selection: what a wave and a split do -------------------------------------------------------------------------

@kind_cfg
def test_attn_selects_at_every_wave_and_split_boundary(hip, stream, ws, kind, cfg):
    """``attn_decode_cases.split_lengths``: waves without a tile, ragged rounds, the conditional prologue, the steady
    loop and the drain, per split; splits without a token and with one.  G = 16: the 32 heads of every sequence
    target its first and last token and both sides of every cut of every split count tested, so every split that
    has a token holds a target and its partial decides some head's row; the other heads take half, tile and page
    boundaries spread over the whole sequence (``attn_decode_cases.pick_targets``, asserted in the CPU test)."""
    for splits in _splits_of(cfg):
        runs = [(name, p, Dev(p).run(hip, stream, ws, cfg, splits))
                for name, p in ac.split_cases(kind, cfg, splits or 1)]
        stream.sync()
        for name, p, o in runs:
            ac.assert_bits_equal(o, p.want, f"{kind} cfg {cfg}, splits {splits}, {name}")


# ---- 3. selection: block tables, strides, clamped lengths -------------------------------------------------------------

@kind_cfg
def test_attn_follows_block_tables(hip, stream, ws, kind, cfg):
    """Reversed and scattered page orders, a table shared by two sequences, a ``table_stride`` larger than needed, a
    batch that mixes 0 and short lengths with ``max_seq_len``, ``seq_lens`` entries above ``max_seq_len`` that the
    kernel clamps (the slots past it are poison), and entries of -1 and -2^31, clamped to 0: rows of zeros next to a
    live sequence."""
    _check(hip, stream, ws, ac.table_cases(kind), cfg, f"{kind} cfg {cfg}")


# ---- 4. guard bands and 16-B-only alignment -------------------------------------------------------------------------

def _banded(t: torch.Tensor, fill: int):
    """``t`` 16 B past a 256-B boundary inside a byte allocation filled with ``fill``: ``(whole, view)``."""
    raw = t.contiguous().view(torch.uint8).flatten()
    whole = torch.full((4096 + 16 + raw.numel() + 4096,), fill, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 256 == 0
    whole[4096 + 16:4096 + 16 + raw.numel()] = raw.cuda()
    view = whole[4096 + 16:4096 + 16 + raw.numel()].view(t.dtype).view(t.shape)
    assert view.data_ptr() % 32 == 16
    return whole, view


@kind_cfg
def test_attn_guard_bands_and_minimum_alignment(hip, stream, ws, kind, cfg):
    """Every operand 16 B past a 32-B boundary between bands of 0xFF bytes (bf16, e4m3 and fp32 NaN; a page index or a
    length of -1), G = 5 so that rows 5..15 of a group's Q are the next group's or the band.  O's band has to stay as
    it was and nothing else may be written."""
    p = ac.selection_problem(kind, 5, 16, [50, 0, 17], **ac.fp8_scales(kind))
    pairs = [_banded(t, 0xFF) for t in (p.q, p.k_cache, p.v_cache, p.block_table, p.seq_lens)]
    wo, o = _banded(torch.full((p.b, p.hq, ac.D), NAN, dtype=torch.bfloat16), 0xC3)
    before = [w.clone() for w, _ in pairs]
    d = Dev(p, tuple(v for _, v in pairs))
    for splits in _splits_of(cfg):
        o.fill_(NAN)
        d.run(hip, stream, ws, cfg, splits, o)
        stream.sync()
        assert bool((wo[:4096 + 16] == 0xC3).all()) and bool((wo[4096 + 16 + o.numel() * 2:] == 0xC3).all()), \
            f"{kind} cfg {cfg} splits {splits}: a band of O was written"
        ac.assert_bits_equal(o, p.want, f"{kind} cfg {cfg} splits {splits}")
    for (w, _), w0 in zip(pairs, before):
        assert torch.equal(w, w0), f"{kind} cfg {cfg}: an operand or a band of it was written"


# ---- 5. a cache past 4 GiB --------------------------------------------------------------------------------------------

def test_attn_cache_past_4_gib(hip, stream, ws):
    """bf16, Hkv = 2, page 64: a page is 32 KiB, so page 131072 starts at byte 2^32 and a few more pages make a cache of
    just over 4 GiB.  The case's pages lie past that offset; only they (used and poison) are written."""
    first = (1 << 32) // (2 * 64 * ac.D * 2)
    assert first * 2 * 64 * ac.D * 2 == 1 << 32
    moved = ac.selection_problem("bf16", 16, 64, [700, 65, 1], tables="scattered", page_base=first + 7,
                                 cuts=[ac.all_cuts(n) for n in (700, 65, 1)])
    assert int(moved.block_table.min()) >= first + 7 and moved.num_pages * 2 * 64 * ac.D * 2 > 1 << 32
    need = 2 * moved.num_pages * 2 * 64 * ac.D * 2 + (1 << 30)
    free, _ = hip.mem_info(0)
    if free < need:
        pytest.skip(f"{free >> 20} MiB free on the device, {need >> 20} MiB needed")
    k = torch.empty((moved.num_pages, 2, 64, ac.D), dtype=torch.bfloat16, device="cuda")
    v = torch.empty_like(k)
    k[first + 7:] = moved.k_cache.cuda()
    v[first + 7:] = moved.v_cache.cuda()
    d = Dev(moved, (moved.q.cuda(), k, v, moved.block_table.cuda(), moved.seq_lens.cuda()))
    for cfg in ac.ALL:
        for splits in _splits_of(cfg):
            o = d.run(hip, stream, ws, cfg, splits)
            stream.sync()
            ac.assert_bits_equal(o, moved.want, f"cfg {cfg} splits {splits}, pages past byte 2^32")
    del k, v, d
    torch.cuda.empty_cache()


# ---- 6. random inputs: the bound, determinism, placement --------------------------------------------------------------

@pytest.fixture(scope="module")
def random_cases():
    """``{(kind, seed): (problem, fp64 reference, bound)}``, computed once."""
    out = {}
    for kind in ac.KINDS:
        for case in ac.RANDOM_CASES:
            p = ac.random_problem(kind, *case)
            out[kind, case[0]] = (p, ac.reference(p), ac.error_bound(p)[0])
    return out


@kind_cfg
def test_attn_is_deterministic_placement_free_and_within_the_bound(hip, stream, ws, random_cases, kind, cfg):
    """Random normal operands.  Every split count is inside the derived bound of the fp64 reference (they need not be
    equal to each other); two runs are bit-equal and a run on a stream masked to CUs 0 .. 63 is bit-equal to them."""
    masked = hip.Stream(0, hip.mask_words(range(0, 64)))
    try:
        assert masked.mask(8)[:2] == [0xFFFFFFFF, 0xFFFFFFFF]
        for case in ac.RANDOM_CASES:
            p, ref, bound = random_cases[kind, case[0]]
            d = Dev(p)
            for splits in _splits_of(cfg):
                out = []
                for s in (stream, stream, masked):
                    o = d.run(hip, s, ws, cfg, splits)
                    s.sync()
                    out.append(o.cpu())
                what = f"{kind} cfg {cfg} splits {splits} case {case[0]}"
                assert torch.equal(ac.bits(out[0]), ac.bits(out[1])), f"{what}: two runs differ"
                assert torch.equal(ac.bits(out[0]), ac.bits(out[2])), f"{what}: the masked stream's result differs"
                err = np.abs(out[0].double().numpy() - ref)
                assert not np.isnan(err).any(), f"{what}: NaN in the result"
                worst = float((err / np.maximum(bound, 1e-300)).max())
                print(f"{what}: largest error / bound = {worst:.4f}")
                assert bool((err <= bound).all()), f"{what}: error up to {worst:.3f} of the bound"
    finally:
        masked.destroy()


# ---- 6a. windows: every token counted once ----------------------------------------------------------------------------

KIND_ROW = [(kind, cfg) for kind in ac.KINDS for cfg in ac.CFGS]
kind_row = pytest.mark.parametrize("kind,cfg", KIND_ROW, ids=[f"{k}-{c}" for k, c in KIND_ROW])


@kind_cfg
def test_attn_counts_every_token_once_at_every_wave_and_split_boundary(hip, stream, ws, kind, cfg):
    """The lengths of test 2 as window cases (``attn_decode_cases.window_problem``): every head weighs a window of
    s tokens equally and the windows cover the sequence, so a tile, a half or a token that the ring, the drain or a
    split's range takes twice or leaves out changes l and a column of some head's row.  A selection case cannot see
    that: its weights are 0 or 1 (``tests/test_attn_decode_cases.py`` shows both)."""
    for splits in _splits_of(cfg):
        runs = [(name, p, Dev(p).run(hip, stream, ws, cfg, splits))
                for name, p in ac.window_split_cases(kind, cfg, splits or 1)]
        stream.sync()
        for name, p, o in runs:
            ac.assert_bits_equal(o, p.want, f"{kind} cfg {cfg}, splits {splits}, {name}")


@kind_cfg
def test_attn_windows_with_every_score_far_below_zero(hip, stream, ws, kind, cfg):
    """-261 inside a window and -522 outside it: a running maximum that starts at a finite value stays there, and
    every probability underflows."""
    _check(hip, stream, ws, ac.negative_cases(kind), cfg, f"{kind} cfg {cfg}")


@kind_cfg
def test_attn_other_head_counts_page_sizes_and_groups(hip, stream, ws, kind, cfg):
    """Hkv of 1, 3 and 8, pages of 32, 48, 128 and 256 tokens, G of 3, 7 and 12, at lengths around a tile and a page
    boundary: window cases, and selection cases for the addressing."""
    _check(hip, stream, ws, ac.other_shape_cases(kind), cfg, f"{kind} cfg {cfg}")


@kind_row
def test_attn_counts_every_token_once_at_16_to_64_splits(hip, stream, ws, kind, cfg):
    """``MORE_SPLITS`` (16, 32, 37 and 64) through ``_launch_cfg``: 1, W + 1 and 2 F W + 1 tiles per split, and a
    split without a token, with one token and with one full tile.  Every cut lies inside some head's window, so every
    split's partial enters some head's row with weight exactly 1."""
    for splits in ac.MORE_SPLITS:
        for name, p in ac.more_split_cases(kind, cfg, splits):
            o = Dev(p).run(hip, stream, ws, cfg, splits)
            stream.sync()
            ac.assert_bits_equal(o, p.want, f"{kind} cfg {cfg}, splits {splits}, {name}")


@pytest.fixture(scope="module")
def random_more():
    """``{kind: (problem, fp64 reference, bound)}`` of ``RANDOM_MORE``, computed once."""
    out = {}
    for kind in ac.KINDS:
        p = ac.random_problem(kind, *ac.RANDOM_MORE)
        out[kind] = (p, ac.reference(p), ac.error_bound(p)[0])
    return out


@kind_row
def test_attn_merges_16_32_and_64_splits_within_the_bound(hip, stream, ws, random_more, kind, cfg):
    """Random normal operands, 4096 and 45 tokens: the splits' partials are merged with graded weights (a window
    case's are 0 or 1), inside the derived bound of the fp64 reference."""
    p, ref, bound = random_more[kind]
    d = Dev(p)
    for splits in ac.RANDOM_MORE_SPLITS:
        o = d.run(hip, stream, ws, cfg, splits)
        stream.sync()
        what = f"{kind} cfg {cfg} splits {splits} case {ac.RANDOM_MORE[0]}"
        err = np.abs(o.cpu().double().numpy() - ref)
        assert not np.isnan(err).any(), f"{what}: NaN in the result"
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"{what}: largest error / bound = {worst:.4f}")
        assert bool((err <= bound).all()), f"{what}: error up to {worst:.3f} of the bound"


# ---- 6b. the dispatcher -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dispatch_problems():
    """``get(i)``: the cases of row i of ``DISPATCH_SHAPES`` for both cache types; one row is kept at a time."""
    kept = {}

    def get(i):
        if i not in kept:
            kept.clear()
            kept[i] = ac.dispatch_cases(ac.DISPATCH_SHAPES[i])
        return kept[i]

    return get


SHAPE_KIND = [(i, kind) for i in range(len(ac.DISPATCH_SHAPES)) for kind in ac.KINDS]


@pytest.mark.parametrize("shape,kind", SHAPE_KIND,
                         ids=[f"{ac.DISPATCH_SHAPES[i][-1]}-splits-{i}-{k}" for i, k in SHAPE_KIND])
def test_attn_dispatches_the_split_count_of_pick(hip, stream, ws, dispatch_problems, shape, kind):
    """``gsx_decode_attn`` at the smallest shapes where each rule of ``attn_pick`` decides (4, 8, 32, 37 and 64 splits;
    ``DISPATCH_SHAPES``): a window case and a selection case with targets at the cuts, exact.  The split count is read
    from the NaN-prefilled workspace: B * Hq * splits partials of 130 floats are written (a split without a token
    writes zeros and (-inf, 0)), and nothing behind them."""
    splits = ac.DISPATCH_SHAPES[shape][-1]
    for what, p in dispatch_problems(shape)[kind]:
        assert ac.pick(p.b * p.hkv, p.max_seq_len) == splits
        allowed = hip.decode_attn_workspace_bytes(p.b, p.hq, ac.D, p.page, p.max_seq_len) // 4
        written = p.b * p.hq * splits * (ac.D + 2)
        assert written <= allowed and allowed + written <= ws.numel()
        ws[allowed:allowed + written].fill_(NAN)  # Dev.run fills what the query allows; and behind it, for this test
        o = Dev(p).run(hip, stream, ws, None)
        stream.sync()
        ac.assert_bits_equal(o, p.want, f"{kind}, {what}")
        nan = torch.isnan(ws[:allowed + written])
        assert not bool(nan[:written].any()), f"{kind}, {what}: fewer than {splits} splits were dispatched"
        assert bool(nan[written:].all()), f"{kind}, {what}: more than {splits} splits were dispatched"


# ---- 6c. the contract's clamps, and the e4m3 codes --------------------------------------------------------------------

@kind_cfg
def test_attn_clamps_a_page_index_above_num_pages(hip, stream, ws, kind, cfg):
    """A block-table entry of a page in use is ``num_pages + 1``; its data lies in page ``num_pages - 1``, where the
    unsigned minimum of the contract sends it, and the caches go on for three pages of poison.  (``seq_lens`` below
    zero are among the table cases of test 3.)  Negative page indices are not tested: without the clamp they would
    leave the allocation."""
    p = ac.page_clamp_problem(kind)
    assert int(p.block_table.max()) == p.num_pages + 1 and p.k_cache.shape[0] == p.num_pages + 3
    _check(hip, stream, ws, [("a page index of num_pages + 1", p)], cfg, f"{kind} cfg {cfg}")


@pytest.mark.parametrize("cfg", ac.ALL, ids=lambda c: "dispatch" if c is None else str(c))
def test_attn_converts_every_e4m3_code_of_v(hip, stream, ws, cfg):
    """The 32 target rows hold each of the 254 e4m3 codes that are no NaN at each byte position of a 16-B chunk:
    O is the value times ``v_scale``, exact, subnormals and 448 included; -0 comes out as a zero.  K goes through the
    same conversion function, and the random cases test where its operands land."""
    p, _ = ac.fp8_codes_problem()
    d = Dev(p)
    for splits in _splits_of(cfg):
        o = d.run(hip, stream, ws, cfg, splits)
        stream.sync()
        ac.assert_bits_equal(o, p.want, f"cfg {cfg} splits {splits}", zeros_by_value=True)


# ---- 7. the timing entry point ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ac.KINDS)
def test_time_decode_attn_leaves_the_result_in_o(hip, stream, ws, kind):
    """At 2100 tokens the dispatcher splits (66 tiles: two splits of 8 waves with 4 tiles each; both sides of the cut
    are targets): a workspace that is too small is refused before anything runs."""
    cut = ac.split_cuts(2100, 2)
    assert cut == [33 * ac.TILE]
    p = ac.selection_problem(kind, 8, 16, [2100, 3, 0], cuts=[cut, (), ()], **ac.fp8_scales(kind))
    q, k, v, bt, sl = Dev(p).t
    o = torch.full((p.b, p.hq, ac.D), NAN, device="cuda", dtype=torch.bfloat16)
    ws[:hip.decode_attn_workspace_bytes(p.b, p.hq, ac.D, p.page, p.max_seq_len) // 4].fill_(NAN)
    torch.cuda.synchronize()
    args = (stream, kind, q.data_ptr(), k.data_ptr(), v.data_ptr(), bt.data_ptr(), sl.data_ptr(), o.data_ptr(), p.b,
            p.hq, p.hkv, ac.D, p.page, p.num_pages, p.table_stride, p.max_seq_len, p.scale)
    with pytest.raises(hip.HipError, match="gsx_decode_attn: workspace too small"):
        hip.time_decode_attn(*args, 3, p.k_scale, p.v_scale, ws.data_ptr(), 16)
    assert bool(torch.isnan(o).all())
    ms = hip.time_decode_attn(*args, 3, p.k_scale, p.v_scale, ws.data_ptr(), ws.numel() * 4)
    stream.sync()
    assert ms > 0, ms
    ac.assert_bits_equal(o, p.want, f"time_decode_attn, {kind}")


# ---- 8. the workload, end to end --------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ac.KINDS)
def test_workload_attn_end_to_end(dtype):
    """``gsxtools.workload --workload attn``: a ring of at least two layers of KV cache, a positive rate of KV bytes,
    and the library's kernel named as the one that ran."""
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "gsxtools.workload", "--workload", "attn", "--kv-dtype", dtype,
                        "--batch", "4", "--context", "512", "--kv-gib", "0.125", "--iters", "20", "--json"],
                       env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["workload"] == "attn" and out["batch"] == 4 and out["kv_dtype"] == dtype and out["context"] == 512
    assert out["layers"] >= 2 and out["tbps"] > 0 and out["tokens_per_s"] > 0 and out["iters"] >= 20
    assert out["kernel"] == "gsx" and out["kernels_lib"].endswith("libgsx_kernels.so")
    per_layer = 2 * 4 * 512 * 8 * ac.D * {"bf16": 2, "fp8": 1}[dtype]
    assert out["layers"] * per_layer >= 0.125 * (1 << 30) or out["layers"] == 2
