"""The block-scaled fp8 grouped expert GEMM of MoE decode (native/kernels/moe_fp8_block.hip) on a real MI355X.

The reference is the fp64 sum of the scaled block products of every (row of A, expert).  With power-of-two scales on
``gemm_fp8_cases``' exact operands no order of summation can round and the comparison is on the raw 16 bits; with
general scales every element lies inside the interval the contract's own roundings allow, and a W = 4 configuration
has the skinny kernel's bits.  Every case starts from a C full of NaN.
"""
import functools
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import gemm_cases as gc  # noqa: E402
from tests import gemm_fp8_cases as fc  # noqa: E402
from tests import moe_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
NAN = float("nan")
E, N, PAD, SPARE = 8, 192, 3, 2  # N: three 64-column strips, scale_b's second block row covers 64 columns
CFGS = {0: ("16/4w-f8", 16, 4, 8), 1: ("16/8w-f4", 16, 8, 4), 2: ("32/4w-f4", 32, 4, 4), 3: ("32/8w-f2", 32, 8, 2),
        4: ("64/4w-f2", 64, 4, 2)}


def _picked(n, k):
    """mfb_pick() of moe_fp8_block.hip."""
    return 3 if k // 128 >= 32 else 2 if k // 128 >= 8 else 4


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    from gpushare_scheduler_extender_amd.ops import hip as h

    assert h.moe_gemm_fp8_block_cfgs() == CFGS
    return h


@pytest.fixture(scope="module")
def stream(hip):
    s = hip.Stream(0)
    yield s
    s.destroy()


def _table(a, b, sa, sb, n):
    """``(sum_g p_g sa sb, sum_g |p|_g |sa sb|)`` in fp64 of every row of ``a`` against every expert: ``b`` is
    ``[experts * n][K]``, ``sb`` ``[experts][ceil(n / 128)][K / 128]``; column ``x n + j`` is expert x's column j."""
    a, b, sa = a.double(), b.double(), sa.double()
    cols = sb.double().repeat_interleave(128, dim=1)[:, :n].reshape(b.shape[0], -1)  # [experts * n][K / 128]
    exact = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float64)
    mag = torch.zeros_like(exact)
    for g in range(a.shape[1] // 128):
        ag, bg = a[:, 128 * g:128 * g + 128], b[:, 128 * g:128 * g + 128]
        s = sa[:, g, None] * cols[None, :, g]
        exact += (ag @ bg.t()) * s
        mag += (ag.abs() @ bg.abs().t()) * s.abs()
    return exact, mag


@functools.lru_cache(maxsize=None)
def _exact(tiles):
    """128 rows of A (row r is row r % 16 of the exact case) against 8 experts of 192 columns, scales ``2^e`` with
    ``e`` from {-1, 0, 1} drawn independently per (row, g) and per (expert, nb, g), and the bf16 table of every row
    against every expert; asserts on the CPU that no order of summation can round."""
    k = 128 * tiles
    a16, b, _ = fc.exact_case(16, E * N, k)
    a = a16[torch.arange(mc.MAX_PAIRS) % 16].contiguous()
    rng = np.random.default_rng(7)
    sa = torch.from_numpy(2.0 ** rng.integers(-1, 2, (mc.MAX_PAIRS, tiles))).float()
    sb = torch.from_numpy(2.0 ** rng.integers(-1, 2, (E, (N + 127) // 128, tiles))).float()
    exact, mag = _table(a, b, sa, sb, N)
    assert float(mag.max()) < 2 ** 12 and bool(((exact * 2 ** 10) % 1 == 0).all())
    assert torch.equal(exact.float().double(), exact)
    return a, b, sa, sb, exact.float().bfloat16()


def _wanted(table, ids, a_div):
    """Row p of C: row ``p // a_div`` of the table, the columns of pair p's expert."""
    flat = ids.reshape(-1)
    return torch.stack([table[p // a_div, int(x) * N:(int(x) + 1) * N] for p, x in enumerate(flat)])


def _padded_scales(sa):
    """``sa`` on the device with rows ``g + PAD`` apart, NaN in the padding and NaN right behind the last row."""
    rows, g = sa.shape
    body = torch.full((rows, g + PAD), NAN)
    body[:, :g] = sa
    return torch.cat([body.flatten()[:(rows - 1) * (g + PAD) + g], torch.full((1024,), NAN)]).cuda()


def _launch(hip, s, a, a_div, b, c, plan, m, topk, sa, sa_stride, sb, cfg=None, timed=False, e=E, n=N):
    args = (a.data_ptr(), a_div, b.data_ptr(), c.data_ptr(), plan.data_ptr(), m, topk, e, n, b.shape[-1])
    tail = dict(scale_a=sa.data_ptr(), sa_stride=sa_stride, scale_b=sb.data_ptr())
    torch.cuda.synchronize()
    if timed:
        assert hip.time_moe_gemm_fp8_block(s, *args, 2, **tail) > 0
    elif cfg is None:
        hip.moe_gemm_fp8_block_nt(s, *args, **tail)
    else:
        hip.moe_gemm_fp8_block_nt_cfg(s, *args, cfg, **tail)
    s.sync()


def _run_exact(hip, stream, cfg, tiles, ids, a_div, plan=None, b=None, sb=None):
    """One launch on the exact case: A and scale_a cut to ``ceil(P / a_div)`` rows with NaN behind them, C with SPARE
    rows more.  Returns ``(C on the host, want[P][N])``."""
    a, b0, sa, sb0, table = _exact(tiles)
    m, topk = ids.shape
    rows = -(-m * topk // a_div)
    keep, da = fc.banded(a[:rows], "cuda")
    c = torch.full((m * topk + SPARE, N), NAN, device="cuda", dtype=torch.bfloat16)
    dplan = torch.from_numpy(mc.plan_of(ids, E) if plan is None else plan).cuda()
    _launch(hip, stream, da, a_div, (b0 if b is None else b).cuda(), c, dplan, m, topk, _padded_scales(sa[:rows]),
            tiles + PAD, (sb0 if sb is None else sb).cuda(), cfg)
    del keep
    return c.cpu(), _wanted(table, ids, a_div)


@pytest.mark.parametrize("cfg", list(CFGS))
def test_exact_at_every_routing_and_tile_count(hip, stream, cfg):
    """1, W - 1, W + 1, 2 F W and 67 K-tiles (waves without a tile, a ragged round, the steady loop first entered by
    every wave, the ring wrapped with a ragged tail; 67 is as far as the CPU assertion holds with room to spare), every
    routing of ``moe_cases.routings(8)``, both projections."""
    _, _, w, f = CFGS[cfg]
    for tiles in sorted({1, w - 1, w + 1, 2 * f * w, 67}):
        for name, ids in mc.routings(E):
            for a_div in (ids.shape[1], 1):
                got, want = _run_exact(hip, stream, cfg, tiles, ids, a_div)
                fc.assert_bits_equal(got[:-SPARE], want, f"cfg {cfg}, {tiles} K-tiles, {name}, a_div {a_div}")
                assert bool(got[-SPARE:].isnan().all()), "rows of C without a pair were written"


@pytest.mark.parametrize("cfg", list(CFGS))
def test_inactive_experts_are_never_read(hip, stream, cfg):
    """Every expert the routing does not hit holds e4m3 NaN and NaN scales."""
    tiles = 9
    _, b, _, sb, _ = _exact(tiles)
    for name, ids in mc.routings(E):
        idle = [x for x in range(E) if x not in set(ids.reshape(-1).tolist())]
        pb, psb = b.view(torch.uint8).clone().view(E, N, -1), sb.clone()
        pb[idle], psb[idle] = fc.FP8_NAN, NAN
        got, want = _run_exact(hip, stream, cfg, tiles, ids, 1, b=pb.view(E * N, -1).view(fc.FP8), sb=psb)
        fc.assert_bits_equal(got[:-SPARE], want, f"cfg {cfg}, {name}")


def _valid_pairs(plan, pairs):
    """The pairs the kernel's rules let a plan name, by slot: gsx_kernels.h's list."""
    n_active, _, _, expert, begin, count, rows = mc.plan_fields(plan)
    out = []
    for s in range(min(max(n_active, 0), mc.MAX_PAIRS)):
        if 0 <= expert[s] < E:
            idx = [int(begin[s]) + r for r in range(min(max(int(count[s]), 0), 16))]
            out += [(int(rows[i]), int(expert[s])) for i in idx if 0 <= i < mc.MAX_PAIRS and 0 <= rows[i] < pairs]
    return out


@pytest.mark.parametrize("flaw", ["expert outside [0, E)", "count above 16", "rows index outside", "pair >= P"])
def test_hand_written_plans_break_one_rule_each(hip, stream, flaw):
    """Exactly the pairs that stay valid are written: C has spare rows and NaN around it."""
    tiles, cfg = 5, 2
    ids = np.full((16, 1), 5, np.int32) if flaw == "count above 16" else mc.routings(E)[4][1]  # random M=5 topk=2
    pairs = ids.size
    plan = mc.plan_of(ids, E)
    _, _, _, expert, begin, count, rows = mc.plan_fields(plan)
    if flaw == "expert outside [0, E)":
        expert[0], expert[1] = E, -2
    elif flaw == "count above 16":
        count[0], rows[16:40] = 100, np.arange(24) % 16
    elif flaw == "rows index outside":
        s = int(np.argmax(count))  # its first pair moves to rows[127]; its others would be rows[128 ..]
        rows[127], begin[s] = rows[begin[s]], 127
    else:
        rows[1], rows[pairs - 1] = pairs, 1 << 30
    got, _ = _run_exact(hip, stream, cfg, tiles, ids, 1, plan=plan)
    valid = _valid_pairs(plan, pairs)
    assert 0 < len(valid) < pairs or flaw == "count above 16"
    expected = torch.full_like(got, NAN)
    table = _exact(tiles)[4]
    for p, x in valid:
        expected[p] = table[p, x * N:(x + 1) * N]
    fc.assert_bits_equal(got, expected, flaw)


@functools.lru_cache(maxsize=None)
def _general():
    """7 tokens x 3 of 8 experts, N = 192, K = 3072: randn rows for both projections (the first 7 and all 21),
    experts block-quantised in torch."""
    m, topk, k = 7, 3, 3072
    g = torch.Generator().manual_seed(11)
    x = torch.randn(m * topk, k, generator=g).bfloat16()
    nb = (N + 127) // 128
    w = torch.zeros(E, nb * 128, k)
    w[:, :N] = torch.randn(E, N, k, generator=g)
    blocks = w.view(E, nb, 128, k // 128, 128)
    sb = blocks.abs().amax(dim=(2, 4)) / 448.0
    b = (blocks / sb[:, :, None, :, None]).reshape(E, nb * 128, k)[:, :N].reshape(E * N, k).to(fc.FP8)
    ids = np.stack([np.random.default_rng(13 + i).permutation(E)[:topk] for i in range(m)]).astype(np.int32)
    return x, b.contiguous(), sb.contiguous(), ids


@pytest.mark.parametrize("cfg", list(CFGS))
def test_general_scales_from_the_quantiser(hip, stream, cfg):
    """Every element lies between ``bf16(exact - err)`` and ``bf16(exact + err)``, ``exact`` the fp64 product of the
    dequantised operands and ``err = (127 + K / 128 + 2) 2^-24 sum |a b s|`` (the skinny test's bound: 127 for the
    MFMA's 128-term sum in any order, K / 128 + 2 for the contract's own roundings).  A W = 4 configuration has, for
    every active expert, the bits of the skinny kernel at splits = 1 on that expert's rows gathered contiguously."""
    x, b, sb, ids = _general()
    (m, topk), k = ids.shape, x.shape[1]
    pairs = m * topk
    dx, db, dsb, plan = x.cuda(), b.cuda(), sb.cuda(), torch.from_numpy(mc.plan_of(ids, E)).cuda()
    q = torch.empty(pairs, k, dtype=torch.uint8, device="cuda")
    sa = torch.empty(pairs, k // 128, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    hip.quant_fp8_block(stream, dx.data_ptr(), k, q.data_ptr(), k, sa.data_ptr(), k // 128, pairs, k)
    stream.sync()
    exact, mag = _table(q.cpu().view(fc.FP8), b, sa.cpu(), sb, N)
    err = (127 + k // 128 + 2) * 2.0 ** -24 * mag

    def product(a_div, **kw):
        c = torch.full((pairs, N), NAN, device="cuda", dtype=torch.bfloat16)
        _launch(hip, stream, q, a_div, db, c, plan, m, topk, sa, k // 128, dsb, **kw)
        return c.cpu()

    for a_div in (topk, 1):
        got = product(a_div, cfg=cfg)
        lo, hi = (_wanted((exact + d).float().bfloat16().double(), ids, a_div) for d in (-err, err))
        assert bool(((got.double() >= lo) & (got.double() <= hi)).all())
        assert torch.equal(gc.bits(product(a_div, cfg=cfg)), gc.bits(got)), "the same call twice"
        if cfg == _picked(N, k):
            assert torch.equal(gc.bits(product(a_div)), gc.bits(got)), "the dispatcher's choice"
            assert torch.equal(gc.bits(product(a_div, timed=True)), gc.bits(got)), "the timed call"
        if CFGS[cfg][2] != 4:
            continue
        for x_ in sorted(set(ids.reshape(-1).tolist())):
            mine = np.flatnonzero(ids.reshape(-1) == x_)
            src = torch.from_numpy(mine // a_div).cuda()
            c = torch.full((len(mine), N), NAN, device="cuda", dtype=torch.bfloat16)
            qa, qs = q[src].contiguous(), sa[src].contiguous()
            torch.cuda.synchronize()
            hip.skinny_gemm_fp8_block_nt_cfg(stream, qa.data_ptr(), db.data_ptr() + x_ * N * k, c.data_ptr(), len(mine),
                                             N, k, 0, 1, scale_a=qs.data_ptr(), sa_stride=k // 128,
                                             scale_b=dsb[x_].data_ptr(), workspace=0, workspace_bytes=0)
            stream.sync()
            assert torch.equal(gc.bits(c.cpu()), gc.bits(got[mine])), f"expert {x_}, a_div {a_div}: the skinny bits"


REFUSALS = [  # (what to change, the text)
    (dict(m=17), "need 1 <= M <= 16"), (dict(k=192), "need N%64==0, K%128==0"), (dict(n=96), "need N%64==0, K%128==0"),
    (dict(sa_stride=0), "need sa_stride >= K/128"), (dict(a_off=8), "operands must be 16-B aligned"),
    (dict(c_is_a=True), "C must not overlap A, B, plan, scale_a or scale_b"), (dict(cfg=len(CFGS)), "unknown config")]


@pytest.mark.parametrize("change,text", REFUSALS)
def test_refusals(hip, stream, change, text):
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    sc = torch.ones(4096, device="cuda")
    plan = torch.from_numpy(mc.plan_of(np.zeros((1, 1), np.int32), E)).cuda()
    v = dict(m=1, n=64, k=128, sa_stride=1, a_off=0, c_is_a=False, cfg=0) | change
    a = buf.data_ptr() + v["a_off"]
    c = a if v["c_is_a"] else buf.data_ptr() + (1 << 19)
    with pytest.raises(hip.HipError, match="gsx_moe_gemm_fp8_block_nt_launch_cfg: " + text):
        hip.moe_gemm_fp8_block_nt_cfg(stream, a, 1, buf.data_ptr() + 4096, c, plan.data_ptr(), v["m"], 1, E, v["n"],
                                      v["k"], v["cfg"], sc.data_ptr(), v["sa_stride"], sc.data_ptr() + 1024)


def test_workload_runs_the_moe_mlp_on_block_scaled_experts():
    main = str(ROOT / "samples" / "workload" / "main.py")
    r = subprocess.run([sys.executable, main, "--workload", "moe", "--dtype", "fp8-block", "--kernel", "gsx",
                        "--experts", "16", "--experts-active", "2", "--batch", "3", "--size", "256", "--ffn", "128",
                        "--iters", "2", "--json"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["workload"] == "moe" and out["dtype"] == "fp8-block" and np.isfinite(out["tbps"]) and out["tbps"] > 0
    assert all(2 <= h <= 6 for h in out["n_active"]) and out["activations_finite"], out
