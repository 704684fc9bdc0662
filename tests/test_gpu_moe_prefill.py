"""The MoE prefill kernels (native/kernels/moe_prefill.hip) on a real MI355X: the router against the decode router's
twin, the tile plan against its definition in NumPy, the grouped 128x128 GEMM bit for bit against the fp64 product on
exact operands and against the dense ``128x128/4w`` configuration on random ones, the combine against its twin, and
the ``prefill-moe`` workload end to end."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import gemm_cases as gc  # noqa: E402
from tests import moe_cases as mo  # noqa: E402
from tests import sample_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
BM = 128


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    from gpushare_scheduler_extender_amd.ops import hip as h

    assert h.moe_prefill_gemm_cfgs() == {0: ("128x128/4w-gather", 128, 128, 4)}
    return h


@pytest.fixture(scope="module")
def stream(hip):
    s = hip.Stream(0)
    yield s
    s.destroy()


def dev(x: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def plan_ref(ids: np.ndarray, e: int) -> np.ndarray:
    """The header's definition: experts in ascending order, each its pairs in ascending order over ceil(c / 128)
    tiles, -1 everywhere else; an id outside [0, e) is in no tile."""
    flat = ids.reshape(-1)
    p = flat.size
    t_max = (p + min(e, p) * (BM - 1)) // BM
    tile_expert, rows, t = np.full(t_max, -1, np.int32), np.full(t_max * BM, -1, np.int32), 0
    for x in range(e):
        mine = np.flatnonzero(flat == x)
        n = -(-len(mine) // BM)
        tile_expert[t:t + n] = x
        rows[t * BM:t * BM + len(mine)] = mine
        t += n
    return np.concatenate([np.array([t, p, e, BM], np.int32), tile_expert, rows])


# ---- 1. the router -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,e,topk,pad", [(1, 8, 1, 0), (17, 128, 8, 8), (300, 1024, 2, 0)])
def test_route_is_the_decode_routers_twin_row_by_row(hip, stream, m, e, topk, pad):
    """Logits keep two mantissa bits, so every row has ties: ids equal ``moe_cases.select`` (the lowest index first),
    weights lie within the header's bound of the fp64 softmax; the NaN padding of a wider stride is never picked."""
    bits = mo.random_logits(np.random.default_rng(5000 + m), m, e) & np.uint16(0xFFE0)
    logits = np.full((m, e + pad), mo.NAN, np.uint16)
    logits[:, :e] = bits
    lg, ids, w = dev(logits), dev(np.full((m, topk), -7, np.int32)), dev(np.full((m, topk), np.nan, np.float32))
    torch.cuda.synchronize()
    assert hip.time_moe_prefill_route(stream, lg.data_ptr(), e + pad, ids.data_ptr(), w.data_ptr(), m, e, topk, 2) > 0
    stream.sync()
    want = mo.select(bits, topk)
    assert np.array_equal(ids.cpu().numpy(), want)
    w64 = mo.weights64(bits, want)
    err = np.abs(w.cpu().numpy().astype(np.float64) - w64)
    assert (err <= mo.weight_bound(bits, want, w64)).all(), err.max()


# ---- 2. the plan -----------------------------------------------------------------------------------------------------

def _routings():
    rng = np.random.default_rng(5100)
    alt = lambda a, b, n: np.where(np.arange(n) % 2 == 0, a, b).astype(np.int32).reshape(-1, 1)  # noqa: E731
    odd = np.full((128, 1), 4, np.int32)
    odd[77] = 2
    bad = rng.integers(0, 8, (150, 2)).astype(np.int32)
    bad[40, 1], bad[99, 0] = 8, -1
    return {"300 on one expert": (np.full((300, 1), 5, np.int32), 8), "counts of 128": (alt(2, 6, 256), 8),
            "counts of 129": (alt(1, 3, 258), 8), "counts of 1 and 127": (odd, 8),
            "E = 1024 > P": (rng.permutation(1024)[:10].reshape(5, 2).astype(np.int32), 1024),
            "ids outside [0, E)": (bad, 8), "two blocks of pairs": (rng.integers(0, 16, (700, 2)).astype(np.int32), 16)}


@pytest.mark.parametrize("name", list(_routings()))
def test_plan_is_the_definition_whole(hip, stream, name):
    """Header, tile_expert and rows, unused tiles and rows included; the timed form runs it three times over the same
    scratch and leaves the same plan."""
    ids, e = _routings()[name]
    m, topk = ids.shape
    n = hip.moe_prefill_plan_ints(m, topk, e)
    want = plan_ref(ids, e)
    assert n == len(want)
    if name == "300 on one expert":
        assert want[0] == 3 and (want[4 + (n - 4) // 129 + 2 * BM:][:BM] >= 0).sum() == 44
    ids_d, plan = dev(ids), dev(np.full(n + 16, -7, np.int32))
    wsb = hip.moe_prefill_workspace_bytes(m, topk, e)
    ws = torch.empty(wsb // 4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert hip.time_moe_prefill_plan(stream, ids_d.data_ptr(), plan.data_ptr(), m, topk, e, ws.data_ptr(), wsb, 3) > 0
    stream.sync()
    got = plan.cpu().numpy()
    assert np.array_equal(got[:n], want), np.flatnonzero(got[:n] != want)[:8]
    assert (got[n:] == -7).all(), "written past the plan"


# ---- 3. the grouped GEMM ---------------------------------------------------------------------------------------------

def _gemm_ids() -> np.ndarray:
    """M = 193, topk = 2, E = 8 with 129, 128, 127, 1 and 1 pairs on experts 0, 1, 2, 3 and 5, a token's two experts
    distinct, tokens shuffled.  Counts of 129, 128, 127 and 1 are 385 pairs, more than M = 160 tokens of two have: 193
    is the fewest tokens with topk = 2 that hold them (the odd pair goes to a fifth expert)."""
    lab = np.repeat(np.array([0, 1, 2, 3, 5]), [129, 128, 127, 1, 1]).astype(np.int32)
    ids = np.stack([lab[:193], lab[193:]], 1)
    assert (ids[:, 0] != ids[:, 1]).all()
    return ids[np.random.default_rng(5200).permutation(193)]


def _run_gemm(hip, stream, a, a_div, b, plan, ids, n, k, timed=False):
    m, topk = ids.shape
    whole, c = gc.banded(torch.full((m * topk, n), float("nan"), dtype=torch.bfloat16), gc.C_BAND, "cuda")
    a_d, b_d, plan_d = a.cuda(), b.cuda(), dev(plan)
    torch.cuda.synchronize()
    args = (stream, a_d.data_ptr(), a_div, b_d.data_ptr(), c.data_ptr(), plan_d.data_ptr(), m, topk, 8, n, k)
    if timed:
        assert hip.time_moe_prefill_gemm(*args, 2) > 0
    else:
        hip.moe_prefill_gemm_nt_cfg(*args, 0)
    stream.sync()
    for band in gc.bands_of(whole, c.numel()):
        assert bool((band == gc.C_BAND - 0x10000).all()), "a guard band of C was written"
    return c.cpu()


@pytest.mark.parametrize("n", [128, 256])
@pytest.mark.parametrize("k", [64, 192])
@pytest.mark.parametrize("up", [True, False], ids=["a_div=topk", "a_div=1"])
def test_grouped_gemm_exact(hip, stream, n, k, up):
    """Exact operands: every pair's row is the fp64 product against its expert, rounded once.  Then the same launch
    on a plan that claims T_max + 5 tiles and lists pair P: that entry's own pair stays NaN, nothing else changes."""
    ids = _gemm_ids()
    m, topk = ids.shape
    p, a_div = m * topk, topk if up else 1
    a, b = gc.exact_operands(p // a_div, 8 * n, k)
    full = gc.reference(a, b)
    want = torch.stack([full[q // a_div, x * n:(x + 1) * n] for q, x in enumerate(ids.reshape(-1).tolist())])
    plan = plan_ref(ids, 8)
    gc.assert_bits_equal(_run_gemm(hip, stream, a, a_div, b, plan, ids, n, k, timed=n == 256), want, "the plan")
    t_max = (p + 8 * (BM - 1)) // BM
    at = 4 + t_max + 5  # a row of tile 0
    lost, plan[0], plan[at] = int(plan[at]), t_max + 5, p
    got = _run_gemm(hip, stream, a, a_div, b, plan, ids, n, k)
    assert bool(got[lost].isnan().all()), "the pair whose entry was overwritten was stored"
    keep = torch.arange(p) != lost
    gc.assert_bits_equal(got[keep], want[keep], "n_tiles = T_max + 5, a row of P")


def test_grouped_gemm_random_operands_have_the_dense_kernels_bits(hip, stream):
    """The summation order: per expert, its gathered rows padded to 128 through the dense ``128x128/4w``."""
    ids, n, k = _gemm_ids(), 256, 192
    m, topk = ids.shape
    g = torch.Generator().manual_seed(53)
    a, b = torch.randn(m, k, generator=g).bfloat16(), torch.randn(8 * n, k, generator=g).bfloat16()
    got = _run_gemm(hip, stream, a, topk, b, plan_ref(ids, 8), ids, n, k)
    dense = {name: i for i, name in hip.gemm_cfgs().items()}["128x128/4w"]
    flat = ids.reshape(-1)
    for x in np.unique(flat):
        prs = np.flatnonzero(flat == x)
        rows = -(-len(prs) // BM) * BM
        ga = torch.zeros(rows, k, dtype=torch.bfloat16)
        ga[:len(prs)] = a[torch.from_numpy(prs // topk)]
        ga, xb, cs = ga.cuda(), b[x * n:(x + 1) * n].cuda(), torch.empty(rows, n, dtype=torch.bfloat16, device="cuda")
        torch.cuda.synchronize()
        hip.gemm_bf16_nt_cfg(stream, ga.data_ptr(), xb.data_ptr(), cs.data_ptr(), rows, n, k, dense)
        stream.sync()
        gc.assert_bits_equal(got[torch.from_numpy(prs)], cs[:len(prs)].cpu(), f"expert {x}")


# ---- 4. the combine --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("topk", [1, 2, 8])
@pytest.mark.parametrize("h", [8, 264])
def test_combine_is_the_twin_bit_for_bit(hip, stream, topk, h):
    m, ys, os_ = 300, h + 8, h + 24
    rng = np.random.default_rng(5300 + topk)
    y = np.full((m * topk, ys), mo.NAN, np.uint16)
    y[:, :h] = sc.bf16_bits(rng.normal(0, 1, (m * topk, h)).astype(np.float32))
    w = rng.random((m, topk)).astype(np.float32)
    w /= w.sum(1, keepdims=True)
    y_d, w_d, out = dev(y), dev(w), dev(np.full((m, os_), 0x5A5A, np.uint16))
    torch.cuda.synchronize()
    hip.moe_prefill_combine(stream, y_d.data_ptr(), ys, w_d.data_ptr(), out.data_ptr(), os_, m, topk, h)
    assert hip.time_moe_prefill_combine(stream, y_d.data_ptr(), ys, w_d.data_ptr(), out.data_ptr(), os_, m, topk, h, 2) > 0
    stream.sync()
    got = out.cpu().numpy()
    assert (got[:, h:] == 0x5A5A).all(), "the padding of out was written"
    assert np.array_equal(got[:, :h], mo.combine(y[:, :h], w))


# ---- 5. the workload -------------------------------------------------------------------------------------------------

def test_workload_prefill_moe_end_to_end():
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "gsxtools.workload", "--workload", "prefill-moe", "--experts", "128",
                        "--experts-active", "2", "--heads", "2", "--kv-heads", "1", "--ffn", "64", "--context", "128",
                        "--chunk", "128", "--batch", "1", "--iters", "2", "--json", "--weights-gib", "0.01", "--kv-gib",
                        "0.0005"], env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["workload"] == "prefill-moe" and out["experts"] == 128 and out["experts_active"] == 2
    assert out["activations_finite"] is True and out["kernel"] == "gsx" and out["tflops"] > 0
    assert 0 <= out["pad_share"] < 1, out["pad_share"]
