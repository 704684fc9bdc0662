"""The block-scaled fp8 grouped GEMM of MoE prefill (native/kernels/moe_prefill_fp8_block.hip) on a real MI355X: bit
for bit against the fp64 sum of scaled block products on exact operands with power-of-two scales, bit for bit against
the dense ``128x128/4w`` block-scaled configuration on 24-bit scales, and the ``prefill-moe`` workload end to end.  The
routing is ``tests/test_gpu_moe_prefill.py``'s: 129, 128, 127, 1 and 1 pairs on five of eight experts."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import gemm_cases as gc  # noqa: E402
from tests import gemm_fp8_cases as fc  # noqa: E402
from tests.test_gpu_gemm_fp8_block import _dev_scales  # noqa: E402
from tests.test_gpu_moe_prefill import BM, _gemm_ids, dev, plan_ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
E = 8


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    from gpushare_scheduler_extender_amd.ops import hip as h

    assert h.moe_prefill_gemm_fp8_block_cfgs() == {0: ("128x128/4w-gather", 128, 128, 4)}
    return h


@pytest.fixture(scope="module")
def stream(hip):
    s = hip.Stream(0)
    yield s
    s.destroy()


def _by_expert(a, b, sa, sb, a_div, p, n):
    """``(exact, mag)[pair][expert][n]`` in fp64: the sum over g of the scaled block products of every pair's row of A
    against every expert, and the same of the magnitudes.  ``sb`` is ``[E][n / 128][K / 128]``."""
    r = torch.arange(p) // a_div
    a, b, sa, sb = a.double()[r], b.double(), sa.double()[r], sb.double()
    exact = torch.zeros(p, E * n, dtype=torch.float64)
    mag = torch.zeros_like(exact)
    for g in range(a.shape[1] // 128):
        ag, bg = a[:, 128 * g:128 * g + 128], b[:, 128 * g:128 * g + 128]
        s = sa[:, g, None] * sb[:, :, g].reshape(-1).repeat_interleave(128)[None, :]
        exact += (ag @ bg.t()) * s
        mag += (ag.abs() @ bg.abs().t()) * s.abs()
    return exact.view(p, E, n), mag.view(p, E, n)


def _run(hip, stream, a, a_div, b, plan, n, k, sa, sb, stride=None, timed=False):
    """The launch into a C full of NaN between guard bands, the scales between NaN: C on the host."""
    m, topk = _gemm_ids().shape
    whole, c = gc.banded(torch.full((m * topk, n), float("nan"), dtype=torch.bfloat16), gc.C_BAND, "cuda")
    a_d, b_d, plan_d = a.cuda(), b.cuda(), dev(plan)
    (keep_a, pa), (keep_b, pb) = _dev_scales(sa, stride), _dev_scales(sb.reshape(-1, k // 128))
    torch.cuda.synchronize()
    args = (stream, a_d.data_ptr(), a_div, b_d.data_ptr(), c.data_ptr(), plan_d.data_ptr(), m, topk, E, n, k)
    if timed:
        assert hip.time_moe_prefill_gemm_fp8_block(*args, 2, pa, stride or k // 128, pb) > 0
    else:
        hip.moe_prefill_gemm_fp8_block_nt_cfg(*args, 0, pa, stride or k // 128, pb)
    stream.sync()
    for band in gc.bands_of(whole, c.numel()):
        assert bool((band == gc.C_BAND - 0x10000).all()), "a guard band of C was written"
    return c.cpu()


@pytest.mark.parametrize("n", [128, 256])
@pytest.mark.parametrize("k", [128, 384, 640])
@pytest.mark.parametrize("up", [True, False], ids=["a_div=topk", "a_div=1"])
def test_grouped_gemm_exact(hip, stream, n, k, up):
    """1, 3 and 5 K-tiles, power-of-two scales: every pair's row is the fp64 sum against its own expert, rounded once,
    and no order of summation can round.  Then the same launch on a plan that claims T_max + 5 tiles and lists pair P:
    that entry's own pair stays NaN, nothing else changes."""
    ids = _gemm_ids()
    m, topk = ids.shape
    p, a_div, flat = m * topk, topk if up else 1, torch.from_numpy(ids.reshape(-1)).long()
    a, b, _ = fc.exact_case(p // a_div, E * n, k)
    rng = np.random.default_rng(1000 * n + k + up)
    sa = torch.from_numpy(2.0 ** rng.integers(-1, 2, (p // a_div, k // 128))).float()
    sb = torch.from_numpy(2.0 ** rng.integers(-1, 2, (E, n // 128, k // 128))).float()
    exact, mag = _by_expert(a, b, sa, sb, a_div, p, n)
    assert float(mag.max()) < 2 ** 12 and bool(((exact * 2 ** 10) % 1 == 0).all())
    assert torch.equal(exact.float().double(), exact)
    own = exact[torch.arange(p), flat]
    others = torch.arange(E) != flat[0]
    assert bool((exact[0, others] != own[0]).any(dim=1).all()), "pair 0's row does not tell its expert from the others"
    want = own.float().bfloat16()
    plan = plan_ref(ids, E)
    fc.assert_bits_equal(_run(hip, stream, a, a_div, b, plan, n, k, sa, sb), want, "the plan")
    t_max = (p + E * (BM - 1)) // BM
    at = 4 + t_max + 5  # a row of tile 0
    lost, plan[0], plan[at] = int(plan[at]), t_max + 5, p
    got = _run(hip, stream, a, a_div, b, plan, n, k, sa, sb)
    assert bool(got[lost].isnan().all()), "the pair whose entry was overwritten was stored"
    keep = torch.arange(p) != lost
    fc.assert_bits_equal(got[keep], want[keep], "n_tiles = T_max + 5, a row of P")


def test_grouped_gemm_general_scales_have_the_dense_kernels_bits(hip, stream):
    """The summation order and the scale gather: 24-bit scales of both signs, ``sa_stride = K / 128 + 3`` with NaN in
    the padding, through the timed call; per expert, its gathered rows and scale rows padded to 128 through the dense
    ``128x128/4w``."""
    ids, n, k = _gemm_ids(), 256, 640
    (m, topk), g = ids.shape, k // 128
    a, b, _ = fc.exact_case(m, E * n, k)
    sa, sb = fc.row_scales(m * g, 61).view(m, g), fc.row_scales(E * (n // 128) * g, 67).view(E, n // 128, g)
    got = _run(hip, stream, a, topk, b, plan_ref(ids, E), n, k, sa, sb, stride=g + 3, timed=True)
    dense = {name: i for i, name in hip.gemm_fp8_block_cfgs().items()}["128x128/4w"]
    flat = ids.reshape(-1)
    for x in np.unique(flat):
        prs = np.flatnonzero(flat == x)
        src, rows = torch.from_numpy(prs // topk), -(-len(prs) // BM) * BM
        ga, gs = torch.zeros(rows, k, dtype=torch.uint8), torch.ones(rows, g)  # code 0 is +0
        ga[:len(prs)], gs[:len(prs)] = a.view(torch.uint8)[src], sa[src]
        ga, xb, cs = ga.cuda(), b[x * n:(x + 1) * n].cuda(), torch.empty(rows, n, dtype=torch.bfloat16, device="cuda")
        (keep_a, pa), (keep_b, pb) = _dev_scales(gs, g + 3), _dev_scales(sb[x])
        torch.cuda.synchronize()
        hip.gemm_fp8_block_nt_cfg(stream, ga.data_ptr(), xb.data_ptr(), cs.data_ptr(), rows, n, k, dense, pa, g + 3, pb)
        stream.sync()
        fc.assert_bits_equal(got[torch.from_numpy(prs)], cs[:len(prs)].cpu(), f"expert {x}")


def test_workload_prefill_moe_fp8_block_end_to_end():
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "gsxtools.workload", "--workload", "prefill-moe", "--dtype", "fp8-block",
                        "--experts", "128", "--experts-active", "2", "--heads", "2", "--kv-heads", "1", "--ffn", "128",
                        "--context", "128", "--chunk", "128", "--batch", "1", "--iters", "2", "--json", "--weights-gib",
                        "0.01", "--kv-gib", "0.0005"], env=env, cwd=str(ROOT), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["workload"] == "prefill-moe" and out["dtype"] == "fp8-block" and out["kernel"] == "gsx"
    assert out["activations_finite"] is True and out["tflops"] > 0
    assert 0 <= out["pad_share"] < 1, out["pad_share"]
