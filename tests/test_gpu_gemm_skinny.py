"""The skinny GEMM (native/kernels/gemm_skinny.hip, 1 <= M <= 128) on a real MI355X: bit for bit on operands whose
result is exact in any summation order, for every configuration and split of K; nothing read or written outside the
M rows; random operands within the decode family's derived bound; and the ``decode-wide`` workload."""
import json
import math
import subprocess
import sys
from pathlib import Path

import pytest

torch = pytest.importorskip("torch")

from tests import gemm_cases as gc  # noqa: E402
from tests import gemm_decode_cases as dc  # noqa: E402
from tests import gemm_fp8_cases as gf  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
KINDS = ("bf16", "fp8")
N = 192  # three strips of 64 columns, six of 32
MS = (1, 17, 47, 64, 113, 128)  # 17 and 113: one row, and one row short of a full fragment, in the ragged fragment
K_TILES = (1, 13, 67)  # most waves and splits idle; divisible by no wave count or split; the steady loop, ring wrapped
SPLITS = (1, 3, 16)
WS_BYTES = 16 * 128 * N * 4


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    from gpushare_scheduler_extender_amd.ops import hip as h

    assert h.SO.exists()
    return h


@pytest.fixture(scope="module")
def stream(hip):
    s = hip.Stream(0)
    yield s
    s.destroy()


@pytest.fixture(scope="module")
def ws():
    return torch.empty(WS_BYTES, device="cuda", dtype=torch.uint8)


def _problem(kind, k):
    """``(a, b, want, sa, sb, mode)`` of 128 rows on the CPU: the families' exact generators; fp8 with ROW scales."""
    if kind == "bf16":
        a, b, want = gc.exact_case(128, N, k)
        return a, b, want, None, None, gf.SCALE_NONE
    a, b, acc = gf.exact_case(128, N, k)
    sa, sb = gf.row_scales(128, 5), gf.row_scales(N, 7)
    return a, b, gf.scaled(acc, sa, sb), sa, sb, gf.SCALE_ROW


def _launch(hip, stream, kind, a, b, c, m, k, sa, sb, mode, ws, cfg=None, splits=None, n=N):
    args = (stream, kind, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k)
    tail = {"scale_a": 0 if sa is None else sa.data_ptr(), "scale_b": 0 if sb is None else sb.data_ptr(),
            "scale_mode": mode, "workspace": ws.data_ptr(), "workspace_bytes": ws.numel()}
    if cfg is None:
        hip.skinny_gemm_nt(*args, **tail)
    else:
        hip.skinny_gemm_nt_cfg(*args, cfg, splits, **tail)
    stream.sync()


@pytest.mark.parametrize("cfg", (0, 1, 2))
@pytest.mark.parametrize("kind", KINDS)
def test_exact_for_every_configuration_split_and_m(hip, stream, ws, kind, cfg):
    assert set(hip.skinny_gemm_cfgs()) == {0, 1, 2}
    for tiles in K_TILES:
        k = tiles * dc.BK[kind]
        a, b, want, sa, sb, mode = _problem(kind, k)
        da, db, dsa, dsb = (None if t is None else t.cuda() for t in (a, b, sa, sb))
        for splits in SPLITS:
            for m in MS:
                c = torch.full((m, N), float("nan"), device="cuda", dtype=torch.bfloat16)
                _launch(hip, stream, kind, da, db, c, m, k, dsa, dsb, mode, ws, cfg, splits)
                gc.assert_bits_equal(c, want[:m], f"{kind} cfg {cfg} splits {splits} M {m} K {k}")


@pytest.mark.parametrize("m", (17, 113))
@pytest.mark.parametrize("kind", KINDS)
def test_nothing_is_read_or_written_outside_the_m_rows(hip, stream, ws, kind, m):
    k = 13 * dc.BK[kind]
    a, b, want, sa, sb, mode = _problem(kind, k)
    # A's band of NaN begins right behind row m - 1; scale_a has exactly m entries
    a_whole, da = gc.banded(a[:m], gc.BF16_QNAN, "cuda") if kind == "bf16" else gf.banded(a[:m], "cuda")
    blank = torch.full((128, N), gc.C_BAND - 0x10000, dtype=torch.int16).view(torch.bfloat16)
    c_whole, dc_ = gc.banded(blank, gc.C_BAND, "cuda")
    dsa, dsb = (None, None) if sa is None else (sa[:m].cuda(), sb.cuda())
    _launch(hip, stream, kind, da, b.cuda(), dc_, m, k, dsa, dsb, mode, ws)
    gc.assert_bits_equal(dc_[:m], want[:m], f"{kind} M {m}: a read past row M - 1 shows as NaN")
    assert bool((gc.bits(dc_[m:].cpu()) == gc.C_BAND).all()), "rows M .. 127 of C were written"
    for band in gc.bands_of(c_whole, 128 * N):
        assert bool(((band.cpu().to(torch.int32) & 0xFFFF) == gc.C_BAND).all()), "C's band was written"
    del a_whole


@pytest.mark.parametrize("kind", KINDS)
def test_random_operands_dispatched_within_the_bound_and_repeatable(hip, stream, kind):
    m, n, k = 100, 1024, 8192
    g = torch.Generator().manual_seed(11)
    a, b = torch.randn(m, k, generator=g).bfloat16(), torch.randn(n, k, generator=g).bfloat16()
    one = None
    if kind == "fp8":
        a, b, one = a.to(gf.FP8), b.to(gf.FP8), torch.ones(1, device="cuda")
    mode = gf.SCALE_NONE if one is None else gf.SCALE_TENSOR
    ref64 = a.double() @ b.double().t()
    bound = dc.error_bound(ref64, a.double().abs() @ b.double().abs().t(), k)
    ws = torch.empty(max(16, hip.skinny_gemm_workspace_bytes(m, n, k)), device="cuda", dtype=torch.uint8)
    da, db = a.cuda(), b.cuda()
    got = [torch.full((m, n), float("nan"), device="cuda", dtype=torch.bfloat16) for _ in range(2)]
    for c in got:
        _launch(hip, stream, kind, da, db, c, m, k, one, one, mode, ws, n=n)
    err = (got[0].cpu().double() - ref64).abs()
    print(f"{kind}: largest error / bound = {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all()) and math.isfinite(float(err.max()))
    assert torch.equal(gc.bits(got[0].cpu()), gc.bits(got[1].cpu()))
    # a row has the same bits at every M that contains it, given the configuration and the splits
    cfg, splits = hip.skinny_gemm_pick(kind, m, n, k)
    big = torch.empty(16 * m * n * 4, device="cuda", dtype=torch.uint8)
    c100, c32 = torch.empty(m, n, device="cuda", dtype=torch.bfloat16), torch.empty(32, n, device="cuda",
                                                                                   dtype=torch.bfloat16)
    _launch(hip, stream, kind, da, db, c100, m, k, one, one, mode, big, cfg, splits, n=n)
    _launch(hip, stream, kind, da, db, c32, 32, k, one, one, mode, big, cfg, splits, n=n)
    gc.assert_bits_equal(c32, c100[:32].cpu(), f"{kind}: rows 0..31 at M = 32 and at M = 100")
    gc.assert_bits_equal(c100, got[0].cpu(), f"{kind}: the dispatched launch is cfg {cfg} with {splits} splits")


def test_decode_wide_workload_runs():
    r = subprocess.run([sys.executable, "-m", "gsxtools.workload", "--workload", "decode-wide", "--batch", "64",
                        "--size", "1024", "--iters", "2", "--json", "--kernel", "gsx"], cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["workload"] == "decode-wide" and out["batch"] == 64 and out["kernel"] == "gsx"
    assert math.isfinite(out["tbps"]) and out["tbps"] > 0
