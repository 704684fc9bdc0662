"""The block-scaled fp8 skinny GEMM (native/kernels/gemm_skinny_fp8_block.hip) on a real MI355X.

The reference is the fp64 sum of the scaled block products.  With power-of-two scales on ``gemm_fp8_cases``' exact
operands no order of summation can round and the comparison is on the raw 16 bits; with general scales every element
lies inside the interval the contract's own roundings allow.  Every case starts from a C full of NaN.
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

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
NAN = float("nan")
N = 192  # three 64-column strips; the second block row of scale_b covers 64 columns
PAD = 3  # sa_stride = K / 128 + PAD


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    from gpushare_scheduler_extender_amd.ops import hip as h

    return h


@pytest.fixture(scope="module")
def stream(hip):
    s = hip.Stream(0)
    yield s
    s.destroy()


@pytest.fixture(scope="module")
def ws():
    return torch.empty(16 * 128 * 1024 * 4, dtype=torch.uint8, device="cuda")


def _reference(a, b, sa, sb):
    """``(sum_g p_g sa sb, sum_g |p|_g |sa sb|)`` in fp64; ``sb`` has ``ceil(N / 128)`` rows."""
    a, b, sa, sb = a.double(), b.double(), sa.double(), sb.double()
    exact = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float64)
    mag = torch.zeros_like(exact)
    for g in range(a.shape[1] // 128):
        ag, bg = a[:, 128 * g:128 * g + 128], b[:, 128 * g:128 * g + 128]
        s = sa[:, g, None] * sb[:, g].repeat_interleave(128)[None, :b.shape[0]]
        exact += (ag @ bg.t()) * s
        mag += (ag.abs() @ bg.abs().t()) * s.abs()
    return exact, mag


@functools.lru_cache(maxsize=None)
def _exact(tiles):
    """128 x 192 x ``128 tiles`` exact operands, scales ``2^e`` with ``e`` from {-1, 0, 1} drawn independently per
    (row, g) and per (nb, g), and the bf16 result; asserts on the CPU that no order of summation can round."""
    k = 128 * tiles
    a, b, _ = fc.exact_case(128, N, k)
    rng = np.random.default_rng(3)
    sa = torch.from_numpy(2.0 ** rng.integers(-1, 2, (128, tiles))).float()
    sb = torch.from_numpy(2.0 ** rng.integers(-1, 2, ((N + 127) // 128, tiles))).float()
    exact, mag = _reference(a, b, sa, sb)
    assert float(mag.max()) < 2 ** 12 and bool(((exact * 2 ** 10) % 1 == 0).all())
    assert torch.equal(exact.float().double(), exact)
    return a, b, sa, sb, exact.float().bfloat16()


def _padded_scales(sa):
    """``sa`` on the device with rows ``g + PAD`` apart, NaN in the padding and NaN right behind the last row."""
    rows, g = sa.shape
    body = torch.full((rows, g + PAD), NAN)
    body[:, :g] = sa
    return torch.cat([body.flatten()[:(rows - 1) * (g + PAD) + g], torch.full((1024,), NAN)]).cuda()


def _launch(hip, s, a, b, c, m, sa, sa_stride, sb, ws, cfg=None, splits=None, timed=False):
    n, k = b.shape
    args = (a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k)
    tail = dict(scale_a=sa.data_ptr(), sa_stride=sa_stride, scale_b=sb.data_ptr(), workspace=ws.data_ptr(),
                workspace_bytes=ws.numel())
    torch.cuda.synchronize()
    if timed:
        assert hip.time_skinny_gemm_fp8_block(s, *args, 2, **tail) > 0
    elif cfg is None:
        hip.skinny_gemm_fp8_block_nt(s, *args, **tail)
    else:
        hip.skinny_gemm_fp8_block_nt_cfg(s, *args, cfg, splits, **tail)
    s.sync()


@pytest.mark.parametrize("cfg", [0, 1, 2])
def test_exact_at_every_split_and_row_count(hip, stream, ws, cfg):
    """1, 13 and 67 K-tiles (most waves and splits idle, no divisor of a wave count or split, the steady loop with the
    ring wrapped) under 1, 3 and 16 splits, at row counts with and without a ragged last fragment."""
    assert set(hip.skinny_gemm_fp8_block_cfgs()) == {0, 1, 2}
    for tiles in (1, 13, 67):
        a, b, sa, sb, want = _exact(tiles)
        da, db, dsa, dsb = a.cuda(), b.cuda(), _padded_scales(sa), sb.cuda()
        for splits in (1, 3, 16):
            for m in (1, 17, 47, 64, 113, 128):
                c = torch.full((m, N), NAN, device="cuda", dtype=torch.bfloat16)
                _launch(hip, stream, da, db, c, m, dsa, tiles + PAD, dsb, ws, cfg, splits)
                fc.assert_bits_equal(c, want[:m], f"cfg {cfg}, {tiles} K-tiles, {splits} splits, M {m}")


@pytest.mark.parametrize("m", [17, 113])
def test_nothing_is_read_or_written_outside_the_m_rows(hip, stream, ws, m):
    """A's band of e4m3 NaN begins right behind row M - 1, scale_a has exactly M rows with NaN behind them, C is 128
    rows of NaN between bands."""
    tiles = 13
    a, b, sa, sb, want = _exact(tiles)
    a_whole, da = fc.banded(a[:m], "cuda")
    dsa, db, dsb = _padded_scales(sa[:m]), b.cuda(), sb.cuda()
    for cfg, splits in ((0, 1), (1, 3), (2, 16)):
        c_whole, dc = gc.banded(torch.full((128, N), NAN, dtype=torch.bfloat16), gc.C_BAND, "cuda")
        blank = gc.bits(dc[m:].cpu()).clone()
        _launch(hip, stream, da, db, dc, m, dsa, tiles + PAD, dsb, ws, cfg, splits)
        fc.assert_bits_equal(dc[:m], want[:m], f"cfg {cfg} M {m}: a read past row M - 1 shows as NaN")
        assert torch.equal(gc.bits(dc[m:].cpu()), blank), "rows M .. 127 of C were written"
        for band in gc.bands_of(c_whole, 128 * N):
            assert bool(((band.cpu().to(torch.int32) & 0xFFFF) == gc.C_BAND).all()), "C's band was written"
    del a_whole


def test_general_scales_from_the_quantiser_dispatched(hip, stream, ws):
    """100 x 1024 x 8192: A and scale_a from ``gsx_quant_fp8_block`` on randn rows, B block-quantised in torch.
    Every element lies between ``bf16(exact - err)`` and ``bf16(exact + err)``, ``exact`` the fp64 product of the
    dequantised operands and ``err = (127 + K / 128 + 2) 2^-24 sum |a b s|``: 127 for the MFMA's 128-term sum in any
    order, K / 128 + 2 for the contract's own roundings (at most K / 128 - 1 additions in any tree of waves and
    splits, the rounding of s_g, and slack for second order)."""
    m, n, k = 100, 1024, 8192
    g = torch.Generator().manual_seed(5)
    x = torch.randn(m, k, generator=g).bfloat16().cuda()
    blocks = torch.randn(n, k, generator=g).view(n // 128, 128, k // 128, 128)
    sb = blocks.abs().amax(dim=(1, 3)) / 448.0
    b = (blocks / sb[:, None, :, None]).reshape(n, k).to(fc.FP8).cuda()
    q = torch.empty(m, k, dtype=torch.uint8, device="cuda")
    sa = torch.empty(m, k // 128, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    hip.quant_fp8_block(stream, x.data_ptr(), k, q.data_ptr(), k, sa.data_ptr(), k // 128, m, k)
    stream.sync()
    dsb = sb.cuda()

    def product(rows, **kw):
        c = torch.full((rows, n), NAN, device="cuda", dtype=torch.bfloat16)
        _launch(hip, stream, q, b, c, rows, sa, k // 128, dsb, ws, **kw)
        return c.cpu()

    got = product(m)
    exact, mag = _reference(q.cpu().view(fc.FP8), b.cpu(), sa.cpu(), sb)
    err = (127 + k // 128 + 2) * 2.0 ** -24 * mag
    lo, hi = ((exact + d).float().bfloat16().double() for d in (-err, err))
    assert bool(((got.double() >= lo) & (got.double() <= hi)).all())
    print(f"largest |got - exact| / err: {float(((got.double() - exact).abs() / err).max()):.4f}")
    cfg, splits = hip.skinny_gemm_fp8_block_pick(m, n, k)
    assert torch.equal(gc.bits(product(m)), gc.bits(got)), "the same call twice"
    assert torch.equal(gc.bits(product(m, cfg=cfg, splits=splits)), gc.bits(got)), "_launch_cfg with _pick's answer"
    assert torch.equal(gc.bits(product(32, cfg=cfg, splits=splits)), gc.bits(got[:32])), "rows 0 .. 31 at M = 32"
    assert torch.equal(gc.bits(product(m, timed=True)), gc.bits(got)), "the timed call"


def test_workload_runs_decode_wide_on_block_scaled_operands():
    main = str(ROOT / "samples" / "workload" / "main.py")
    r = subprocess.run([sys.executable, main, "--workload", "decode-wide", "--dtype", "fp8-block", "--kernel", "gsx",
                        "--batch", "40", "--size", "1024", "--iters", "2", "--json"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["dtype"] == "fp8-block" and np.isfinite(out["tbps"]) and out["tbps"] > 0, out
