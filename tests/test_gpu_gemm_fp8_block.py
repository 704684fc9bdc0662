"""The block-scaled fp8 GEMM and its quantiser (native/kernels/gemm_fp8_block.hip) on a real MI355X.

Operands come from ``tests/gemm_fp8_cases.py``: every block product ``p_g`` is exact, whatever the MFMA's order.  The
reference is the fp64 sum of the scaled block products.  With power-of-two scales every order of every rounding
scheme is exact and the comparison is on the raw 16 bits; with general scales the bound is the contract's own
roundings (``_assert_within``) and every element is checked.  Every case starts from a C full of NaN.
"""
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
from tests import norm_act_cases as nc  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CFGS = [0, 1, 2]
TILE = {0: (128, 128), 1: (256, 128), 2: (256, 256)}  # 128x128/4w, 256x128/8w, 256x256/8w (dispatched)
NAN = float("nan")
U = 2.0 ** -24


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    from gpushare_scheduler_extender_amd.ops import hip as h

    assert len(h.gemm_fp8_block_cfgs()) == len(CFGS)
    return h


@pytest.fixture(scope="module")
def stream(hip):
    s = hip.Stream(0)
    yield s
    s.destroy()


def _pow2_scales(m, n, k, seed):
    """``2^e``, ``e`` from {-1, 0, 1} independently per (row, g) and per (nb, g)."""
    rng = np.random.default_rng(seed)
    return (torch.from_numpy(2.0 ** rng.integers(-1, 2, (m, k // 128))).float(),
            torch.from_numpy(2.0 ** rng.integers(-1, 2, (n // 128, k // 128))).float())


def _reference(a, b, sa, sb):
    """``(sum_g p_g sa sb, sum_g |p|_g |sa sb|)`` in fp64, ``|p|_g`` the block product of the magnitudes."""
    a, b, sa, sb = a.double(), b.double(), sa.double(), sb.double()
    exact = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float64)
    mag = torch.zeros_like(exact)
    for g in range(a.shape[1] // 128):
        ag, bg = a[:, 128 * g:128 * g + 128], b[:, 128 * g:128 * g + 128]
        s = sa[:, g, None] * sb[:, g].repeat_interleave(128)[None, :]
        exact += (ag @ bg.t()) * s
        mag += (ag.abs() @ bg.abs().t()) * s.abs()
    return exact, mag


def _dev_scales(s, stride=None):
    """``s`` as fp32 rows ``stride`` apart on the device, 4-B aligned and no more, with NaN in the padding of every
    row and in 1 KiB-and-more bands on either side: ``(keep, address)``."""
    rows, g = s.shape
    body = torch.full((rows, stride or g), NAN)
    body[:, :g] = s
    whole = torch.cat([torch.full((1025,), NAN), body.flatten(), torch.full((1024,), NAN)]).cuda()
    assert whole[1025:].data_ptr() % 8 == 4
    return whole, whole[1025:].data_ptr()


def _nan_c(m, n):
    return torch.full((m, n), NAN, device="cuda", dtype=torch.bfloat16)


def _run(hip, s, a, b, c, sa, sb, cfg=None, stride=None, timed=False):
    (m, k), n = a.shape, b.shape[0]
    keep_a, pa = _dev_scales(sa, stride)
    keep_b, pb = _dev_scales(sb)
    args = (a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k)
    torch.cuda.synchronize()
    if timed:
        assert hip.time_gemm_fp8_block(s, *args, 3, pa, stride or k // 128, pb) > 0
    elif cfg is None:
        hip.gemm_fp8_block_nt(s, *args, pa, stride or k // 128, pb)
    else:
        hip.gemm_fp8_block_nt_cfg(s, *args, cfg, pa, stride or k // 128, pb)
    s.sync()


def _product(hip, s, a_h, b_h, sa, sb, **kw):
    c = _nan_c(a_h.shape[0], b_h.shape[0])
    _run(hip, s, a_h.cuda(), b_h.cuda(), c, sa, sb, **kw)
    return c.cpu()


def _exact_want(m, n, k, seed):
    """Case 1's operands, scales and bf16 result; asserts on the CPU that no order of summation can round."""
    a, b, _ = fc.exact_case(m, n, k)
    sa, sb = _pow2_scales(m, n, k, seed)
    exact, mag = _reference(a, b, sa, sb)
    assert float(mag.max()) < 2 ** 12 and bool(((exact * 2 ** 10) % 1 == 0).all())
    assert torch.equal(exact.float().double(), exact)
    return a, b, sa, sb, exact.float().bfloat16()


def _assert_within(got, exact, err, what):
    """Every element between ``bf16(exact - err)`` and ``bf16(exact + err)``: rounding is monotone."""
    lo, hi = ((exact + d).float().bfloat16().double() for d in (-err, err))
    bad = ~((got.double() >= lo) & (got.double() <= hi))
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements outside their interval, first at "
                                 f"{bad.nonzero()[0].tolist()}; largest |got - exact| {float((got.double() - exact).abs().max())}")


# ---- 1. exact, bit for bit -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("k", [128, 256, 384, 896])
@pytest.mark.parametrize("shape", ["tile", "blocks"])
def test_fp8_block_gemm_exact(hip, stream, shape, k, cfg):
    """1, 2, 3 and 7 K-tiles (buffer parity, a K / 128 that is no multiple of 4) on one block tile and on several."""
    m, n = TILE[cfg] if shape == "tile" else (384, 256) if cfg == 0 else (768, 512)
    a, b, sa, sb, want = _exact_want(m, n, k, 7 * k + cfg)
    fc.assert_bits_equal(_product(hip, stream, a, b, sa, sb, cfg=cfg), want, f"cfg {cfg} at {m}x{n}x{k}")


# ---- 2. general scales, against fp64 within the contract's roundings -----------------------------------------------

@pytest.mark.parametrize("cfg", CFGS)
def test_fp8_block_gemm_general_scales(hip, stream, cfg):
    """24-bit scales of both signs, ``sa_stride = K / 128 + 3`` with NaN in the padding.  The roundings are one for
    ``s_g`` and one per fma: ``|acc - exact| <= (K / 128 + 2) 2^-24 sum_g |p_g s_g|``."""
    (m, n), k = ((384, 256) if cfg == 0 else (768, 512)), 1024
    a, b, _ = fc.exact_case(m, n, k)
    sa = fc.row_scales(m * (k // 128), 31 + cfg).view(m, k // 128)
    sb = fc.row_scales((n // 128) * (k // 128), 37 + cfg).view(n // 128, k // 128)
    exact, mag = _reference(a, b, sa, sb)
    got = _product(hip, stream, a, b, sa, sb, cfg=cfg, stride=k // 128 + 3)
    _assert_within(got, exact, (k // 128 + 2) * U * mag, f"cfg {cfg}, general scales")


# ---- 3. guard bands and minimum alignment --------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", CFGS)
def test_fp8_block_gemm_guard_bands_and_minimum_alignment(hip, stream, cfg):
    """768 x 512 x 384 on operands 16 B past a 32-B boundary between bands of fp8 NaN (A, B), NaN (the scales, and the
    padding of scale_a's rows) and 0xC3C3 (C)."""
    m, n, k = 768, 512, 384
    a_h, b_h, sa, sb, want = _exact_want(m, n, k, 99)
    wa, a = fc.banded(a_h, "cuda")
    wb, b = fc.banded(b_h, "cuda")
    wc, c = gc.banded(torch.full((m, n), NAN, dtype=torch.bfloat16), gc.C_BAND, "cuda")
    wa0, wb0 = wa.clone(), wb.clone()
    _run(hip, stream, a, b, c, sa, sb, cfg=cfg, stride=k // 128 + 2)
    for band in gc.bands_of(wc, c.numel()):
        assert not bool(((band.to(torch.int32) & 0xFFFF) != gc.C_BAND).any()), f"cfg {cfg}: a band of C was written"
    assert torch.equal(wa, wa0) and torch.equal(wb, wb0), f"cfg {cfg}: A or B, or a band of theirs, was written"
    fc.assert_bits_equal(c.cpu(), want, f"cfg {cfg} at {m}x{n}x{k}")


# ---- 4. refusals ---------------------------------------------------------------------------------------------------

def test_fp8_block_gemm_refusals(hip, stream):
    m, n, k = 256, 256, 256
    a_h, b_h, sa_h, sb_h, _ = _exact_want(m, n, k, 5)
    a, b, c = a_h.cuda(), b_h.cuda(), _nan_c(m, n)
    (_ka, sa), (_kb, sb) = _dev_scales(sa_h), _dev_scales(sb_h)
    base = dict(a=a.data_ptr(), b=b.data_ptr(), c=c.data_ptr(), m=m, n=n, k=k, scale_a=sa, sa_stride=2, scale_b=sb)
    k_bad = (2 ** 31 - 1 - 112) // 255 // 128 * 128 + 128
    bad = [(dict(m=384), "need M%256==0"), (dict(n=128), "need M%256==0, N%256==0"), (dict(k=192), "K%128==0"),
           (dict(m=0), "need M%256==0"), (dict(a=0), "must not be NULL"), (dict(c=0), "must not be NULL"),
           (dict(scale_b=0), "must not be NULL"), (dict(b=b.data_ptr() + 8), "operands must be 16-B aligned"),
           (dict(scale_a=sa + 2), "scale_a and scale_b must be 4-B aligned"), (dict(sa_stride=1), "need sa_stride >= K/128"),
           (dict(k=k_bad, sa_stride=k_bad // 128), "K too large"), (dict(c=a.data_ptr()), "C must not overlap"),
           (dict(cfg=3), "unknown config"), (dict(cfg=-1), "unknown config")]
    torch.cuda.synchronize()
    for change, text in bad:
        kw = {"cfg": 2, **base, **change}
        with pytest.raises(hip.HipError, match=f"gsx_gemm_fp8_block_nt_launch_cfg: .*{text}"):
            hip.gemm_fp8_block_nt_cfg(stream, **kw)
    with pytest.raises(hip.HipError, match="gsx_gemm_fp8_block_nt: need M%128==0, N%128==0"):
        hip.gemm_fp8_block_nt(stream, **{**base, "n": 192})
    with pytest.raises(hip.HipError, match="gsx_gemm_fp8_block_nt: K too large"):
        hip.gemm_fp8_block_nt(stream, **{**base, "k": k_bad, "sa_stride": k_bad // 128})
    stream.sync()
    assert bool(torch.isnan(c).all())  # no refused call launched anything


# ---- 5. the dispatching entry point and the timed call -------------------------------------------------------------

@pytest.mark.parametrize("m,n,k", [(384, 128, 256), (512, 512, 256)])
@pytest.mark.parametrize("timed", [False, True])
def test_fp8_block_gemm_dispatch_and_timed_call(hip, stream, timed, m, n, k):
    """The 128 tile at 384 x 128 and the 256 tile at 512 x 512, directly and through the timed call."""
    a, b, sa, sb, want = _exact_want(m, n, k, 17)
    fc.assert_bits_equal(_product(hip, stream, a, b, sa, sb, timed=timed), want, f"dispatched at {m}x{n}x{k}")


# ---- 6. the quantiser ----------------------------------------------------------------------------------------------

def _quantise(hip, stream, x, q_stride, s_stride):
    """``x`` (bf16, possibly a strided view) through ``quant_fp8_block``: the codes and scales, padding checked."""
    r, k = x.shape
    q = torch.full((r, q_stride), 0x5A, dtype=torch.uint8, device="cuda")
    s = torch.full((r, s_stride), NAN, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    hip.quant_fp8_block(stream, x.data_ptr(), x.stride(0), q.data_ptr(), q_stride, s.data_ptr(), s_stride, r, k)
    stream.sync()
    assert bool((q[:, k:] == 0x5A).all()) and bool(torch.isnan(s[:, k // 128:]).all()), "padding was written"
    return q[:, :k], s[:, :k // 128]


def test_fp8_block_quantiser_groups(hip, stream):
    """130 rows of 3 groups, padded strides, magnitudes from 2^-20 to 2^15: a zero group, the amax at position 0 and
    at position 127, a negative amax.  Checked per group as ``GSX_ACT_OUT_FP8_ROW`` is per row, with no input error."""
    r, k = 130, 384
    rng = np.random.default_rng(3)
    x = rng.standard_normal((r, k)) * 2.0 ** rng.integers(-20, 13, (r, k // 128)).repeat(128, axis=1)
    x[0, :128] = 0
    x[1, 128], x[2, 255], x[3, 300] = 2.0 ** 15, 2.0 ** 15, -(2.0 ** 15)
    xd = torch.zeros(r, k + 8, dtype=torch.bfloat16)
    xd[:, :k] = torch.from_numpy(x).bfloat16()
    q, s = _quantise(hip, stream, xd.cuda()[:, :k], k + 16, k // 128 + 2)
    exact = xd[:, :k].double().numpy().reshape(-1, 128)
    nc.check_fp8(q.cpu().numpy().reshape(-1, 128), s.cpu().numpy().reshape(-1), exact, 0.0, "quant_fp8_block")


def test_fp8_block_quantiser_feeds_the_gemm(hip, stream):
    """The quantiser's Q and S and a B block-quantised in torch through the GEMM at 128 x 256 x 512, against the fp64
    product of the dequantised operands: the any-order bound of a 128-term fp32 sum plus case 2's,
    ``(127 + K / 128 + 2) 2^-24 sum |a b s|``."""
    m, n, k = 128, 256, 512
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(m, k, generator=g) * 3).bfloat16()
    blocks = torch.randn(n, k, generator=g).view(n // 128, 128, k // 128, 128)
    sb = blocks.abs().amax(dim=(1, 3)) / 448.0
    b = (blocks / sb[:, None, :, None]).reshape(n, k).to(fc.FP8)
    q, sa = _quantise(hip, stream, x.cuda(), k, k // 128)
    c = _nan_c(m, n)
    torch.cuda.synchronize()
    hip.gemm_fp8_block_nt(stream, q.data_ptr(), b.cuda().data_ptr(), c.data_ptr(), m, n, k, sa.data_ptr(), k // 128,
                          sb.cuda().data_ptr())
    stream.sync()
    exact, mag = _reference(q.cpu().view(fc.FP8), b, sa.cpu(), sb)
    _assert_within(c.cpu(), exact, (127 + k // 128 + 2) * U * mag, "quantiser into the GEMM")


# ---- 7. the workload -----------------------------------------------------------------------------------------------

def test_workload_runs_fp8_block_and_other_workloads_refuse_it():
    main = str(ROOT / "samples" / "workload" / "main.py")
    r = subprocess.run([sys.executable, main, "--workload", "gemm", "--dtype", "fp8-block", "--kernel", "gsx", "--size",
                        "1024", "--iters", "2", "--json"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["dtype"] == "fp8-block" and np.isfinite(out["tflops"]) and out["tflops"] > 0, out
    r = subprocess.run([sys.executable, main, "--workload", "decode", "--dtype", "fp8-block"], capture_output=True,
                       text=True, timeout=60, env={**os.environ, "HIP_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": ""})
    assert r.returncode == 2 and "gemm workload's only" in r.stderr, r.stderr[-2000:]
