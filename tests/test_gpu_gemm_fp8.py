"""The fp8 (e4m3) GEMM (native/kernels/gemm_fp8.hip), bit for bit on a real MI355X.

Operands and the reference come from ``tests/gemm_fp8_cases.py``; ``tests/test_gemm_fp8_cases.py`` checks on the CPU
that the operands have the properties relied on here.  The reference everywhere is the fp64 product on the CPU
rounded once to fp32, the epilogue's two fp32 multiplies where scales are given, and one rounding to bf16.  Every
comparison is on the raw 16 bits: a NaN has to be a quiet NaN (any sign and payload), everything else has to be
bit-equal, nothing is left out and nothing has a tolerance.
"""
import ctypes

import pytest

torch = pytest.importorskip("torch")

from tests import gemm_cases as gc  # noqa: E402
from tests import gemm_fp8_cases as fc  # noqa: E402

pytestmark = pytest.mark.gpu

CFGS = [0, 1, 2]  # 128x128/4w, 256x256/8w-phased-g4 (dispatched), 256x256/8w-phased-g4-mfma32
TILE = {0: 128, 1: 256, 2: 256}
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    from gpushare_scheduler_extender_amd.ops import hip as h

    assert h.SO.exists()
    assert len(h.gemm_fp8_cfgs()) == len(CFGS)
    for cfg in CFGS:
        bm, bn = ctypes.c_int(0), ctypes.c_int(0)
        assert h.lib().gsx_gemm_fp8_cfg_tile(cfg, ctypes.byref(bm), ctypes.byref(bn)) == 0
        assert bm.value == bn.value == TILE[cfg]
    return h


@pytest.fixture(scope="module")
def stream(hip):
    s = hip.Stream(0)
    yield s
    s.destroy()


def _nan_c(m, n):
    return torch.full((m, n), NAN, device="cuda", dtype=torch.bfloat16)


def _run(hip, s, a, b, c, cfg=None, sa=None, sb=None, mode=fc.SCALE_NONE):
    """One configuration (``cfg`` None: the dispatching entry point) on our own stream, after everything torch's
    stream did to the operands has finished."""
    (m, k), n = a.shape, b.shape[0]
    assert b.shape[1] == k and c.shape == (m, n) and a.is_contiguous() and b.is_contiguous() and c.is_contiguous()
    assert a.dtype == b.dtype == fc.FP8 and c.dtype == torch.bfloat16
    pa, pb = (0, 0) if sa is None else (sa.data_ptr(), sb.data_ptr())
    torch.cuda.synchronize()
    if cfg is None:
        hip.gemm_fp8_nt(s, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, pa, pb, mode)
    else:
        hip.gemm_fp8_nt_cfg(s, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, cfg, pa, pb, mode)
    s.sync()


def _product(hip, s, a_h, b_h, cfg=None, **kw):
    c = _nan_c(a_h.shape[0], b_h.shape[0])
    _run(hip, s, a_h.cuda(), b_h.cuda(), c, cfg, **kw)
    return c.cpu()


# ---- 1. K-tile counts and tile maps, exactly -----------------------------------------------------------------------

@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("k", [128, 256, 384, 512, 896, 16384])
@pytest.mark.parametrize("shape", ["tile", "768x512"])
def test_fp8_gemm_k_tile_counts_exact(hip, stream, shape, k, cfg):
    """nk = 1 (prologue only), 2, 3, 4 and 7 (buffer parity and the clamped past-the-end stages) and nk = 128 (a
    long loop), on one block and on 768 x 512: six workgroups for the 256 x 256 kernels, fewer than the eight XCDs
    the tile map remaps over, and six tile-rows for the 128 x 128 tile, whose groups of eight end ragged."""
    m, n = (TILE[cfg], TILE[cfg]) if shape == "tile" else (768, 512)
    a, b, acc = fc.exact_case(m, n, k)
    fc.assert_bits_equal(_product(hip, stream, a, b, cfg), fc.scaled(acc), f"cfg {cfg} at {m}x{n}x{k}")


# ---- 2. every e4m3 code, and the k positions of the two operand paths ----------------------------------------------

@pytest.mark.parametrize("cfg", CFGS)
def test_fp8_gemm_code_sweep(hip, stream, cfg):
    """Every e4m3 code, at every k position of a K-tile, against +-2^-9 .. 2^8 (subnormals included): tells OCP
    e4m3 from fnuz, catches a wrong format select and a hardware scale that is not 1.  The two NaN codes make their
    rows NaN and touch nothing else; zeros are compared by value."""
    a, b, want = fc.code_sweep()
    fc.assert_bits_equal(_product(hip, stream, a, b, cfg), want, f"cfg {cfg}, code sweep", zeros_by_value=True)


@pytest.mark.parametrize("cfg", CFGS)
def test_fp8_gemm_k_slots_of_a_and_b_agree(hip, stream, cfg):
    """``C[i][j] = u_i v_j`` where ``i = j (mod 256)`` and 0 elsewhere: a k position that A's path and B's path
    disagree on shows as a named row and column, in both LDS buffers."""
    a, b, want = fc.k_slot_case()
    fc.assert_bits_equal(_product(hip, stream, a, b, cfg), want, f"cfg {cfg}, k slots")


# ---- 3. guard bands and 16-B-only alignment ------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", CFGS)
def test_fp8_gemm_guard_bands_and_minimum_alignment(hip, stream, cfg):
    """512 x 768 x 384 on operands 16 B past a 32-B boundary, between bands of fp8 NaN (A and B) and 0xC3C3 (C): any
    use of data outside A or B turns into a NaN in C, any element of C not written stays NaN, and a store outside C
    lands in a band."""
    m, n, k = 512, 768, 384
    a_h, b_h, acc = fc.exact_case(m, n, k)
    wa, a = fc.banded(a_h, "cuda")
    wb, b = fc.banded(b_h, "cuda")
    wc, c = gc.banded(torch.full((m, n), NAN, dtype=torch.bfloat16), gc.C_BAND, "cuda")
    for t in (a, b, c):
        assert t.data_ptr() % 32 == 16
    wa0, wb0 = wa.clone(), wb.clone()
    _run(hip, stream, a, b, c, cfg)
    for band in gc.bands_of(wc, c.numel()):
        changed = (band.to(torch.int32) & 0xFFFF) != gc.C_BAND
        assert not bool(changed.any()), f"cfg {cfg}: {int(changed.sum())} elements of a band of C were written"
    assert torch.equal(wa, wa0) and torch.equal(wb, wb0), f"cfg {cfg}: A or B, or a band of theirs, was written"
    fc.assert_bits_equal(c.cpu(), fc.scaled(acc), f"cfg {cfg} at {m}x{n}x{k}")


# ---- 4. scales -----------------------------------------------------------------------------------------------------

SCALE_SHAPES = {0: (384, 256, 384), 1: (512, 768, 384)}  # several blocks each; the second shares section 3's case


@pytest.mark.parametrize("cfg", [0, 1])
def test_fp8_gemm_no_scales_equal_unit_scales(hip, stream, cfg):
    m, n, k = SCALE_SHAPES[cfg]
    a, b, acc = fc.exact_case(m, n, k)
    one = torch.ones(1, device="cuda", dtype=torch.float32)
    plain = _product(hip, stream, a, b, cfg)
    unit = _product(hip, stream, a, b, cfg, sa=one, sb=one, mode=fc.SCALE_TENSOR)
    assert torch.equal(gc.bits(plain), gc.bits(unit))
    fc.assert_bits_equal(plain, fc.scaled(acc), f"cfg {cfg}, no scales")
    # no scales: the pointers are not looked at
    a_d, b_d, c = a.cuda(), b.cuda(), _nan_c(m, n)
    torch.cuda.synchronize()
    hip.gemm_fp8_nt_cfg(stream, a_d.data_ptr(), b_d.data_ptr(), c.data_ptr(), m, n, k, cfg, 3, 5, fc.SCALE_NONE)
    stream.sync()
    assert torch.equal(gc.bits(c.cpu()), gc.bits(plain))


@pytest.mark.parametrize("cfg", [0, 1])
@pytest.mark.parametrize("sa,sb", [(8.0, 2.0 ** -5), (-(2.0 ** -3), 4.0)])
def test_fp8_gemm_per_tensor_scales(hip, stream, sa, sb, cfg):
    m, n, k = SCALE_SHAPES[cfg]
    a, b, acc = fc.exact_case(m, n, k)
    sa_h, sb_h = torch.tensor([sa], dtype=torch.float32), torch.tensor([sb], dtype=torch.float32)
    got = _product(hip, stream, a, b, cfg, sa=sa_h.cuda(), sb=sb_h.cuda(), mode=fc.SCALE_TENSOR)
    fc.assert_bits_equal(got, fc.scaled(acc, sa_h, sb_h), f"cfg {cfg}, per-tensor scales {sa}, {sb}")


@pytest.mark.parametrize("cfg", [0, 1])
def test_fp8_gemm_per_row_scales(hip, stream, cfg):
    """Random 24-bit scales of both signs per row of A and of B: ``bf16((acc * sa[row]) * sb[col])`` with the two
    multiplies in that order.  The scale vectors are 4-B aligned and no more."""
    m, n, k = SCALE_SHAPES[cfg]
    a, b, acc = fc.exact_case(m, n, k)
    sa_h, sb_h = fc.row_scales(m, 11 + cfg), fc.row_scales(n, 13 + cfg)
    sa, sb = (torch.cat([torch.full((1,), NAN), t]).cuda()[1:] for t in (sa_h, sb_h))
    assert sa.data_ptr() % 8 == 4 and sb.data_ptr() % 8 == 4
    got = _product(hip, stream, a, b, cfg, sa=sa, sb=sb, mode=fc.SCALE_ROW)
    fc.assert_bits_equal(got, fc.scaled(acc, sa_h, sb_h), f"cfg {cfg}, per-row scales")


# ---- 5. the other entry points -------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n,k,tile", [(384, 128, 256, 128), (512, 512, 256, 256)])
def test_fp8_gemm_dispatch_and_time_gemm_leave_the_product_in_c(hip, stream, m, n, k, tile):
    """``gsx_gemm_fp8_nt`` takes the 128 tile at 384 x 128 and the phased kernel at 512 x 512 (the 256 x 256
    configurations refuse the first shape); both are exact, directly and through ``gsx_event_time_gemm_fp8``."""
    a_h, b_h, acc = fc.exact_case(m, n, k)
    want = fc.scaled(acc)
    a, b = a_h.cuda(), b_h.cuda()
    if tile == 128:
        with pytest.raises(hip.HipError, match="gsx_gemm_fp8_nt_launch_cfg: need M%256==0"):
            hip.gemm_fp8_nt_cfg(stream, a.data_ptr(), b.data_ptr(), 0x1000, m, n, k, 1)
    c = _nan_c(m, n)
    _run(hip, stream, a, b, c)
    fc.assert_bits_equal(c.cpu(), want, f"gemm_fp8_nt at {m}x{n}x{k}")
    c = _nan_c(m, n)
    torch.cuda.synchronize()
    ms = hip.time_gemm_fp8(stream, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, 3)
    stream.sync()
    assert ms > 0, ms
    fc.assert_bits_equal(c.cpu(), want, f"time_gemm_fp8 at {m}x{n}x{k}")
    sa_h, sb_h = fc.row_scales(m, 21), fc.row_scales(n, 22)
    sa, sb = sa_h.cuda(), sb_h.cuda()
    c = _nan_c(m, n)
    torch.cuda.synchronize()
    hip.time_gemm_fp8(stream, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, 2, sa.data_ptr(), sb.data_ptr(),
                      fc.SCALE_ROW)
    fc.assert_bits_equal(c.cpu(), fc.scaled(acc, sa_h, sb_h), f"time_gemm_fp8 with row scales at {m}x{n}x{k}")


def test_fp8_gemm_on_a_cu_masked_stream(hip, stream):
    """``gemm_fp8_nt`` on a stream masked to CUs 0..63, the way the isolation benchmarks run it: 64 blocks, one per
    CU of the mask.  Bit-equal to the unmasked stream's result and to the reference."""
    m, n, k = 2048, 2048, 256
    a_h, b_h, acc = fc.exact_case(m, n, k)
    want = fc.scaled(acc)
    a, b = a_h.cuda(), b_h.cuda()
    out = []
    masked = hip.Stream(0, hip.mask_words(range(0, 64)))
    try:
        assert masked.mask(8)[:2] == [0xFFFFFFFF, 0xFFFFFFFF]
        for s in (stream, masked):
            c = _nan_c(m, n)
            _run(hip, s, a, b, c)
            out.append(c.cpu())
    finally:
        masked.destroy()
    fc.assert_bits_equal(out[1], out[0], "masked stream against unmasked stream")
    fc.assert_bits_equal(out[1], want, "masked stream")
    fc.assert_bits_equal(out[0], want, "unmasked stream")


# ---- 6. the longest K: the edge of the kernels' 32-bit offsets inside an operand tile ------------------------------

@pytest.mark.parametrize("cfg", [0, 1])
def test_fp8_gemm_longest_k_is_exact_and_a_longer_one_is_rejected(hip, stream, cfg):
    """One block at the largest K that the launcher accepts: the per-lane source offset of the tile's last row,
    ``(side - 1) * K + 112``, is then the largest that stays below 2^31.  The next K, 128 more, would wrap it and is
    refused.  A and B are zero but for their first and last K-tile, so the product of those 256 columns is the whole
    product; the kernel still walks all 65793 (132104 for 128 x 128) K-tiles.

    Each operand sits behind 2^32 untouched bytes of its own allocation, which is where the wrapped offset of the
    refused K would point: if the check ever went missing, that call would compute garbage and this test would fail
    on its return code, without an access outside the buffers."""
    side = TILE[cfg]
    k_ok = (2 ** 31 - 1 - 112) // (side - 1) // 128 * 128
    k_bad = k_ok + 128
    assert (side - 1) * k_ok + 112 < 2 ** 31 <= (side - 1) * k_bad + 112
    edge_a, edge_b, _ = fc.exact_case(side, side, 256)
    ops = []
    for edge in (edge_a, edge_b):
        whole = torch.empty((1 << 32) + side * k_bad, dtype=torch.uint8, device="cuda")
        t = whole[1 << 32:][:side * k_ok].view(side, k_ok)
        t.zero_()  # code 0 is +0
        t[:, :128] = edge.view(torch.uint8)[:, :128].cuda()
        t[:, k_ok - 128:] = edge.view(torch.uint8)[:, 128:].cuda()
        ops.append((whole, t.view(fc.FP8)))
    (_, a), (_, b) = ops
    want = fc.reference(edge_a, edge_b)
    assert len(set(gc.bits(want).flatten().tolist())) > 20
    c = _nan_c(side, side)
    torch.cuda.synchronize()
    with pytest.raises(hip.HipError, match="gsx_gemm_fp8_nt_launch_cfg: K too large"):
        hip.gemm_fp8_nt_cfg(stream, a.data_ptr(), b.data_ptr(), c.data_ptr(), side, side, k_bad, cfg)
    with pytest.raises(hip.HipError, match="gsx_gemm_fp8_nt: K too large"):
        hip.gemm_fp8_nt(stream, a.data_ptr(), b.data_ptr(), c.data_ptr(), side, side, k_bad)
    stream.sync()
    assert bool(torch.isnan(c).all())  # no rejected call launched anything
    _run(hip, stream, a, b, c, cfg)
    fc.assert_bits_equal(c.cpu(), want, f"cfg {cfg} at K = {k_ok}")
    del ops, a, b, c
    torch.cuda.empty_cache()
