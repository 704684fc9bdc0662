"""The MXFP4 GEMM (native/kernels/gemm_mxfp4.hip), bit for bit on a real MI355X.

Operands and the reference come from ``tests/gemm_mxfp4_cases.py``; ``tests/test_gemm_mxfp4_cases.py`` checks on the
CPU that the operands have the properties relied on here, the exactness condition first of all.  The reference
everywhere is the fp64 value of the block-scaled product rounded once to fp32 and once to bf16.  Every comparison is
on the raw 16 bits, nothing is left out and nothing has a tolerance.

Configurations 0 and 1 and the dispatching entry point (``None``) run every case.  Configuration 2 is the ablation
that takes every scale as 127: it runs the cases that tell operand paths apart, against the reference with unit
scales.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import gemm_cases as gc  # noqa: E402
from tests import gemm_mxfp4_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu

CFGS = [0, 1, 2]  # 128x128/4w, 256x256/8w-phased-g4 (dispatched), 256x256/8w-phased-g4-unit
SCALED = [0, 1, None]  # the configurations that read the scales; None: gsx_gemm_mxfp4_nt
ALL = [0, 1, 2, None]
TILE = {0: 128, 1: 256, 2: 256, None: 256}
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    from gpushare_scheduler_extender_amd.ops import hip as h

    assert h.SO.exists()
    assert hasattr(h, "gemm_mxfp4_cfgs"), "the bindings have no mxfp4 GEMM"
    assert len(h.gemm_mxfp4_cfgs()) == len(CFGS)
    for cfg in CFGS:
        bm, bn = ctypes.c_int(0), ctypes.c_int(0)
        assert h.lib().gsx_gemm_mxfp4_cfg_tile(cfg, ctypes.byref(bm), ctypes.byref(bn)) == 0
        assert bm.value == bn.value == TILE[cfg]
    return h


@pytest.fixture(scope="module")
def stream(hip):
    s = hip.Stream(0)
    yield s
    s.destroy()


def _nan_c(m, n):
    return torch.full((m, n), NAN, device="cuda", dtype=torch.bfloat16)


def _dev(x: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _run(hip, s, aq, sa, bq, sb, c, cfg=None):
    """One configuration (``cfg`` None: the dispatching entry point) on our own stream, after everything torch's
    stream did to the operands has finished."""
    (m, k2), n = aq.shape, bq.shape[0]
    k = 2 * k2
    assert bq.shape == (n, k2) and sa.shape == (m, k // 32) and sb.shape == (n, k // 32) and c.shape == (m, n)
    for t in (aq, sa, bq, sb):
        assert t.dtype == torch.uint8 and t.is_contiguous() and t.is_cuda
    assert c.dtype == torch.bfloat16 and c.is_contiguous()
    torch.cuda.synchronize()
    args = (s, aq.data_ptr(), bq.data_ptr(), c.data_ptr(), m, n, k)
    if cfg is None:
        hip.gemm_mxfp4_nt(*args, sa.data_ptr(), sb.data_ptr())
    else:
        hip.gemm_mxfp4_nt_cfg(*args, cfg, sa.data_ptr(), sb.data_ptr())
    s.sync()


def _product(hip, s, case: mc.Case, cfg=None) -> torch.Tensor:
    c = _nan_c(case.m, case.n)
    _run(hip, s, _dev(case.aq), _dev(case.sa), _dev(case.bq), _dev(case.sb), c, cfg)
    return c.cpu()


def _want(case: mc.Case, cfg) -> torch.Tensor:
    return case.want_unit if cfg == 2 else case.want


# ---- 1. K-tile counts and tile maps, exactly -----------------------------------------------------------------------

@pytest.mark.parametrize("cfg", ALL)
@pytest.mark.parametrize("k", [256, 512, 768, 1024, 1792, 32768])
@pytest.mark.parametrize("shape", ["tile", "768x512"])
def test_mxfp4_gemm_k_tile_counts_exact(hip, stream, shape, k, cfg):
    """nk = 1 (prologue only), 2, 3, 4 and 7 (buffer parity and the clamped past-the-end stages, of operands and of
    scales) and nk = 128 (a long loop), on one block and on 768 x 512: six workgroups for the 256 x 256 kernels,
    fewer than the eight XCDs the tile map remaps over, and six tile-rows for the 128 x 128 tile, whose groups of
    eight end ragged.  Random codes, random scales within the spread the exactness condition allows."""
    m, n = (TILE[cfg], TILE[cfg]) if shape == "tile" else (768, 512)
    case = mc.exact_case(m, n, k)
    mc.assert_bits_equal(_product(hip, stream, case, cfg), _want(case, cfg), f"cfg {cfg} at {m}x{n}x{k}")


# ---- 2. every e2m1 code, and the k positions of the two operand paths ----------------------------------------------

@pytest.mark.parametrize("cfg", ALL)
def test_mxfp4_gemm_code_sweep(hip, stream, cfg):
    """Each of the 16 codes at each of the 256 k positions of a K-tile, in both nibbles and both LDS buffers, against
    +-2^-1 .. 2^2: catches a wrong format select, a swapped nibble order and a wrong block scale.  Zeros are compared
    by value."""
    case = mc.code_sweep()
    mc.assert_bits_equal(_product(hip, stream, case, cfg), _want(case, cfg), f"cfg {cfg}, code sweep",
                         zeros_by_value=True)


@pytest.mark.parametrize("cfg", ALL)
def test_mxfp4_gemm_k_slots_of_a_and_b_agree(hip, stream, cfg):
    """``C[i][j]`` is nonzero only where ``i = j (mod 256)``: a k position that A's path and B's path disagree on
    shows as a named row and column."""
    case = mc.k_slot_case()
    mc.assert_bits_equal(_product(hip, stream, case, cfg), _want(case, cfg), f"cfg {cfg}, k slots")


# ---- 3. the scales ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", SCALED)
@pytest.mark.parametrize("k", [512, 1792])
def test_mxfp4_gemm_scale_slots(hip, stream, k, cfg):
    """``C[i][j] = 32 * 2^(sa[i][g_j] + sb[j][g_j] - 254)``, ``g_j = j mod (K / 32)``: every element is a power of
    two that names the scale byte its row, its column and its block really got.  A wrong byte select, a wrong
    lane-to-block map, the scales of A and B exchanged and a scale buffer left over from another K-tile all show, at
    two K-tiles (both buffers) and at seven."""
    case = mc.scale_slot_case(k)
    mc.assert_bits_equal(_product(hip, stream, case, cfg), case.want, f"cfg {cfg}, scale slots at K = {k}")


@pytest.mark.parametrize("cfg", SCALED)
def test_mxfp4_gemm_every_e8m0_code(hip, stream, cfg):
    """Every code 1 .. 254 in A's scales and in B's, paired so that the combined exponent of a dot product is the
    same in all its blocks."""
    case = mc.e8m0_sweep()
    mc.assert_bits_equal(_product(hip, stream, case, cfg), case.want, f"cfg {cfg}, e8m0 sweep")


# ---- 4. guard bands and 16-B-only alignment ------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", SCALED)
def test_mxfp4_gemm_guard_bands_and_minimum_alignment(hip, stream, cfg):
    """512 x 768 x 768 with the operands and both scale arrays 16 B past a 32-B boundary, between bands of 0x77 (two
    +6.0; A and B), 0xFE (the scales) and 0xC3C3 (C).  C starts as NaN: an element not written stays NaN, data used
    from outside an operand or a scale array changes elements, and a store outside C lands in a band."""
    case = mc.exact_case(512, 768, 768)
    wa, aq = mc.banded(case.aq, mc.A_BAND, "cuda")
    wb, bq = mc.banded(case.bq, mc.A_BAND, "cuda")
    wsa, sa = mc.banded(case.sa, mc.S_BAND, "cuda")
    wsb, sb = mc.banded(case.sb, mc.S_BAND, "cuda")
    wc, c = gc.banded(torch.full((case.m, case.n), NAN, dtype=torch.bfloat16), gc.C_BAND, "cuda")
    for t in (aq, bq, sa, sb, c):
        assert t.data_ptr() % 32 == 16
    before = [w.clone() for w in (wa, wb, wsa, wsb)]
    _run(hip, stream, aq, sa, bq, sb, c, cfg)
    for band in gc.bands_of(wc, c.numel()):
        changed = (band.to(torch.int32) & 0xFFFF) != gc.C_BAND
        assert not bool(changed.any()), f"cfg {cfg}: {int(changed.sum())} elements of a band of C were written"
    for w, w0 in zip((wa, wb, wsa, wsb), before):
        assert torch.equal(w, w0), f"cfg {cfg}: an operand, a scale array or a band of theirs was written"
    mc.assert_bits_equal(c.cpu(), case.want, f"cfg {cfg} at 512x768x768")


# ---- 5. the other entry points -------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n,k,tile", [(384, 128, 512, 128), (512, 512, 512, 256)])
def test_mxfp4_gemm_dispatch_and_time_gemm_leave_the_product_in_c(hip, stream, m, n, k, tile):
    """``gsx_gemm_mxfp4_nt`` takes the 128 tile at 384 x 128 and the phased kernel at 512 x 512 (the 256 x 256
    configurations refuse the first shape); both are exact, directly and through ``gsx_event_time_gemm_mxfp4``."""
    case = mc.exact_case(m, n, k)
    aq, sa, bq, sb = (_dev(x) for x in (case.aq, case.sa, case.bq, case.sb))
    if tile == 128:
        with pytest.raises(hip.HipError, match="gsx_gemm_mxfp4_nt_launch_cfg: need M%256==0"):
            hip.gemm_mxfp4_nt_cfg(stream, aq.data_ptr(), bq.data_ptr(), 0x1000, m, n, k, 1, sa.data_ptr(),
                                  sb.data_ptr())
    c = _nan_c(m, n)
    _run(hip, stream, aq, sa, bq, sb, c)
    mc.assert_bits_equal(c.cpu(), case.want, f"gemm_mxfp4_nt at {m}x{n}x{k}")
    c = _nan_c(m, n)
    torch.cuda.synchronize()
    ms = hip.time_gemm_mxfp4(stream, aq.data_ptr(), bq.data_ptr(), c.data_ptr(), m, n, k, 3, sa.data_ptr(),
                             sb.data_ptr())
    stream.sync()
    assert ms > 0, ms
    mc.assert_bits_equal(c.cpu(), case.want, f"time_gemm_mxfp4 at {m}x{n}x{k}")


def test_mxfp4_gemm_on_a_cu_masked_stream(hip, stream):
    """``gemm_mxfp4_nt`` on a stream masked to CUs 0..63, the way the isolation benchmarks run it: 64 blocks, one
    per CU of the mask.  Bit-equal to the unmasked stream's result and to the reference."""
    case = mc.exact_case(2048, 2048, 512)
    aq, sa, bq, sb = (_dev(x) for x in (case.aq, case.sa, case.bq, case.sb))
    out = []
    masked = hip.Stream(0, hip.mask_words(range(0, 64)))
    try:
        assert masked.mask(8)[:2] == [0xFFFFFFFF, 0xFFFFFFFF]
        for s in (stream, masked):
            c = _nan_c(case.m, case.n)
            _run(hip, s, aq, sa, bq, sb, c)
            out.append(c.cpu())
    finally:
        masked.destroy()
    mc.assert_bits_equal(out[1], out[0], "masked stream against unmasked stream")
    mc.assert_bits_equal(out[1], case.want, "masked stream")
    mc.assert_bits_equal(out[0], case.want, "unmasked stream")


# ---- 6. the longest K: the edge of the kernels' 32-bit offsets inside an operand tile ------------------------------

@pytest.mark.parametrize("cfg", [0, 1])
def test_mxfp4_gemm_longest_k_is_exact_and_a_longer_one_is_rejected(hip, stream, cfg):
    """One block at the largest K that the launcher accepts: the per-lane source offset of the tile's last row,
    ``(side - 1) * K / 2 + 112`` bytes, is then the largest that stays below 2^31.  The next K, 256 more, would wrap
    it and is refused.  A and B are zero but for their first and last K-tile, so the product of those 512 columns is
    the whole product; the kernel still walks every K-tile, and the scales of the tiles between are 127.

    Each operand sits behind 2^32 untouched bytes of its own allocation, which is where the wrapped offset of the
    refused K would point: if the check ever went missing, that call would compute garbage and this test would fail
    on its return code, without an access outside the buffers."""
    side = TILE[cfg]
    k_ok = (2 ** 31 - 1 - 112) // (side - 1) // 128 * 128 * 2
    k_bad = k_ok + 256
    assert (side - 1) * (k_ok // 2) + 112 < 2 ** 31 <= (side - 1) * (k_bad // 2) + 112
    edge = mc.exact_case(side, side, 512)
    ops = []
    for q, sc in ((edge.aq, edge.sa), (edge.bq, edge.sb)):
        whole = torch.empty((1 << 32) + side * (k_bad // 2), dtype=torch.uint8, device="cuda")
        t = whole[1 << 32:][:side * (k_ok // 2)].view(side, k_ok // 2)
        t.zero_()  # code 0 is +0
        t[:, :128] = _dev(q[:, :128])
        t[:, k_ok // 2 - 128:] = _dev(q[:, 128:])
        s = torch.full((side, k_ok // 32), 127, dtype=torch.uint8, device="cuda")
        s[:, :8] = _dev(sc[:, :8])
        s[:, k_ok // 32 - 8:] = _dev(sc[:, 8:])
        ops.append((whole, t, s))
    (_, aq, sa), (_, bq, sb) = ops
    assert len(set(gc.bits(edge.want).flatten().tolist())) > 20
    c = _nan_c(side, side)
    torch.cuda.synchronize()
    with pytest.raises(hip.HipError, match="gsx_gemm_mxfp4_nt_launch_cfg: K too large"):
        hip.gemm_mxfp4_nt_cfg(stream, aq.data_ptr(), bq.data_ptr(), c.data_ptr(), side, side, k_bad, cfg,
                              sa.data_ptr(), sb.data_ptr())
    with pytest.raises(hip.HipError, match="gsx_gemm_mxfp4_nt: K too large"):
        hip.gemm_mxfp4_nt(stream, aq.data_ptr(), bq.data_ptr(), c.data_ptr(), side, side, k_bad, sa.data_ptr(),
                          sb.data_ptr())
    stream.sync()
    assert bool(torch.isnan(c).all())  # no rejected call launched anything
    _run(hip, stream, aq, sa, bq, sb, c, cfg)
    mc.assert_bits_equal(c.cpu(), edge.want, f"cfg {cfg} at K = {k_ok}")
    del ops, aq, bq, sa, sb, c
    torch.cuda.empty_cache()
