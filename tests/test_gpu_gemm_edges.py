"""The bf16 GEMM (native/kernels/gemm.hip) on the edges of what ``launch()`` accepts, bit for bit on a real MI355X.

Operands, the reference and the comparison come from ``tests/gemm_cases.py``; ``tests/test_gemm_cases.py`` checks
on the CPU that the operands have the properties relied on here.  The reference everywhere is the fp64 product on
the CPU rounded once to fp32 and once to bf16, and every comparison is on the raw 16 bits: a NaN has to be a quiet
NaN (any sign and payload), everything else has to be bit-equal, nothing is left out and nothing has a tolerance.
"""
import random

import pytest

torch = pytest.importorskip("torch")

from tests import gemm_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu

CFGS = list(range(11))
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    from gpushare_scheduler_extender_amd.ops import hip as h

    assert h.SO.exists()
    assert len(h.gemm_cfgs()) == len(CFGS)
    return h


@pytest.fixture(scope="module")
def stream(hip):
    s = hip.Stream(0)
    yield s
    s.destroy()


def _run_cfg(hip, s, a, b, c, cfg):
    """One configuration on our own stream, after everything torch's stream did to the operands has finished."""
    (m, k), n = a.shape, b.shape[0]
    assert b.shape[1] == k and c.shape == (m, n) and a.is_contiguous() and b.is_contiguous() and c.is_contiguous()
    torch.cuda.synchronize()
    hip.gemm_bf16_nt_cfg(s, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, cfg)
    s.sync()


def _banded_run(hip, s, a_h, b_h, cfg):
    """The configuration on operands that are 16-B aligned and no more, each between two guard bands of at least
    64 KiB: NaN around A and B, 0xC3C3 around C, C itself prefilled with NaN.  Returns C on the host after checking
    that the bands of C, and A and B with theirs, are unchanged."""
    wa, a = gc.banded(a_h, gc.BF16_QNAN, "cuda")
    wb, b = gc.banded(b_h, gc.BF16_QNAN, "cuda")
    wc, c = gc.banded(torch.full((a_h.shape[0], b_h.shape[0]), NAN, dtype=torch.bfloat16), gc.C_BAND, "cuda")
    for t in (a, b, c):
        assert t.data_ptr() % 32 == 16
    wa0, wb0 = wa.clone(), wb.clone()
    _run_cfg(hip, s, a, b, c, cfg)
    for band in gc.bands_of(wc, c.numel()):
        changed = (band.to(torch.int32) & 0xFFFF) != gc.C_BAND
        assert not bool(changed.any()), f"cfg {cfg}: {int(changed.sum())} elements of a band of C were written"
    assert torch.equal(wa, wa0) and torch.equal(wb, wb0), f"cfg {cfg}: A or B, or a band of theirs, was written"
    return c.cpu()


# ---- 1. epilogue rounding ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rounding_results(hip, stream):
    """Each configuration's C for the rounding case, computed once and shared by the two tests below."""
    rc, done = gc.rounding_case(), {}

    def get(cfg):
        if cfg not in done:
            a, b = rc.a.cuda(), rc.b.cuda()
            c = torch.full((gc.ROUND_M, gc.ROUND_N), NAN, device="cuda", dtype=torch.bfloat16)
            _run_cfg(hip, stream, a, b, c, cfg)
            done[cfg] = c.cpu()
        return done[cfg]
    return get


@pytest.mark.parametrize("cfg", CFGS)
def test_gemm_epilogue_rounding_16_bit_values(rounding_results, cfg):
    """Rows whose x has 16 significant bits (pieces h and m only, l == 0) against every finite column: ties under an
    even and an odd last bit, near-ties, carries into the exponent, the largest finite bf16 and finite values that
    round to inf, with both signs.  A sum of two pieces needs one exact add of an 8-bit value to an 8-bit value, so a
    failure here is a failure of the conversion ``f2bf`` (or of the data path), not of the MFMA's adder."""
    rc = gc.rounding_case()
    got, want = rounding_results(cfg), rc.want
    rows = torch.from_numpy(rc.rows16)
    gc.assert_bits_equal(got[rows], want[rows], f"cfg {cfg}, 16-bit rows {rc.rows16.tolist()}",
                         zero_by_value_cols=(rc.zero_col,))


@pytest.mark.parametrize("cfg", CFGS)
def test_gemm_epilogue_rounding_any_fp32_value(rounding_results, cfg):
    """256 x 256 x 128, ``C[i][j] = bf16(x_i * s_j)``: 24-bit values x in [1, 2) pushed through the accumulator as three
    bf16 pieces in three different MFMA instructions, scaled by +-2^e with e from -103 to 127.  Covers sticky bits
    below bit 8, ties, the carry into the exponent, finite values that round to inf, +-inf, inf - inf and inf * 0
    (NaN), a NaN operand and overflow inside the fp32 accumulation; the special rows and the zero column must change
    their own cells only.  In the zero column a zero is compared by value (the sign of a zero sum of zero products
    is not specified here); everything else is bit-exact.

    Relies on "C + one exactly representable product is exact" in the MFMA's accumulate.  Unmeasured and not used:
    bf16-subnormal inputs and fp32-subnormal products or sums (how gfx950's bf16 MFMA treats them is not in the
    guides and has not been measured; the workload never produces them)."""
    rc = gc.rounding_case()
    gc.assert_bits_equal(rounding_results(cfg), rc.want, f"cfg {cfg}", zero_by_value_cols=(rc.zero_col,))


# ---- 2. guard bands and 16-B-only alignment ------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("m,n,k", [(512, 768, 192), (1024, 512, 192)])
def test_gemm_guard_bands_and_minimum_alignment(hip, stream, m, n, k, cfg):
    """512 x 768 (6 blocks of 256 x 256: fewer than the 8 XCDs) and 1024 x 512 (8, 16 or 32 blocks: whole multiples
    of 8), three K-tiles.  Any use of data outside A or B turns into a NaN in C, any element of C not written stays
    NaN, and a store outside C lands in a band."""
    a_h, b_h, want = gc.exact_case(m, n, k)
    got = _banded_run(hip, stream, a_h, b_h, cfg)
    gc.assert_bits_equal(got, want, f"cfg {cfg} at {m}x{n}x{k}")


# ---- 3. K-tile counts, exactly -------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("k", [64, 128, 192, 256, 448, 8192])
def test_gemm_k_tile_counts_exact(hip, stream, k, cfg):
    """One block, nk = 1, 2, 3, 4 and 7 (prologue, buffer parity and the clamped prefetch of the pipelined kernels)
    and nk = 128 (many reuses of both LDS buffers).  Operands sit between NaN bands like in the test above."""
    a_h, b_h, want = gc.exact_case(256, 256, k)
    got = _banded_run(hip, stream, a_h, b_h, cfg)
    gc.assert_bits_equal(got, want, f"cfg {cfg} at K = {k}")


# ---- 5. the two entry points nobody checked -------------------------------------------------------------------------

@pytest.mark.parametrize("m,n,k", [(512, 512, 128), (384, 128, 64)])
def test_time_gemm_leaves_the_product_in_c(hip, stream, m, n, k):
    """``gsx_event_time_gemm`` with both dispatch targets (phased 256 x 256, grouped 128 x 128): a positive time,
    and C holds the product afterwards."""
    a_h, b_h, want = gc.exact_case(m, n, k)
    a, b = a_h.cuda(), b_h.cuda()
    c = torch.full((m, n), NAN, device="cuda", dtype=torch.bfloat16)
    torch.cuda.synchronize()
    ms = hip.time_gemm(stream, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, 3)
    stream.sync()
    assert ms > 0, ms
    gc.assert_bits_equal(c.cpu(), want, f"time_gemm at {m}x{n}x{k}")


@pytest.mark.parametrize("m,n,k", [(2048, 2048, 256), (4096, 2048, 256)])
def test_gemm_on_a_cu_masked_stream(hip, stream, m, n, k):
    """``gemm_bf16_nt`` on a stream masked to CUs 0..63, the way the isolation benchmarks run it: 64 blocks (one per
    CU of the mask) and 128 blocks (two rounds).  Bit-equal to the unmasked stream's result and to the reference."""
    a_h, b_h, want = gc.exact_case(m, n, k)
    a, b = a_h.cuda(), b_h.cuda()
    out = []
    masked = hip.Stream(0, hip.mask_words(range(0, 64)))
    try:
        assert masked.mask(8)[:2] == [0xFFFFFFFF, 0xFFFFFFFF]
        for s in (stream, masked):
            c = torch.full((m, n), NAN, device="cuda", dtype=torch.bfloat16)
            torch.cuda.synchronize()
            hip.gemm_bf16_nt(s, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k)
            s.sync()
            out.append(c.cpu())
    finally:
        masked.destroy()
    gc.assert_bits_equal(out[1], out[0], "masked stream against unmasked stream")
    gc.assert_bits_equal(out[1], want, "masked stream")
    gc.assert_bits_equal(out[0], want, "unmasked stream")


# ---- 4. offsets past 2^31 elements (last: these allocate more than 4 GiB each) ----------------------------------------

BIG_CFGS = (0, 3, 5, 7)  # one per kernel template and tile size
TILE = 256  # regions compared are 256 x 256 and 256-aligned: one tile of the large configurations, four of cfg 0


def _device_small_ints(rows, cols, seed):
    """``rows x cols`` integers in [-3, 3] as bf16, generated on the device in pieces of at most 2^28 elements."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    out = torch.empty((rows, cols), dtype=torch.bfloat16, device="cuda")
    step = max(1, (1 << 28) // cols)
    for r in range(0, rows, step):
        blk = out[r:r + step]
        blk.copy_(torch.randint(-3, 4, blk.shape, dtype=torch.int8, device="cuda", generator=g))
    return out


def _has_nan(c):
    step = max(1, (1 << 28) // c.shape[1])
    return any(bool(torch.isnan(c[r:r + step]).any()) for r in range(0, c.shape[0], step))


def _check_big(hip, s, a, b, regions):
    """Every configuration of BIG_CFGS on ``a``, ``b``: no NaN left anywhere in a NaN-prefilled C, and the listed
    256 x 256 regions ``(row0, col0)`` bit-equal to the CPU reference, which is computed once."""
    (m, k), n = a.shape, b.shape[0]
    assert 3 * 3 * k < 1 << 18  # |sum| < 2^18: every partial sum is an integer that fp32 holds exactly
    assert len(set(regions)) == len(regions) and all(r % TILE == 0 and r + TILE <= m and c % TILE == 0 and c + TILE <= n
                                                     for r, c in regions)
    want = {(r, c): gc.reference(a[r:r + TILE], b[c:c + TILE]) for r, c in regions}
    c_dev = torch.empty((m, n), dtype=torch.bfloat16, device="cuda")
    for cfg in BIG_CFGS:
        c_dev.fill_(NAN)
        _run_cfg(hip, s, a, b, c_dev, cfg)
        assert not _has_nan(c_dev), f"cfg {cfg}: elements of C were not written, or NaN was computed"
        for (r, c), w in want.items():
            gc.assert_bits_equal(c_dev[r:r + TILE, c:c + TILE].cpu(), w, f"cfg {cfg}, region at ({r}, {c})")
    del c_dev


def _between(rng, count, lo, hi):
    """``count`` distinct multiples of TILE in ``(lo, hi)``, drawn with the fixed-seed ``rng``."""
    return [t * TILE for t in rng.sample(range(lo // TILE + 1, hi // TILE), count)]


def test_gemm_large_a_past_2_to_31_elements(hip, stream):
    """A is 131328 x 16384 (4.3 GB): row 131072 starts at element 2^31, so the last 256 rows lie past it and the 256
    before them end at it."""
    m, n, k = 131328, 256, 16384
    assert (m - TILE) * k == 1 << 31
    a, b = _device_small_ints(m, k, 41), _device_small_ints(n, k, 42)
    rows = [0, m - 2 * TILE, m - TILE] + _between(random.Random(43), 8, 0, m - 2 * TILE)
    _check_big(hip, stream, a, b, [(r, 0) for r in rows])
    del a, b
    torch.cuda.empty_cache()


def test_gemm_large_b_past_2_to_31_elements(hip, stream):
    """The same with M and N swapped: B is 131328 x 16384, its last 256 rows (the last columns of C) past 2^31."""
    m, n, k = 256, 131328, 16384
    assert (n - TILE) * k == 1 << 31
    a, b = _device_small_ints(m, k, 44), _device_small_ints(n, k, 45)
    cols = [0, n - 2 * TILE, n - TILE] + _between(random.Random(46), 8, 0, n - 2 * TILE)
    _check_big(hip, stream, a, b, [(0, c) for c in cols])
    del a, b
    torch.cuda.empty_cache()


def test_gemm_large_c_past_2_to_31_elements(hip, stream):
    """C is 46592 x 46592 (2.17 * 10^9 elements), one K-tile.  Element 2^31 of C is the first column of the tile at
    (46080, 11776), in its row 46091: that tile straddles it, the tile to its left ends just before it."""
    m = n = 46592
    k = 64
    row, col = divmod(1 << 31, n)
    r0, c0 = row // TILE * TILE, col // TILE * TILE
    assert (r0, c0) == (46080, 11776) and r0 < row < r0 + TILE and col == c0
    a, b = _device_small_ints(m, k, 47), _device_small_ints(n, k, 48)
    rng = random.Random(49)
    regions = [(0, 0), (r0, c0 - TILE), (r0, c0), (m - TILE, n - TILE)]
    regions += list(zip(_between(rng, 8, 0, m - TILE), _between(rng, 8, 0, n - TILE)))
    _check_big(hip, stream, a, b, regions)
    del a, b
    torch.cuda.empty_cache()


# ---- the longest K: the edge of the kernels' 32-bit offsets inside an operand tile ------------------------------------

@pytest.mark.parametrize("cfg", BIG_CFGS)
def test_gemm_longest_k_is_exact_and_a_longer_one_is_rejected(hip, stream, cfg):
    """One block at the largest K that ``launch()`` accepts: the per-lane source offset of the tile's last row,
    ``(side - 1) * K + 56`` with ``side = max(BM, BN)``, is then the largest that stays below 2^31.  The next K, 64
    more, would wrap it and is refused.  A and B are zero but for their first and last K-tile (small integers), so
    the product of those 128 columns is the whole product; the kernel still walks all 131586 (264208 for
    128 x 128) K-tiles.

    Each operand sits behind 2^32 untouched elements of its own allocation, which is where the wrapped offset of
    the refused K would point: if the check ever went missing, that call would compute garbage and this test would
    fail on its return code, without an access outside the buffers."""
    import ctypes

    bm, bn = ctypes.c_int(0), ctypes.c_int(0)
    assert hip.lib().gsx_gemm_cfg_tile(cfg, ctypes.byref(bm), ctypes.byref(bn)) == 0
    m, n, side = bm.value, bn.value, max(bm.value, bn.value)
    k_ok = (2 ** 31 - 1 - 56) // (side - 1) // 64 * 64
    k_bad = k_ok + 64
    assert (side - 1) * k_ok + 56 < 2 ** 31 <= (side - 1) * k_bad + 56
    g = torch.Generator(device="cuda")
    g.manual_seed(50 + cfg)
    ops = []
    for rows in (m, n):
        whole = torch.empty((1 << 32) + rows * k_bad, dtype=torch.bfloat16, device="cuda")
        t = whole[1 << 32:][:rows * k_ok].view(rows, k_ok)
        t.zero_()
        for cols in (slice(0, 64), slice(k_ok - 64, k_ok)):
            t[:, cols] = torch.randint(-3, 4, (rows, 64), dtype=torch.int8, device="cuda", generator=g).bfloat16()
        ops.append((whole, t))
    (_, a), (_, b) = ops
    want = gc.reference(torch.cat([a[:, :64], a[:, k_ok - 64:]], dim=1), torch.cat([b[:, :64], b[:, k_ok - 64:]], dim=1))
    assert len(set(gc.bits(want).flatten().tolist())) > 20
    c = torch.full((m, n), NAN, device="cuda", dtype=torch.bfloat16)
    torch.cuda.synchronize()
    with pytest.raises(hip.HipError, match="gsx_gemm_bf16_nt_launch_cfg: K too large"):
        hip.gemm_bf16_nt_cfg(stream, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k_bad, cfg)
    if cfg in (0, 5):  # the two rows the dispatching entry point uses
        with pytest.raises(hip.HipError, match="gsx_gemm_bf16_nt: K too large"):
            hip.gemm_bf16_nt(stream, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k_bad)
    stream.sync()
    assert bool(torch.isnan(c).all())  # no rejected call launched anything
    _run_cfg(hip, stream, a, b, c, cfg)
    gc.assert_bits_equal(c.cpu(), want, f"cfg {cfg} at K = {k_ok}")
    del ops, a, b, c
    torch.cuda.empty_cache()
