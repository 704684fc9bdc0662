"""The MXFP4 quantiser (``gsx_quant_mxfp4``, native/kernels/gemm_mxfp4.hip) on a real MI355X: byte for byte the NumPy
twin of ``tests/gemm_mxfp4_cases.py``, which is its definition, and end to end into the GEMM."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import gemm_mxfp4_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu

Q_BAND, S_BAND = 0xA5, 0x5A  # what the guard bands of the two outputs hold


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    from gpushare_scheduler_extender_amd.ops import hip as h

    assert h.SO.exists()
    assert hasattr(h, "quant_mxfp4"), "the bindings have no mxfp4 quantiser"
    return h


@pytest.fixture(scope="module")
def stream(hip):
    s = hip.Stream(0)
    yield s
    s.destroy()


def _quantise(hip, s, xbits: np.ndarray):
    """``(q, s)`` of the kernel as NumPy arrays; the outputs sit between guard bands that have to stay intact."""
    r, k = xbits.shape
    x = torch.from_numpy(xbits.view(np.int16)).cuda()
    wq, q = mc.banded(np.zeros((r, k // 2), dtype=np.uint8), Q_BAND, "cuda")
    ws, sc = mc.banded(np.zeros((r, k // 32), dtype=np.uint8), S_BAND, "cuda")
    q.fill_(Q_BAND)
    sc.fill_(S_BAND)
    torch.cuda.synchronize()
    hip.quant_mxfp4(s, x.data_ptr(), q.data_ptr(), sc.data_ptr(), r, k)
    s.sync()
    lead = mc.gc.BAND + 16
    for whole, n, fill in ((wq, q.numel(), Q_BAND), (ws, sc.numel(), S_BAND)):
        assert bool((whole[:lead] == fill).all()) and bool((whole[lead + n:] == fill).all()), "a band was written"
    return q.cpu().numpy(), sc.cpu().numpy()


def _assert_same(got, want, what):
    (gq, gs), (wq, ws) = got, want
    bad = np.argwhere(gs != ws)
    assert not len(bad), f"{what}: {len(bad)} scales differ, first at {bad[0]}: got {gs[tuple(bad[0])]} want " \
                         f"{ws[tuple(bad[0])]}"
    bad = np.argwhere(gq != wq)
    assert not len(bad), f"{what}: {len(bad)} bytes differ, first at {bad[0]}: got {gq[tuple(bad[0])]:#04x} want " \
                         f"{wq[tuple(bad[0])]:#04x}"


def _every_exponent() -> np.ndarray:
    """One block of 32 per bf16 exponent field 0 .. 254 and per mantissa 0, 0x40 (1.5: the last that does not
    saturate), 0x41 and 0x7F of the block's largest magnitude (field 0: subnormals, and the all-zero block).  The
    other 31 elements are ``y 2^e`` for y = 0, 1/4, .. 7 1/2, ``e`` the block's exponent: every e2m1 value, every
    midpoint between two (ties in both directions) and values on either side, every other one negative (the zeros
    too); those above the maximum are left out."""
    y = np.arange(31) * 0.25
    rows = []
    for field in range(255):
        for mant in (0x00, 0x40, 0x41, 0x7F):
            top_bits = np.uint16((field << 7) | mant)
            top = mc.bf16_values(np.array([top_bits]))[0]
            e = min(max(field - 2, 1), 254) - 127
            vals = np.where(y * 2.0 ** e <= top, y * 2.0 ** e, 0.0)
            bits = np.concatenate([mc.bf16_bits(vals), [top_bits]]).astype(np.uint16)
            bits[1::2] |= 0x8000
            rows.append(bits)
    return np.stack(rows)


def test_quantiser_is_the_twin_on_every_exponent_ties_saturation_and_zeros(hip, stream):
    x = _every_exponent()
    assert x.shape == (255 * 4, 32)
    want = mc.quant_twin(x)
    assert set(want[1].flatten().tolist()) >= set(range(1, 253))  # every scale code the format can produce
    assert set(mc.unpack(want[0]).flatten().tolist()) == set(range(16))  # every code, +0 and -0 among them
    _assert_same(_quantise(hip, stream, x), want, "every exponent, K = 32")


@pytest.mark.parametrize("r,k", [(1021, 32), (37, 8224)])
def test_quantiser_is_the_twin_on_random_rows_of_odd_counts(hip, stream, r, k):
    """Random bf16 words of every exponent (inf and NaN fields excluded), with blocks of all zeros and blocks of one
    value among zeros, R a prime and K = 32 (one block a row) and 8224 = 257 blocks."""
    rng = np.random.default_rng([r, k])
    x = rng.integers(0, 1 << 16, size=(r, k), dtype=np.uint16)
    x = np.where((x & 0x7F80) == 0x7F80, x & 0x807F, x).astype(np.uint16)
    blocks = x.reshape(r, k // 32, 32)
    kind = rng.integers(0, 8, size=blocks.shape[:2])
    blocks[kind == 0] = 0
    blocks[kind == 1] &= 0x8000  # zeros of both signs
    blocks[kind == 2, 1:] = 0
    # a narrow range of exponents in the other blocks, so that elements land all over the grid
    narrow = (blocks & 0x807F) | (((blocks >> 7) & 3) + 120 << 7)
    blocks[kind >= 5] = narrow[kind >= 5]
    x = blocks.reshape(r, k)
    want = mc.quant_twin(x)
    assert set(mc.unpack(want[0]).flatten().tolist()) == set(range(16))
    _assert_same(_quantise(hip, stream, x), want, f"random words, {r} x {k}")


def test_quantised_lossless_inputs_give_the_exact_product(hip, stream):
    """bf16 inputs that quantise without loss (e2m1 values times per-block powers of two), quantised on the GPU and
    multiplied there: C is the bf16 of the fp64 product of the bf16 inputs, bit for bit."""
    m, n, k = 256, 384, 1024
    xa, ca, sa = mc.lossless_inputs(m, k, 1)
    xb, cb, sb = mc.lossless_inputs(n, k, 2)
    qa, qsa = _quantise(hip, stream, xa)
    qb, qsb = _quantise(hip, stream, xb)
    _assert_same((qa, qsa), (mc.pack(ca), sa), "A")
    _assert_same((qb, qsb), (mc.pack(cb), sb), "B")
    want = (torch.from_numpy(mc.bf16_values(xa)) @ torch.from_numpy(mc.bf16_values(xb)).t()).float().bfloat16()
    dev = [torch.from_numpy(t).cuda() for t in (qa, qb, qsa, qsb)]
    c = torch.full((m, n), float("nan"), device="cuda", dtype=torch.bfloat16)
    torch.cuda.synchronize()
    hip.gemm_mxfp4_nt(stream, dev[0].data_ptr(), dev[1].data_ptr(), c.data_ptr(), m, n, k, dev[2].data_ptr(),
                      dev[3].data_ptr())
    stream.sync()
    mc.assert_bits_equal(c.cpu(), want, "quantise, then multiply")
