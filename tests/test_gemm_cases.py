"""CPU checks of the GEMM test operands (tests/gemm_cases.py): conditions on the inputs that the GPU tests of
tests/test_gpu_gemm_edges.py rely on, checked here without a GPU."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import gemm_cases as gc  # noqa: E402

TINY = np.float32(2.0 ** -126)  # the smallest normal fp32


@pytest.fixture(scope="module")
def rc():
    return gc.rounding_case()


def _bf16_exact(v: np.ndarray) -> bool:
    return bool(((v.astype(np.float32).view(np.uint32) & 0xFFFF) == 0).all())


def _exact_f32(rc):
    """``x_i * s_j`` over the finite rows and columns: fp64 (exact), and the same as fp32 bit patterns."""
    v = rc.x().astype(np.float64)[:, None] * rc.s[rc.finite_cols][None, :]
    v32 = v.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), v)  # the fp64 product is an fp32 value
    return v, v32.view(np.uint32)


def test_f2bf_twin_agrees_with_torch():
    """The transcription of the kernel's conversion against ``Tensor.bfloat16()``: equal on every non-NaN value,
    NaN with the quiet bit for every NaN."""
    rng = np.random.default_rng(5)
    u = rng.integers(0, 1 << 32, size=200_000, dtype=np.uint64).astype(np.uint32)
    edge = [0x3F800000 | (hi << 16) | lo for hi in (0x00, 0x01, 0x7E, 0x7F) for lo in gc.LOW16 + gc.LOW16_NO_L]
    edge += [0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x7F800001, 0x7FC00000, 0xFFFFFFFF, 0, 1 << 31]
    u = np.concatenate([u, np.array(edge, dtype=np.uint32)])
    got = gc.f2bf_twin(u).astype(np.int32)
    want = gc.bits(torch.from_numpy(u.view(np.float32).copy()).bfloat16()).numpy()
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    assert nan.sum() > 100
    assert np.array_equal(got[~nan], want[~nan])
    assert (((got[nan] & 0x7FFF) > 0x7F80) & ((got[nan] & 0x40) != 0)).all()
    assert ((want[nan] & 0x7FFF) > 0x7F80).all()


def test_rounding_rows_hold_the_required_mantissas(rc):
    mant = set((rc.xbits[rc.finite_rows] & 0x7FFFFF).tolist())
    for lo in gc.LOW16:
        assert any(m & 0xFFFF == lo and not (m >> 16) & 1 for m in mant), hex(lo)  # under an even bit 16
        assert any(m & 0xFFFF == lo and (m >> 16) & 1 for m in mant), hex(lo)  # and an odd one
        assert (0x7F << 16) | lo in mant  # bits 16..22 all ones
    assert ((rc.xbits[rc.finite_rows] >> 23) == 0x7F).all()  # x in [1, 2)
    assert len(rc.finite_rows) == gc.ROUND_M - 5 and len(set(rc.special.values())) == 5
    assert not set(rc.special.values()) & set(rc.finite_rows.tolist())
    assert len(mant) >= 200  # the random rows did not collapse
    # the 16-bit-only subset: l == 0, with ties and near-ties of its own
    m16 = set((rc.xbits[rc.rows16] & 0x7FFFFF).tolist())
    assert len(rc.rows16) >= 64 and all(m & 0xFF == 0 for m in m16)
    assert {(hi << 16) | lo for hi in (0x00, 0x01, 0x7E, 0x7F) for lo in gc.LOW16_NO_L} <= m16


def test_rounding_pieces_are_bf16_same_sign_disjoint_and_normal(rc):
    h, m, l = rc.pieces()
    x = rc.x()
    for p in (h, m, l):
        assert _bf16_exact(p)
        assert ((p == 0) | (np.abs(p) >= np.float32(2.0 ** -23))).all()  # normal, and at least x's last bit
        assert (p >= 0).all()
    assert (h >= 1).all() and (h < 2).all()
    hb, mb, lb = (p.view(np.uint32) for p in (h, m, l))
    assert np.array_equal(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64), x.astype(np.float64))
    # disjoint bit-fields: each piece is below the last set bit of the one before it
    for hi, lo in ((h, m), (m, l), (h, l)):
        nz = (hi != 0) & (lo != 0)
        ulp_hi = np.ldexp(1.0, np.frexp(hi[nz].astype(np.float64))[1] - 8)  # a bf16 has 8 significant bits
        assert (lo[nz].astype(np.float64) < ulp_hi).all()
    assert (l[(rc.xbits[rc.finite_rows] & 0xFF) == 0] == 0).all()  # 16 significant bits need two pieces
    assert (l[np.isin(rc.finite_rows, rc.rows16)] == 0).all() and (l != 0).sum() >= 100
    assert (hb != 0).all() and (mb != 0).any() and (lb != 0).any()
    # and A holds exactly these, at k = 0, 32, 64, with +0 everywhere else
    a = rc.a.float().numpy()
    rows = rc.finite_rows
    for k, p in zip(gc.PIECE_K, (h, m, l)):
        assert np.array_equal(a[rows, k].view(np.uint32), p.view(np.uint32))
    rest = np.delete(a[rows], gc.PIECE_K, axis=1)
    assert (rest.view(np.uint32) == 0).all()
    assert len({k // 16 for k in gc.PIECE_K}) == 3 and len({k // 32 for k in gc.PIECE_K}) == 3


def test_rounding_columns_are_signed_powers_of_two_over_the_whole_range(rc):
    b = rc.b.double().numpy()
    assert (b == b[:, :1]).all()  # the same value in every k position
    s = b[:, 0]
    assert np.array_equal(s, rc.s) and s[rc.zero_col] == 0 and not np.signbit(s[rc.zero_col])
    fin = rc.finite_cols
    assert len(fin) == gc.ROUND_N - 1
    mant, _ = np.frexp(s[fin])
    assert (np.abs(mant) == 0.5).all()
    e = rc.e[fin]
    assert e.min() == gc.E_MIN and e.max() == gc.E_MAX and len(set(e.tolist())) >= 200
    for want_e in (gc.E_MIN, 0, gc.E_MAX - 1, gc.E_MAX):
        assert {1.0, -1.0} <= set(rc.sign[fin][e == want_e].tolist()), want_e
    assert (rc.sign[fin] > 0).sum() >= 100 and (rc.sign[fin] < 0).sum() >= 100
    assert s[rc.one_col] == 1.0 and s[rc.minus_one_col] == -1.0


def test_rounding_products_are_normal_and_sum_exactly_in_all_six_orders(rc):
    v, _ = _exact_f32(rc)
    s32 = rc.s[rc.finite_cols].astype(np.float32)
    prods = []
    with np.errstate(over="raise", under="raise", invalid="raise"):
        for p in rc.pieces():
            q = p[:, None] * s32[None, :]  # fp32 multiply
            assert np.array_equal(q.astype(np.float64), p.astype(np.float64)[:, None] * rc.s[rc.finite_cols][None, :])
            nz = p != 0
            assert (np.abs(q[nz]) >= TINY).all() and np.isfinite(q).all()  # all three products normal
            prods.append(q)
        assert len(gc.ORDERS) == 6
        for o in gc.ORDERS:
            acc = np.zeros_like(prods[0])  # the accumulator starts at +0
            for t in o:
                acc = acc + prods[t]  # fp32 adds
            assert acc.dtype == np.float32 and np.array_equal(acc.astype(np.float64), v), o


def test_rounding_want_is_the_single_rounding_of_x_times_s(rc):
    """The matrix product of the reference equals the elementwise construction: the zeros of a row add nothing, and
    the special rows and the zero column change only their own cells."""
    _, u = _exact_f32(rc)
    w = gc.bits(rc.want).numpy()
    cell = w[np.ix_(rc.finite_rows, rc.finite_cols)]
    assert np.array_equal(cell, gc.f2bf_twin(u).astype(np.int32))
    assert (w[rc.finite_rows, rc.zero_col] == 0).all()  # finite * 0
    s, sp = rc.s, rc.special
    fin = rc.finite_cols
    pinf, ninf = 0x7F80, 0xFF80
    assert np.array_equal(w[sp["+inf"], fin], np.where(s[fin] > 0, pinf, ninf))
    assert np.array_equal(w[sp["-inf"], fin], np.where(s[fin] > 0, ninf, pinf))
    for name in ("+inf", "-inf", "inf-inf", "nan"):
        assert (w[sp[name], rc.zero_col] & 0x7FFF) > 0x7F80  # inf * 0, nan * 0
    for name in ("inf-inf", "nan"):
        assert ((w[sp[name]] & 0x7FFF) > 0x7F80).all()
    # overflow inside the accumulation: two products of the largest finite bf16, each finite on its own
    big = float(np.array([0x7F7F0000], dtype=np.uint32).view(np.float32)[0])
    assert np.isfinite(np.float32(big * s[rc.one_col])) and w[sp["acc-overflow"], rc.one_col] == pinf
    assert w[sp["acc-overflow"], rc.minus_one_col] == ninf and w[sp["acc-overflow"], rc.zero_col] == 0
    exact = 2 * big * s[fin]
    with np.errstate(over="ignore"):
        assert np.array_equal(w[sp["acc-overflow"], fin], gc.f2bf_twin(exact.astype(np.float32).view(np.uint32)))
    # NaN nowhere else: a kernel that mixed rows or columns would spread it
    nan = (w & 0x7FFF) > 0x7F80
    allowed = np.zeros_like(nan)
    allowed[[sp["inf-inf"], sp["nan"]], :] = True
    allowed[[sp["+inf"], sp["-inf"]], rc.zero_col] = True
    assert np.array_equal(nan, allowed)


def test_rounding_want_holds_every_class_in_both_directions(rc):
    _, u = _exact_f32(rc)
    r = gc.f2bf_twin(u).astype(np.uint32)
    neg = (u >> 31) == 1
    assert ((u & 0x7F800000) != 0).all() and ((u & 0x7F800000) != 0x7F800000).all()  # no zero, subnormal, inf
    tie = (u & 0xFFFF) == 0x8000
    up = tie & (((u >> 16) & 1) == 1)
    down = tie & (((u >> 16) & 1) == 0)
    finite_out = (r & 0x7FFF) < 0x7F80
    carry = finite_out & (((r >> 7) & 0xFF) == ((u >> 23) & 0xFF) + 1)
    to_inf = (r & 0x7FFF) == 0x7F80
    sticky = ((u & 0xFF) != 0) & ((u & 0xFFFF) != 0x8000)  # bits below bit 8 that the rounding has to see
    top = r == 0x7F7F
    for name, cls, least in (("tie up", up, 64), ("tie down", down, 64), ("carry", carry, 16), ("to inf", to_inf, 8),
                             ("sticky", sticky, 64), ("tie", tie, 64)):
        assert (cls & ~neg).sum() >= least and (cls & neg).sum() >= least, (name, cls.sum())
    assert top.sum() >= 8 and (r == 0xFF7F).sum() >= 8  # the largest finite bf16, reached from below and by rounding
    assert (carry & tie).sum() >= 2 and (to_inf & tie).sum() >= 2
    # a hair below and a hair above the tie, and below the largest finite bf16's rounding boundary
    assert ((u & 0xFFFF) == 0x7FFF).sum() >= 64 and ((u & 0xFFFF) == 0x8001).sum() >= 64
    assert ((u & 0x7FFFFFFF) == 0x7F7F7FFF).sum() >= 1 and ((u & 0x7FFFFFFF) == 0x7F7F8000).sum() >= 1
    # the same classes inside the 16-bit-only subset, which does not need the third piece
    sub = np.isin(rc.finite_rows, rc.rows16)
    for cls, least in ((up, 64), (down, 64), (carry, 16), (to_inf, 8)):
        assert (cls[sub] & ~neg[sub]).sum() >= least and (cls[sub] & neg[sub]).sum() >= least
    # the whole of want: the inf and NaN cells are there, and no fp32 subnormal anywhere
    w = gc.bits(rc.want).numpy()
    assert (w == 0x7F80).sum() >= 8 and (w == 0xFF80).sum() >= 8 and ((w & 0x7FFF) > 0x7F80).sum() >= 2 * gc.ROUND_N
    with np.errstate(over="ignore", invalid="ignore"):
        f = (rc.a.double() @ rc.b.double().t()).float().numpy()
    assert not ((f != 0) & (np.abs(f) < TINY)).any()


def test_mismatches_is_bit_exact_but_for_nan_payload_and_listed_zero_columns():
    def bf(*words):
        return torch.tensor([[w - 0x10000 if w & 0x8000 else w for w in words]], dtype=torch.int16).view(torch.bfloat16)

    want = bf(0x7FC0, 0x7FC0, 0x7FC0, 0x7FC0, 0x0000, 0x0000, 0x3F80, 0x7F80)
    assert len(gc.mismatches(want, want)) == 0
    got = bf(0xFFC1, 0x7F81, 0x7F80, 0x3F80, 0x8000, 0x8000, 0x3F81, 0xFF80)
    #        ok      signalling  inf   finite  -0 listed  -0   1 ulp  wrong sign
    assert gc.mismatches(got, want, zero_by_value_cols=(4,)).tolist() == [[0, c] for c in (1, 2, 3, 5, 6, 7)]
    assert gc.mismatches(bf(0x7FC0), bf(0x3F80)).tolist() == [[0, 0]]  # a NaN where none is wanted
    assert gc.mismatches(bf(0x0001), bf(0x0000), zero_by_value_cols=(0,)).tolist() == [[0, 0]]
    with pytest.raises(AssertionError, match=r"cfg 3: 6 of 8 elements differ: \[0,1\] got 0x7f81 want 0x7fc0"):
        gc.assert_bits_equal(got, want, "cfg 3", zero_by_value_cols=(4,))


def test_banded_operand_is_16_byte_aligned_and_no_more_between_full_bands():
    a, _ = gc.exact_operands(8, 8, 24)
    whole, view = gc.banded(a, gc.BF16_QNAN, "cpu")
    assert view.data_ptr() % 32 == 16 and view.data_ptr() - whole.data_ptr() == gc.BAND + 16
    assert torch.equal(view, a) and view.is_contiguous()
    lead, trail = gc.bands_of(whole, a.numel())
    assert lead.numel() * 2 == gc.BAND + 16 and trail.numel() * 2 == gc.BAND >= 64 * 1024
    assert lead.numel() + a.numel() + trail.numel() == whole.numel()
    assert bool(torch.isnan(lead.view(torch.bfloat16)).all()) and bool(torch.isnan(trail.view(torch.bfloat16)).all())
    assert set((lead.to(torch.int32) & 0xFFFF).tolist()) == {gc.BF16_QNAN}
    whole, view = gc.banded(a, gc.C_BAND, "cpu")
    lead, trail = gc.bands_of(whole, a.numel())
    assert set((torch.cat([lead, trail]).to(torch.int32) & 0xFFFF).tolist()) == {gc.C_BAND}
    view.fill_(float("nan"))  # writing the operand leaves the bands alone
    assert set((torch.cat(gc.bands_of(whole, a.numel())).to(torch.int32) & 0xFFFF).tolist()) == {gc.C_BAND}


def test_exact_generator_stays_exact_up_to_the_longest_k():
    """Inputs are q/16; at K = 8192 the sum of the products' magnitudes stays below 2^13, so every partial sum, in
    any order, is a multiple of 2^-8 below 2^13: 21 bits, exact in fp32."""
    a, b, want = gc.exact_case(256, 256, 8192)
    for t in (a, b):
        q = t.double() * 16
        assert torch.equal(q, q.round()) and float(q.abs().max()) <= 15
    assert float((a.double().abs() @ b.double().abs().t()).max()) < 2 ** 13
    assert torch.equal((a.double() @ b.double().t()).float().double(), a.double() @ b.double().t())
    assert gc.exact_case(256, 256, 8192)[2] is want  # built once
    # different data under every tile: no two 64-wide K-tiles and no two 128-row blocks of A repeat
    a5 = gc.exact_operands(768, 1280, 320)[0]
    assert not torch.equal(a5[:128], a5[128:256]) and not torch.equal(a5[:, :64], a5[:, 64:128])
    w = gc.bits(gc.exact_case(256, 256, 448)[2])
    assert int(((w & 0x7FFF) > 0x7F80).sum()) == 0 and len(set(w.flatten().tolist())) > 200
