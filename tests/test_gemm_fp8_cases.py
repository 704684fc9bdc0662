"""CPU checks for the fp8 GEMM (native/kernels/gemm_fp8.hip): the properties of the operands of
tests/gemm_fp8_cases.py that tests/test_gpu_gemm_fp8.py relies on, what the library's entry points reject before
they touch a device, and the tools' ``--dtype`` option.  No GPU is opened."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import gemm_cases as gc  # noqa: E402
from tests import gemm_fp8_cases as fc  # noqa: E402

TINY = 2.0 ** -126  # the smallest normal fp32


def _is_bf16(v: torch.Tensor) -> torch.Tensor:
    return (v.float().contiguous().view(torch.int32) & 0xFFFF) == 0


# ---- the operands --------------------------------------------------------------------------------------------------

def test_every_e4m3_code_survives_the_round_trip_and_the_two_nan_codes_are_the_only_specials():
    c = fc.from_codes(np.arange(256))
    v = c.double()
    assert torch.equal(fc.codes(v.to(fc.FP8))[~torch.isnan(v)], torch.arange(256, dtype=torch.int32)[~torch.isnan(v)])
    assert torch.isnan(v).nonzero().flatten().tolist() == list(fc.NAN_CODES)
    assert not bool(torch.isinf(v).any()) and float(v[~torch.isnan(v)].abs().max()) == 448.0  # OCP e4m3fn, not fnuz
    assert float(v[0x08]) == 2.0 ** -6 and float(v[0x01]) == 2.0 ** -9 and float(v[0x80]) == 0.0


def test_exact_generator_is_the_bf16_one_and_e4m3_holds_it():
    a, b = fc.exact_operands(128, 128, 1024)
    a16, b16 = gc.exact_operands(128, 128, 1024)
    assert torch.equal(a.double(), a16.double()) and torch.equal(b.double(), b16.double())
    for t in (a, b):
        q = t.double() * 16
        assert torch.equal(q, q.round()) and float(q.abs().max()) <= 15
        assert torch.equal(t.double().to(fc.FP8).double(), t.double())  # the round trip is the identity


def test_exact_generator_sums_exactly_and_needs_the_rounding_to_bf16():
    """Products are multiples of 2^-8 below 1, so a partial sum in any order is a multiple of 2^-8 below K: 24 bits
    at K = 2^16.  At 128 x 128 x 1024 some 45 % of the outputs are no bf16 values: the epilogue has to round them."""
    a, b, acc = fc.exact_case(128, 128, 1024)
    exact = a.double() @ b.double().t()
    assert torch.equal(acc.double(), exact)
    assert float((a.double().abs() @ b.double().abs().t()).max()) < 1024
    assert torch.equal(exact * 256, (exact * 256).round())
    a, b, acc = fc.exact_case(256, 256, 16384)  # the longest K of the GPU tests
    assert torch.equal(acc.double(), a.double() @ b.double().t())
    assert float((a.double().abs() @ b.double().abs().t()).max()) * 256 < 2 ** 24
    need = 1.0 - float(_is_bf16(fc.exact_case(128, 128, 1024)[2]).double().mean())
    assert 0.40 < need < 0.50, need
    assert fc.exact_case(128, 128, 1024)[2] is fc.exact_case(128, 128, 1024)[2]  # built once


def test_code_sweep_holds_every_code_at_every_k_position_against_every_exponent():
    a, b, want = fc.code_sweep()
    ac = fc.codes(a)
    assert ac.shape == (256, 256) and b.shape == (256, 256)
    assert sorted(int(ac[i].max()) for i in range(256)) == list(range(256))  # all 256 codes are there
    ks = [fc.sweep_k_of_row(i) for i in range(256)]
    assert sorted(ks) == list(range(256)) and {k % 128 for k in ks} == set(range(128))  # both tiles, every position
    for i in range(256):
        row = ac[i].clone()
        assert int(row[ks[i]]) == i
        row[ks[i]] = 0
        assert not bool(row.any())  # +0 everywhere else
    bv = b.double()
    assert bool((bv == bv[:, :1]).all())  # the same value at every k
    s = bv[:, 0]
    mant, e = np.frexp(s.numpy())
    assert (np.abs(mant) == 0.5).all() and set((e - 1).tolist()) == set(fc.SWEEP_E) == set(range(-9, 9))
    for ex in fc.SWEEP_E:
        assert {1.0, -1.0} <= set(np.sign(s.numpy()[(e - 1) == ex]).tolist())  # both signs of every power
    sub = fc.codes(b[:, 0])[torch.from_numpy((e - 1) < -6)] & 0x78
    assert len(sub) >= 3 * 2 and not bool(sub.any())  # 2^-9, 2^-8, 2^-7 are stored as e4m3 subnormals


def test_code_sweep_products_are_bf16_values_and_nan_stays_in_its_rows():
    a, b, want = fc.code_sweep()
    acc = fc.accumulator(a, b)
    nan_rows = torch.isnan(acc).all(dim=1)
    assert nan_rows.nonzero().flatten().tolist() == list(fc.NAN_CODES)
    assert not bool(torch.isnan(acc[~nan_rows]).any())
    fin = acc[~nan_rows]
    val = fc.from_codes(np.arange(256)).double()[~nan_rows]
    assert torch.equal(fin.double(), val[:, None] * b.double()[:, 0][None, :])  # code i times column j's power
    assert bool(_is_bf16(fin).all())
    assert not bool(((fin != 0) & (fin.abs() < TINY)).any())
    assert torch.equal(gc.bits(want[~nan_rows]), gc.bits(fin.bfloat16()))
    assert int((fin == 0).all(dim=1).sum()) == 2  # the codes of +0 and -0
    # an fnuz reading of the same bytes is another matrix: half the value, and 0x80 is NaN there
    assert float(fc.from_codes([0x38]).double()) == 1.0
    assert float(torch.as_tensor(np.array([0x38], dtype=np.uint8)).view(torch.float8_e4m3fnuz).double()) == 0.5


def test_k_slot_case_has_one_entry_per_row_and_names_row_and_column():
    a, b, want = fc.k_slot_case()
    assert a.shape == (512, 256) and b.shape == (512, 256)
    for t in (a, b):
        nz = t.double() != 0
        assert bool((nz.sum(dim=1) == 1).all())
        assert torch.equal(nz.double().argmax(dim=1), torch.arange(512) % 256)
        assert float(t.double().min()) == 0.0 and not bool((fc.codes(t) == 0x80).any())  # positive values and +0
    u, v = a.double().sum(dim=1), b.double().sum(dim=1)
    assert len(set(u.tolist())) == 15 and len(set(v.tolist())) == 13
    w = want.double()
    i, j = torch.arange(512)[:, None], torch.arange(512)[None, :]
    diag = (i % 256) == (j % 256)
    assert torch.equal(w, torch.where(diag, u[:, None] * v[None, :], torch.zeros(()).double()))  # exact in bf16
    assert bool((w[diag] != 0).all()) and not bool((gc.bits(want)[~diag] != 0).any())
    # the entries tell rows and columns apart: the pairs (u_i, v_j) of one k position differ along the diagonals
    assert len({(float(u[r]), float(v[r])) for r in range(256)}) >= 100


def test_row_scales_have_full_mantissas_both_signs_and_the_stated_range():
    s = fc.row_scales(768, 3)
    assert s.dtype == torch.float32 and s.shape == (768,)
    bits = s.view(torch.int32)
    assert int(((bits & 0xFF) != 0).sum()) > 700  # the low mantissa byte is in use: products are not fp32-exact
    assert 300 < int((s < 0).sum()) < 468
    assert float(s.abs().min()) >= 2.0 ** -4 and float(s.abs().max()) < 2.0 ** 4
    assert torch.equal(fc.row_scales(768, 3), s) and not torch.equal(fc.row_scales(768, 4), s)
    # results stay normal: |acc| is 0 or at least 2^-8, the scales at least 2^-4 each
    a, b, acc = fc.exact_case(128, 128, 1024)
    sa, sb = fc.row_scales(128, 5), fc.row_scales(128, 6)
    out = (acc * sa.reshape(-1, 1)) * sb.reshape(1, -1)
    assert not bool(((out != 0) & (out.abs() < TINY)).any()) and bool(torch.isfinite(out).all())
    want = fc.scaled(acc, sa, sb)
    assert torch.equal(gc.bits(want), gc.bits(out.bfloat16()))
    # the order of the two multiplies shows in fp32 (the rounding to bf16 hides most of it, not all in general)
    other = acc * (sa.reshape(-1, 1) * sb.reshape(1, -1))
    assert int((other != out).sum()) > 1000
    assert torch.equal(gc.bits(fc.scaled(acc)), gc.bits(fc.scaled(acc, torch.ones(1), torch.ones(1))))


def test_zeros_by_value_accepts_a_zero_of_either_sign_only_where_a_zero_is_wanted():
    def bf(*words):
        return torch.tensor([[w - 0x10000 if w & 0x8000 else w for w in words]], dtype=torch.int16).view(torch.bfloat16)

    want = bf(0x0000, 0x8000, 0x3F80, 0x7FC0)
    fc.assert_bits_equal(bf(0x8000, 0x0000, 0x3F80, 0xFFC1), want, zeros_by_value=True)
    with pytest.raises(AssertionError, match="2 of 4 elements differ"):
        fc.assert_bits_equal(bf(0x8000, 0x0000, 0x3F80, 0x7FC0), want)
    with pytest.raises(AssertionError, match=r"\[0,2\] got 0x0000 want 0x3f80"):
        fc.assert_bits_equal(bf(0x0000, 0x8000, 0x0000, 0x7FC0), want, zeros_by_value=True)


def test_banded_fp8_operand_is_16_byte_aligned_and_no_more_between_nan_bands():
    a, _ = fc.exact_operands(8, 8, 128)
    whole, view = fc.banded(a, "cpu")
    assert view.data_ptr() % 32 == 16 and view.data_ptr() - whole.data_ptr() == gc.BAND + 16
    assert torch.equal(fc.codes(view), fc.codes(a))
    lead, trail = whole[:gc.BAND + 16], whole[gc.BAND + 16 + a.numel():]
    assert trail.numel() == gc.BAND and set(lead.tolist()) | set(trail.tolist()) == {fc.FP8_NAN}
    assert bool(torch.isnan(lead.view(fc.FP8).float()).all())


# ---- the library's host code (no GPU is opened) ---------------------------------------------------------------------

FP8_CFGS = {0: ("128x128/4w", 128, 128), 1: ("256x256/8w-phased-g4", 256, 256),
            2: ("256x256/8w-phased-g4-mfma32", 256, 256)}


@pytest.fixture(scope="module")
def hip():
    from gpushare_scheduler_extender_amd.ops import hip as h

    h.lib()
    return h


def test_fp8_config_table_has_its_three_rows_and_the_bf16_table_keeps_eleven(hip):
    L = hip.lib()
    assert hip.gemm_fp8_cfgs() == {c: row[0] for c, row in FP8_CFGS.items()}
    for c in (-1, 3, 11):
        assert L.gsx_gemm_fp8_cfg_name(c) is None
        bm, bn = ctypes.c_int(0), ctypes.c_int(0)
        assert L.gsx_gemm_fp8_cfg_tile(c, ctypes.byref(bm), ctypes.byref(bn)) != 0
    for c, (_, m, n) in FP8_CFGS.items():
        bm, bn = ctypes.c_int(0), ctypes.c_int(0)
        assert L.gsx_gemm_fp8_cfg_tile(c, ctypes.byref(bm), ctypes.byref(bn)) == 0 and (bm.value, bn.value) == (m, n)
    assert len(hip.gemm_cfgs()) == 11 and hip.gemm_cfgs()[5] == "256x256/8w-phased-g4"


# Addresses that are never dereferenced: every call below is refused before the first device call.
A, B, C, SA, SB = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000


class _NoStream:
    """Stands in for ``hip.Stream``: the calls under test never get as far as using one."""
    handle = None


def _rejects(hip, text, *, cfg=None, m=256, n=256, k=256, a=A, b=B, c=C, sa=0, sb=0, mode=0):
    entry = "gsx_gemm_fp8_nt" if cfg is None else "gsx_gemm_fp8_nt_launch_cfg"
    with pytest.raises(hip.HipError, match=f"{entry}: {text}"):
        if cfg is None:
            hip.gemm_fp8_nt(_NoStream, a, b, c, m, n, k, sa, sb, mode)
        else:
            hip.gemm_fp8_nt_cfg(_NoStream, a, b, c, m, n, k, cfg, sa, sb, mode)


@pytest.mark.parametrize("cfg", [None, 0, 1, 2])
def test_fp8_entry_points_reject_bad_arguments_by_name(hip, cfg):
    def rej(text, **kw):
        _rejects(hip, text, cfg=cfg, **kw)

    tile = 128 if cfg in (None, 0) else 256
    shape = "need M%128==0, N%128==0, K%128==0" if cfg is None else f"need M%{tile}==0, N%{tile}==0, K%128==0"
    rej(shape, k=192)  # K % 128
    rej(shape, k=64)
    rej(shape, m=tile + 64)  # M % BM
    rej(shape, n=tile // 2)
    rej(shape, k=0)
    if cfg is not None and tile == 256:
        rej(shape, m=384)  # fine for the dispatching entry point, which takes the 128 tile then
    for name in ("a", "b", "c"):
        rej("operands must be 16-B aligned", **{name: A + 8})
    for mode in (fc.SCALE_TENSOR, fc.SCALE_ROW):
        rej("scale_a and scale_b must not be NULL", mode=mode, sa=0, sb=SB)
        rej("scale_a and scale_b must not be NULL", mode=mode, sa=SA, sb=0)
        rej("scale_a and scale_b must be 4-B aligned", mode=mode, sa=SA + 2, sb=SB)
        rej("scale_a and scale_b must be 4-B aligned", mode=mode, sa=SA, sb=SB + 1)
    for mode in (-1, 3, 7):
        rej(f"unknown scale_mode {mode}", mode=mode, sa=SA, sb=SB)
    # one K-tile past the longest K: the 32-bit offset of the tile's last row would wrap
    side = 256 if cfg is None else tile
    k_ok = (2 ** 31 - 1 - 112) // (side - 1) // 128 * 128
    assert (side - 1) * k_ok + 112 < 2 ** 31 <= (side - 1) * (k_ok + 128) + 112
    assert k_ok == {256: 8421504, 128: 16909312}[side]  # what gsx_kernels.h documents
    rej("K too large", m=side, n=side, k=k_ok + 128)


def test_fp8_unknown_config_is_rejected_by_name(hip):
    for cfg in (-1, 3, 5):
        _rejects(hip, "unknown config", cfg=cfg)


# ---- the tools -----------------------------------------------------------------------------------------------------

def test_workload_and_isolation_parsers_take_dtype_and_default_to_bf16():
    from gsxtools import isolation, workload

    for mod in (workload, isolation):
        ap = mod.build_parser()
        assert ap.parse_args([]).dtype == "bf16"
        assert ap.parse_args(["--dtype", "fp8"]).dtype == "fp8"
        assert ap.parse_args(["--dtype", "bf16"]).dtype == "bf16"
        with pytest.raises(SystemExit):
            ap.parse_args(["--dtype", "fp4"])
