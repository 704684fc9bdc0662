"""CPU checks for the MXFP4 GEMM and its quantiser (native/kernels/gemm_mxfp4.hip): the properties of the operands of
tests/gemm_mxfp4_cases.py that the GPU tests rely on (the exactness condition first), the quantiser's NumPy twin, what
the library's entry points reject before they touch a device, and the tools' ``--dtype`` option.  No GPU is opened."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import gemm_cases as gc  # noqa: E402
from tests import gemm_mxfp4_cases as mc  # noqa: E402

TINY = 2.0 ** -126  # the smallest normal fp32


def _low16(acc: torch.Tensor) -> torch.Tensor:
    return acc.contiguous().view(torch.int32) & 0xFFFF


# ---- the format ----------------------------------------------------------------------------------------------------

def test_e2m1_codes_and_the_nibble_order_are_torchs():
    assert mc.values(np.arange(16)).tolist() == [0, .5, 1, 1.5, 2, 3, 4, 6, -0.0, -.5, -1, -1.5, -2, -3, -4, -6]
    assert np.signbit(mc.values(np.array([8])))[0]
    codes = np.arange(32, dtype=np.uint8).reshape(1, 32) % 16
    q = mc.pack(codes)
    assert q.shape == (1, 16) and q[0, 0] == 0x10 and q[0, 1] == 0x32  # element 0 low, element 1 high
    assert (mc.unpack(q) == codes).all()
    assert torch.from_numpy(q).view(torch.float4_e2m1fn_x2).shape == (1, 16)  # the packed dtype is one byte a pair
    s = torch.tensor([1, 127, 254], dtype=torch.uint8).view(torch.float8_e8m0fnu).float()
    assert s.tolist() == [2.0 ** -126, 1.0, 2.0 ** 127]  # code c is 2^(c - 127)
    d = mc.dequant(np.full((1, 64), 7, dtype=np.uint8), np.array([[126, 130]], dtype=np.uint8))
    assert d[0, 31] == 3.0 and d[0, 32] == 48.0  # a code covers elements 32 g .. 32 g + 31


# ---- the cases ------------------------------------------------------------------------------------------------------

CASES = {
    "exact 128x128x256": lambda: mc.exact_case(128, 128, 256),
    "exact 256x256x1792": lambda: mc.exact_case(256, 256, 1792),
    "exact 768x512x32768": lambda: mc.exact_case(768, 512, 32768),  # the longest K of the GPU tests
    "exact 512x768x768": lambda: mc.exact_case(512, 768, 768),
    "code sweep": mc.code_sweep,
    "k slots": mc.k_slot_case,
    "scale slots 512": lambda: mc.scale_slot_case(512),
    "scale slots 1792": lambda: mc.scale_slot_case(1792),
    "e8m0 sweep": mc.e8m0_sweep,
}


@pytest.mark.parametrize("name", list(CASES))
def test_case_satisfies_the_exactness_condition(name):
    """All terms are multiples of one unit, their magnitudes sum to less than 2^24 units, and unit and sums are normal
    fp32: the fp32 accumulation is exact in any order, and the fp64 reference is the exact value."""
    case = CASES[name]()
    ex = mc.exactness(case.ac, case.sa, case.bc, case.sb)
    assert ex["units"] < 2 ** 24, ex
    assert ex["min_unit"] >= TINY and ex["max_sum"] < 2.0 ** 127, ex
    acc64 = torch.from_numpy(mc.dequant(case.ac, case.sa)) @ torch.from_numpy(mc.dequant(case.bc, case.sb)).t()
    assert torch.equal(acc64.float().double(), acc64)  # an fp32 value: the first rounding of the reference is none
    assert 1 <= int(min(case.sa.min(), case.sb.min())) and int(max(case.sa.max(), case.sb.max())) <= 254
    # with unit scales (the ablation configuration) the condition holds as well
    one = np.full_like(case.sa, 127), np.full_like(case.sb, 127)
    assert mc.exactness(case.ac, one[0], case.bc, one[1])["units"] < 2 ** 24


def test_exact_generator_needs_the_rounding_to_bf16_with_ties_in_both_directions():
    case = mc.exact_case(768, 512, 1792)
    acc = mc.accumulator(case.ac, case.sa, case.bc, case.sb)
    low = _low16(acc)
    assert float((low != 0).double().mean()) > 0.5  # most results are no bf16 values
    tie = low == 0x8000
    keep = (acc.contiguous().view(torch.int32) >> 16) & 1
    assert int((tie & (keep == 0)).sum()) >= 1 and int((tie & (keep == 1)).sum()) >= 1  # down to even, up to even
    assert torch.equal(gc.bits(case.want), gc.bits(acc.bfloat16()))
    assert mc.exact_case(768, 512, 1792) is case  # built once
    # the scales use the spread they claim and rows sit all over the range
    d = case.sa.astype(int) - case.sa.astype(int).min(axis=1, keepdims=True)
    assert set(d.flatten().tolist()) == {0, 1, 2}
    assert int(case.sa.min()) < 70 and int(case.sa.max()) > 175 and int(case.sb.min()) < 70
    assert set(case.ac.flatten().tolist()) == set(range(16)) == set(case.bc.flatten().tolist())
    long = mc.exact_case(768, 512, 32768)
    d = long.sa.astype(int) - long.sa.astype(int).min(axis=1, keepdims=True)
    assert set(d.flatten().tolist()) == {0, 1}


def test_code_sweep_holds_every_code_at_every_k_position_in_both_nibbles_and_tiles():
    case = mc.code_sweep()
    assert case.ac.shape == (4096, 512) and case.bc.shape == (256, 512)
    seen = set()
    for i in range(4096):
        (ks,) = np.nonzero(case.ac[i]) if i % 16 else (np.array([mc.sweep_k_of_row(i)]),)
        assert ks.tolist() == [mc.sweep_k_of_row(i)] and int(case.ac[i, ks[0]]) == i % 16
        seen.add((i % 16, ks[0] % 256, ks[0] // 256))
    assert {(c, p) for c, p, _ in seen} == {(c, p) for c in range(16) for p in range(256)}
    assert {t for _, _, t in seen} == {0, 1}  # both K-tiles, so both LDS buffers
    assert {(c, p & 1) for c, p, _ in seen} == {(c, h) for c in range(16) for h in (0, 1)}  # both nibbles
    bv = mc.values(case.bc)
    assert (bv == bv[:, :1]).all() and set(np.abs(bv[:, 0]).tolist()) == {0.5, 1.0, 2.0, 4.0}
    for mag in (0.5, 1.0, 2.0, 4.0):
        assert {1.0, -1.0} == set(np.sign(bv[np.abs(bv[:, 0]) == mag, 0]).tolist())
    acc = mc.accumulator(case.ac, case.sa, case.bc, case.sb)
    assert not bool(_low16(acc).any())  # every result is a bf16 value
    zero_rows = (acc == 0).all(dim=1).nonzero().flatten()
    assert zero_rows.numel() == 512 and set((zero_rows % 16).tolist()) == {0, 8}  # the codes of +0 and -0
    assert len(set(case.sa.flatten().tolist())) == 13 and len(set(case.sb.flatten().tolist())) == 7


def test_k_slot_case_has_one_entry_per_row_and_names_row_and_column():
    case = mc.k_slot_case()
    for codes in (case.ac, case.bc):
        nz = codes != 0
        assert (nz.sum(axis=1) == 1).all() and (nz.argmax(axis=1) == np.arange(512) % 256).all()
        assert int(codes.max()) <= 7  # positive values and +0
    w = case.want.double()
    i, j = torch.arange(512)[:, None], torch.arange(512)[None, :]
    diag = (i % 256) == (j % 256)
    assert bool((w[diag] != 0).all()) and not bool((gc.bits(case.want)[~diag] != 0).any())
    assert len(set(w[diag].tolist())) > 25  # the entries tell rows and columns apart


@pytest.mark.parametrize("k", [512, 1792])
def test_scale_slot_case_names_the_scale_bytes(k):
    case = mc.scale_slot_case(k)
    nb = k // 32
    i, j = np.arange(512)[:, None], np.arange(512)[None, :]
    e = mc.slot_scale_a(i, j % nb) + mc.slot_scale_b(j, j % nb) - 254
    assert torch.equal(case.want.double(), torch.from_numpy(32 * np.ldexp(1.0, e)))  # powers of two: bf16 values
    # neighbours differ: rows, blocks, the halves of a K-tile, consecutive K-tiles; A's and B's ranges are disjoint
    sa, sb = case.sa.astype(int), case.sb.astype(int)
    for s in (sa, sb):
        assert (s[1:] != s[:-1]).all() and (s[:, 1:] != s[:, :-1]).all()
        assert (s[:, 4:] != s[:, :-4]).all() and (s[:, 8:] != s[:, :-8]).all()
    assert int(sa.max()) < int(sb.min())
    # every block of the K range carries a column's ones, and only that block
    nz = (case.bc.reshape(512, nb, 32) != 0)
    assert (nz.all(axis=2).sum(axis=1) == 1).all() and (nz.any(axis=2).argmax(axis=1) == np.arange(512) % nb).all()
    assert set((np.arange(512) % nb).tolist()) == set(range(nb))


def test_e8m0_sweep_holds_every_code_in_both_scale_arrays():
    case = mc.e8m0_sweep()
    assert set(case.sa.flatten().tolist()) == set(range(1, 255)) == set(case.sb.flatten().tolist())
    e = case.sa.astype(int)[:, None, :] + case.sb.astype(int)[None, :, :] - 254
    assert (e == e[:, :, :1]).all() and set(e[:, :, 0].flatten().tolist()) == {0, 1, 2}


def test_banded_operand_is_16_byte_aligned_and_no_more():
    case = mc.exact_case(128, 128, 256)
    for payload, fill in ((case.aq, mc.A_BAND), (case.sa, mc.S_BAND)):
        whole, view = mc.banded(payload, fill, "cpu")
        assert view.data_ptr() % 32 == 16 and view.data_ptr() - whole.data_ptr() == gc.BAND + 16
        assert (view.numpy() == payload).all()
        assert set(whole[:gc.BAND + 16].tolist()) | set(whole[gc.BAND + 16 + payload.size:].tolist()) == {fill}
    assert mc.values(np.array([mc.A_BAND & 15, mc.A_BAND >> 4])).tolist() == [6.0, 6.0]


# ---- the quantiser's twin ------------------------------------------------------------------------------------------

def test_twin_round_trips_every_grid_value_times_every_power_of_two():
    """``g 2^e`` for every e2m1 value g and every e with a block maximum of 4 or 6 (so that the block's exponent is
    e): the codes come back, the scale is e + 127, zeros keep their sign."""
    for e in range(-126, 126):
        codes = np.concatenate([np.arange(16), [7] * 16]).astype(np.uint8).reshape(1, 32)
        x = mc.bf16_bits(mc.values(codes) * 2.0 ** e)
        x[0, 8] |= 0x8000  # -0
        q, s = mc.quant_twin(x)
        assert s.tolist() == [[e + 127]], e
        assert (mc.unpack(q) == codes).all(), e


def test_twin_rounds_ties_to_even_and_saturates_above_one_and_a_half():
    def q_of(vals, top):
        x = np.zeros((1, 32))
        x[0, :len(vals)] = vals
        x[0, 31] = top
        return mc.unpack(mc.quant_twin(mc.bf16_bits(x))[0])[0, :len(vals)].tolist()

    # block maximum 4: e = 0, elements are rounded as they stand
    assert q_of([0.25, 0.75, 1.25, 1.75, 2.5, 3.5], 4.0) == [0, 2, 2, 4, 4, 6]  # every tie to the even code
    assert q_of([-0.25, -0.75, -2.5, 0.251953125, 0.74609375, 2.515625], 4.0) == [8, 10, 12, 1, 1, 5]  # and beside
    assert q_of([0.375, 1.125, 1.375, 2.25, 2.75], 4.0) == [1, 2, 3, 4, 5]
    # 5 is the tie between 4 and 6; with a maximum of 5 itself the block's e is still 0
    assert q_of([5.0], 5.0) == [6] and q_of([5.5], 5.5) == [7]
    # a maximum whose mantissa is above 1.5 saturates: 6.5, 7, 7.75 -> 6
    for top in (6.5, 7.0, 7.75):
        x = np.zeros((1, 32))
        x[0, 0], x[0, 1] = top, -top
        q, s = mc.quant_twin(mc.bf16_bits(x))
        assert s[0, 0] == 127 and mc.unpack(q)[0, :2].tolist() == [7, 15]
    q, s = mc.quant_twin(mc.bf16_bits(np.array([[6.0] + [0.0] * 31])))
    assert s[0, 0] == 127 and mc.unpack(q)[0, 0] == 7  # 1.5 * 4 is the last maximum that is exact


def test_twin_special_blocks_and_the_clamp():
    z = np.zeros((1, 64), dtype=np.uint16)
    z[0, 1::2] = 0x8000
    q, s = mc.quant_twin(z)
    assert s.tolist() == [[127, 127]] and mc.unpack(q)[0].tolist() == [0, 8] * 32  # all-zero blocks, signs kept
    x = np.zeros((3, 32), dtype=np.uint16)
    x[0, 3], x[1, 3], x[2, 3] = 0x7F80, 0x7FC1, 0xFF80  # +inf, NaN, -inf
    assert mc.quant_twin(x)[1].flatten().tolist() == [255, 255, 255]
    # the smallest binades clamp to code 1, subnormals included: elements are x / 2^-126
    sub = np.zeros((2, 32), dtype=np.uint16)
    sub[0, 0], sub[0, 1] = 0x0001, 0x0040  # 2^-133 and 2^-127 (subnormal)
    sub[1, 0] = 0x0200  # 2^-123: floor(log2) - 2 = -125, code 2
    q, s = mc.quant_twin(sub)
    assert s.flatten().tolist() == [1, 2]
    assert mc.unpack(q)[0, :2].tolist() == [0, 1]  # 2^-7 rounds to 0; 2^-127 / 2^-126 = 0.5
    big = mc.bf16_bits(np.array([[2.0 ** 127 * 1.5] + [0.0] * 31]))
    assert mc.quant_twin(big)[1].tolist() == [[252]]  # the largest code a bf16 input can ask for


def test_lossless_inputs_quantise_to_their_codes():
    x, codes, s = mc.lossless_inputs(64, 512, 1)
    q, sq = mc.quant_twin(x)
    assert (sq == s).all() and (mc.unpack(q) == codes).all()
    assert (mc.bf16_values(x) == mc.dequant(codes, s)).all()
    assert len(set(s.flatten().tolist())) > 20


# ---- the library's host code (no GPU is opened) ---------------------------------------------------------------------

MXFP4_CFGS = {0: ("128x128/4w", 128, 128), 1: ("256x256/8w-phased-g4", 256, 256),
              2: ("256x256/8w-phased-g4-unit", 256, 256)}


@pytest.fixture(scope="module")
def hip():
    from gpushare_scheduler_extender_amd.ops import hip as h

    h.lib()
    assert hasattr(h, "gemm_mxfp4_cfgs"), "the bindings have no mxfp4 GEMM"
    return h


def test_mxfp4_config_table_has_its_rows_and_the_other_tables_keep_theirs(hip):
    L = hip.lib()
    assert hip.gemm_mxfp4_cfgs() == {c: row[0] for c, row in MXFP4_CFGS.items()}
    for c in (-1, 3, 11):
        assert L.gsx_gemm_mxfp4_cfg_name(c) is None
        bm, bn = ctypes.c_int(0), ctypes.c_int(0)
        assert L.gsx_gemm_mxfp4_cfg_tile(c, ctypes.byref(bm), ctypes.byref(bn)) != 0
    for c, (_, m, n) in MXFP4_CFGS.items():
        bm, bn = ctypes.c_int(0), ctypes.c_int(0)
        assert L.gsx_gemm_mxfp4_cfg_tile(c, ctypes.byref(bm), ctypes.byref(bn)) == 0 and (bm.value, bn.value) == (m, n)
    assert len(hip.gemm_cfgs()) == 11 and len(hip.gemm_fp8_cfgs()) == 3


# Addresses that are never dereferenced: every call below is refused before the first device call.
A, B, C, SA, SB = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000


class _NoStream:
    """Stands in for ``hip.Stream``: the calls under test never get as far as using one."""
    handle = None


def _rejects(hip, text, *, cfg=None, m=256, n=256, k=256, a=A, b=B, c=C, sa=SA, sb=SB):
    entry = "gsx_gemm_mxfp4_nt" if cfg is None else "gsx_gemm_mxfp4_nt_launch_cfg"
    with pytest.raises(hip.HipError, match=f"{entry}: {text}"):
        if cfg is None:
            hip.gemm_mxfp4_nt(_NoStream, a, b, c, m, n, k, sa, sb)
        else:
            hip.gemm_mxfp4_nt_cfg(_NoStream, a, b, c, m, n, k, cfg, sa, sb)


@pytest.mark.parametrize("cfg", [None, 0, 1, 2])
def test_mxfp4_entry_points_reject_bad_arguments_by_name(hip, cfg):
    def rej(text, **kw):
        _rejects(hip, text, cfg=cfg, **kw)

    tile = 128 if cfg in (None, 0) else 256
    shape = f"need M%{tile}==0, N%{tile}==0, K%256==0"
    rej(shape, k=128)  # K % 256: a K-tile of the fp8 kernels is not one here
    rej(shape, k=384)
    rej(shape, m=tile + 64)
    rej(shape, n=tile // 2)
    rej(shape, k=0)
    if cfg is not None and tile == 256:
        rej(shape, m=384)  # fine for the dispatching entry point, which takes the 128 tile then
    for name in ("a", "b", "c"):
        rej("operands must be 16-B aligned", **{name: A + 8})
    rej("scale_a and scale_b must be 16-B aligned", sa=SA + 8)
    rej("scale_a and scale_b must be 16-B aligned", sb=SB + 4)
    rej("scale_a and scale_b must not be NULL", sa=0)
    rej("scale_a and scale_b must not be NULL", sb=0)
    # one K-tile past the longest K: the 32-bit byte offset of the tile's last row would wrap
    side = 256 if cfg is None else tile
    k_ok = (2 ** 31 - 1 - 112) // (side - 1) // 128 * 128 * 2
    assert (side - 1) * (k_ok // 2) + 112 < 2 ** 31 <= (side - 1) * ((k_ok + 256) // 2) + 112
    assert k_ok == {256: 16843008, 128: 33818624}[side]  # what gsx_kernels.h documents
    rej("K too large", m=side, n=side, k=k_ok + 256)


def test_mxfp4_unknown_config_is_rejected_by_name(hip):
    for cfg in (-1, 3, 5):
        _rejects(hip, "unknown config", cfg=cfg)


def test_quantiser_rejects_bad_arguments_by_name(hip):
    for kw, text in (({"k": 48}, "K%32==0"), ({"rows": 0}, "need R > 0"), ({"x": 0}, "must not be NULL"),
                     ({"s": 0}, "must not be NULL"), ({"q": A + 8}, "16-B aligned"), ({"x": A + 2}, "16-B aligned")):
        args = {"x": A, "q": B, "s": C + 1, "rows": 3, "k": 64, **kw}
        with pytest.raises(hip.HipError, match=f"gsx_quant_mxfp4: .*{text}"):
            hip.quant_mxfp4(_NoStream, args["x"], args["q"], args["s"], args["rows"], args["k"])


# ---- the tools -----------------------------------------------------------------------------------------------------

def test_workload_and_isolation_parsers_take_mxfp4_and_still_refuse_fp4():
    from gsxtools import isolation, workload

    for mod in (workload, isolation):
        ap = mod.build_parser()
        assert ap.parse_args([]).dtype == "bf16"
        assert ap.parse_args(["--dtype", "mxfp4"]).dtype == "mxfp4"
        assert ap.parse_args(["--dtype", "fp8"]).dtype == "fp8"
        with pytest.raises(SystemExit):
            ap.parse_args(["--dtype", "fp4"])
