"""CPU checks for the decode GEMM (native/kernels/gemm_decode.hip): the helpers of ``tests/gemm_decode_cases.py``
against the families' references, the configuration table, every argument the entry points refuse, the tools'
parsers and the size of the workload's weight ring.  No GPU: the refused calls never reach the device."""
import ctypes
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import gemm_cases as gc  # noqa: E402
from tests import gemm_decode_cases as dc  # noqa: E402
from tests import gemm_fp8_cases as gf  # noqa: E402
from tests import gemm_mxfp4_cases as mc  # noqa: E402


@pytest.fixture(scope="module")
def hip():
    from gpushare_scheduler_extender_amd.ops import hip as h

    h.lib()
    assert hasattr(h, "decode_gemm_cfgs"), "the bindings have no decode GEMM"
    return h


# ---- the helpers -----------------------------------------------------------------------------------------------------

def _same(got, want, **kw):
    gc.assert_bits_equal(got, want, "", **kw)


def _samples():
    rc = gc.rounding_case()
    a8, b8, acc8 = gf.exact_case(48, 80, 384)
    return {
        "bf16 exact": dc.exact_problem("bf16", 80, 320),
        "bf16 rounding": dc.bf16_problem(rc.a, rc.b, rc.want),
        "fp8 k slots": dc.Problem("fp8", *gf.k_slot_case()),
        "fp8 code sweep": dc.Problem("fp8", *gf.code_sweep()),
        "fp8 row scales": dc.fp8_problem(a8, b8, acc8, gf.row_scales(48, 5), gf.row_scales(80, 7), gf.SCALE_ROW),
        "fp8 tensor scales": dc.fp8_problem(a8, b8, acc8, torch.tensor([0.75]), torch.tensor([-3.0]),
                                            gf.SCALE_TENSOR),
        "mxfp4 exact": dc.exact_problem("mxfp4", 48, 768),
        "mxfp4 k slots": dc.mxfp4_problem(mc.k_slot_case()),
        "mxfp4 scale slots": dc.mxfp4_problem(mc.scale_slot_case(512)),
    }


@pytest.mark.parametrize("name", list(_samples()))
def test_slices_and_transposed_slices_are_what_the_references_give(name):
    """A 16-row slice, a ragged slice and 16-row slices of the transposed problem: the result each carries is the
    family's reference of the operands it carries, bit for bit (a NaN where that has one)."""
    p = _samples()[name]
    zero = {"zero_by_value_cols": range(p.n)} if name == "bf16 rounding" else {}  # 0 * -x: the sign is the order's
    assert p.k % dc.BK[p.kind] == 0 and p.want.shape == (p.m, p.n)
    for r0, m in ((0, min(16, p.m)), (p.m - 5, 5)):
        s = p.rows(r0, m)
        assert (s.m, s.n, s.k) == (m, p.n, p.k) and s.want.shape == (m, p.n)
        _same(s.reference(), s.want, **zero)
    t = p.transposed()
    assert (t.m, t.n, t.k) == (p.n, p.m, p.k)
    if p.kind != "fp8" or p.mode == gf.SCALE_NONE:
        assert torch.equal(gc.bits(t.want), gc.bits(p.want.t().contiguous()))
    zero = {"zero_by_value_cols": range(t.n)} if name == "bf16 rounding" else {}
    for r0 in (0, t.m - 16):
        s = t.rows(r0, 16)
        _same(s.reference(), s.want, **zero)
    back = t.transposed()
    assert torch.equal(gc.bits(back.want), gc.bits(p.want)) and back.a is p.a and back.sb is p.sb


def test_exact_problems_are_the_exact_generators_and_stay_exact():
    """Rows of the 16-row bf16 and fp8 problems are the generators' own problems of that M; the mxfp4 problems meet
    the exactness condition at the longest K the GPU tests use."""
    for m in (1, 5, 16):
        a, b, want = gc.exact_case(m, 48, 192)
        p = dc.exact_problem("bf16", 48, 192).rows(0, m)
        assert torch.equal(p.a, a) and torch.equal(p.b, b) and torch.equal(gc.bits(p.want), gc.bits(want))
        a8, b8, acc = gf.exact_case(m, 48, 256)
        p = dc.exact_problem("fp8", 48, 256).rows(0, m)
        assert torch.equal(gf.codes(p.a), gf.codes(a8)) and torch.equal(p.acc, acc)
    case = mc.exact_case(16, 48, dc.MAX_K["mxfp4"])
    ex = mc.exactness(case.ac, case.sa, case.bc, case.sb)
    assert ex["units"] < 2 ** 24 and ex["min_unit"] >= 2.0 ** -126 and ex["max_sum"] < 2.0 ** 127
    assert max(nk * dc.BK[kind] for kind in dc.KINDS for nk in dc.k_tile_counts(None, kind)) <= 65536


def test_exact_b_rows_is_the_generator_formula():
    _, b = gc.exact_operands(1, 300, 256)
    rows = torch.tensor([0, 1, 17, 299])
    assert torch.equal(dc.exact_b_rows(rows, 256), b[rows])


def test_k_tile_counts_hold_what_the_issue_lists():
    for cfg, (_, _, w, f) in dc.CFGS.items():
        listed = {1, 2, w - 1, w, w + 1, 2 * w + 1, f * w - 1, f * w, f * w + 1, 128}
        for kind in dc.KINDS:
            assert listed <= set(dc.k_tile_counts(cfg, kind)) <= set(dc.k_tile_counts(None, kind))


def test_error_bound_is_the_formula():
    ref, mag = torch.tensor([3.0, -5.0], dtype=torch.float64), torch.tensor([7.0, 11.0], dtype=torch.float64)
    want = [2.0 ** -8 * 3 + 4096 * 2.0 ** -23 * 7, 2.0 ** -8 * 5 + 4096 * 2.0 ** -23 * 11]
    assert dc.error_bound(ref, mag, 4096).tolist() == want


# ---- the configuration table ----------------------------------------------------------------------------------------

def test_decode_config_table_matches_and_the_queries_fail_outside_it(hip):
    L = hip.lib()
    assert hip.decode_gemm_cfgs() == dc.CFGS
    for c in (-1, len(dc.CFGS), 99):
        assert L.gsx_decode_gemm_cfg_name(c) is None
        v = [ctypes.c_int(-7) for _ in range(3)]
        assert L.gsx_decode_gemm_cfg_shape(c, *map(ctypes.byref, v)) != 0
        assert [x.value for x in v] == [-7, -7, -7]
    for c, (name, bn, w, f) in dc.CFGS.items():
        assert L.gsx_decode_gemm_cfg_name(c).decode() == name
        assert bn in (16, 32) and w in (4, 8, 16) and f >= 1
    assert {w for _, _, w, _ in dc.CFGS.values()} == {4, 8, 16} and {bn for _, bn, _, _ in dc.CFGS.values()} == {16, 32}
    assert len({f for _, _, _, f in dc.CFGS.values()}) > 1 and any(n.endswith("-nt") for n, *_ in dc.CFGS.values())
    assert hip.DECODE_KINDS == {"bf16": 0, "fp8": 1, "mxfp4": 2}
    # the other families keep their tables
    assert len(hip.gemm_cfgs()) == 11 and len(hip.gemm_fp8_cfgs()) == 3 and len(hip.gemm_mxfp4_cfgs()) == 3


# ---- rejections ------------------------------------------------------------------------------------------------------

# Addresses that are never dereferenced: every call below is refused before the first device call.
A, B, C, SA, SB = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
NONE, TENSOR, ROW = gf.SCALE_NONE, gf.SCALE_TENSOR, gf.SCALE_ROW


class _NoStream:
    """Stands in for ``hip.Stream``: the calls under test never get as far as using one."""
    handle = None


def _good(kind):
    """Arguments every entry point accepts for ``kind`` (were the addresses real)."""
    scales = {"bf16": (0, 0, NONE), "fp8": (SA + 4, SB + 4, ROW), "mxfp4": (SA, SB, NONE)}[kind]
    return {"m": 5, "n": 96, "k": 2 * dc.BK[kind], "a": A, "b": B, "c": C, "sa": scales[0], "sb": scales[1],
            "mode": scales[2]}


def _call(hip, kind, cfg, v):
    args = (_NoStream, kind, v["a"], v["b"], v["c"], v["m"], v["n"], v["k"])
    if cfg is None:
        hip.decode_gemm_nt(*args, v["sa"], v["sb"], v["mode"])
    else:
        hip.decode_gemm_nt_cfg(*args, cfg, v["sa"], v["sb"], v["mode"])


def _rejects(hip, kind, cfg, text, **kw):
    entry = "gsx_decode_gemm_nt" if cfg is None else "gsx_decode_gemm_nt_launch_cfg"
    with pytest.raises(hip.HipError, match=f"{entry}: {text}"):
        _call(hip, kind, cfg, {**_good(kind), **kw})


@pytest.mark.parametrize("cfg", dc.ALL)
@pytest.mark.parametrize("kind", dc.KINDS)
def test_decode_entry_points_reject_bad_arguments_by_name(hip, kind, cfg):
    def rej(text, **kw):
        _rejects(hip, kind, cfg, text, **kw)

    bn = 16 if cfg is None else dc.CFGS[cfg][1]
    bk = dc.BK[kind]
    for m in (0, 17, -1):
        rej("need 1 <= M <= 16", m=m)
    shape = f"need N%{bn}==0, K%{bk}==0"
    for n in (0, 8, 24, bn + 8, -16):
        rej(shape, n=n)
    if bn == 32:
        rej(shape, n=48)  # fine for the strips of 16 columns
    for k in (0, bk // 2, bk + bk // 2, -bk):
        rej(shape, k=k)
    if kind == "mxfp4":
        rej(shape, k=128)  # a K-tile of the fp8 kernels
        rej(shape, k=384)
    if kind == "fp8":
        rej(shape, k=64)  # a K-tile of the bf16 kernels
    for name in ("a", "b", "c"):
        rej("A, B and C must not be NULL", **{name: 0})
        rej("operands must be 16-B aligned", **{name: A + 8})
    if kind == "bf16":
        text = "bf16 takes no scales: scale_a and scale_b must be NULL and scale_mode NONE"
        rej(text, sa=SA)
        rej(text, sb=SB)
        rej(text, mode=TENSOR)
        rej(text, mode=ROW)
    elif kind == "fp8":
        for mode in (TENSOR, ROW):
            rej("scale_a and scale_b must not be NULL in this scale_mode", mode=mode, sa=0)
            rej("scale_a and scale_b must not be NULL in this scale_mode", mode=mode, sb=0)
            rej("scale_a and scale_b must be 4-B aligned", mode=mode, sa=SA + 2)
            rej("scale_a and scale_b must be 4-B aligned", mode=mode, sb=SB + 1)
        rej("unknown scale_mode 3", mode=3)
        rej("unknown scale_mode -1", mode=-1)
    else:
        rej("scale_a and scale_b must not be NULL", sa=0)
        rej("scale_a and scale_b must not be NULL", sb=0)
        rej("scale_a and scale_b must be 16-B aligned", sa=SA + 8)
        rej("scale_a and scale_b must be 16-B aligned", sb=SB + 4)
        rej("mxfp4 takes scale_mode NONE", mode=TENSOR)
        rej("mxfp4 takes scale_mode NONE", mode=ROW)


@pytest.mark.parametrize("cfg", dc.ALL)
def test_decode_unknown_kind_is_rejected_by_name(hip, cfg):
    entry = "gsx_decode_gemm_nt" if cfg is None else "gsx_decode_gemm_nt_launch_cfg"
    L = hip.lib()
    for kind in (-1, 3, 7):
        args = [None, kind, A, B, C, 5, 96, 512, None, None, 0] + ([] if cfg is None else [cfg])
        rc = (L.gsx_decode_gemm_nt if cfg is None else L.gsx_decode_gemm_nt_launch_cfg)(*args)
        assert rc != 0 and L.gsx_last_error().decode() == f"{entry}: unknown kind {kind}"
    with pytest.raises(ValueError, match="decode kind 'fp4'"):
        hip.decode_gemm_nt(_NoStream, "fp4", A, B, C, 5, 96, 512)


@pytest.mark.parametrize("kind", dc.KINDS)
def test_decode_unknown_config_is_rejected_by_name(hip, kind):
    for cfg in (-1, len(dc.CFGS), 40):
        _rejects(hip, kind, cfg, "unknown config")


def test_time_decode_gemm_rejects_before_it_touches_the_device(hip):
    with pytest.raises(hip.HipError, match="gsx_decode_gemm_nt: need 1 <= M <= 16"):
        hip.time_decode_gemm(_NoStream, "bf16", A, B, C, 17, 96, 128, 0)


# ---- the tools -------------------------------------------------------------------------------------------------------

def test_workload_and_isolation_parsers_take_the_decode_workload():
    from gsxtools import isolation, workload

    for mod in (workload, isolation):
        ap = mod.build_parser()
        d = ap.parse_args([])
        assert (d.workload, d.batch, d.dtype) == ("gemm", 8, "bf16")
        for b in (1, 16):
            got = ap.parse_args(["--workload", "decode", "--batch", str(b)])
            assert (got.workload, got.batch) == ("decode", b)
        for bad in (["--batch", "0"], ["--batch", "17"], ["--workload", "prefill"]):
            with pytest.raises(SystemExit):
                ap.parse_args(bad)
    assert workload.build_parser().parse_args([]).weights_gib is None
    assert workload.build_parser().parse_args(["--weights-gib", "0.25"]).weights_gib == 0.25
    # the default scenario list is what it was; the two new names are known
    assert isolation.build_parser().parse_args([]).scenarios == \
        "solo,shared,partitioned,env,env-gsx,solo-small,solo64,noisy,noisy-partitioned"
    assert {"decode-noisy", "decode-noisy-partitioned"} <= set(isolation.SCENARIOS)
    assert set(isolation.build_parser().parse_args([]).scenarios.split(",")) <= set(isolation.SCENARIOS)
    with pytest.raises(SystemExit, match="unknown scenario decode-quiet"):
        isolation.main(["--scenarios", "decode-quiet"])


def test_isolation_summary_adds_the_byte_rates_only_for_decode_pods():
    from gsxtools import isolation

    gemm = isolation.summarize("shared", [{"tflops": 300.0}, {"tflops": 150.0}])
    assert gemm == {"scenario": "shared", "pods": 2, "per_pod_tflops": [300.0, 150.0], "aggregate_tflops": 450.0,
                    "fairness_min_over_max": 0.5}
    mixed = isolation.summarize("decode-noisy", [{"tflops": 0.5, "tbps": 2.1234}, {"tflops": 300.0}])
    assert mixed["per_pod_tbps"] == [2.123, None] and mixed["aggregate_tbps"] == 2.123
    assert mixed["per_pod_tflops"] == [0.5, 300.0]


def test_workload_ring_size():
    from gsxtools import workload as wl

    gib = 1 << 30
    assert wl.matrix_bytes("bf16", 8192, 8192) == 128 << 20
    assert wl.matrix_bytes("fp8", 8192, 8192) == 64 << 20
    assert wl.matrix_bytes("mxfp4", 8192, 8192) == (32 << 20) + (2 << 20)  # codes and one scale byte per 32
    # the default: 4 GiB, or a quarter of the share if that is smaller
    assert wl.default_weights_bytes(0) == 4 * gib
    assert wl.default_weights_bytes(64) == 4 * gib
    assert wl.default_weights_bytes(16) == 4 * gib
    assert wl.default_weights_bytes(8) == 2 * gib
    assert wl.default_weights_bytes(1.5) == 3 * gib // 8
    for dtype in dc.KINDS:
        for size in (1024, 4096, 8192):
            one = wl.matrix_bytes(dtype, size, size)
            for want in (0, 1, one - 1, one, one + 1, gib // 4, 4 * gib, 5 * gib + 3):
                layers = wl.ring_layers(want, one)
                assert layers >= 2 and layers * one >= want  # never one matrix; covers what was asked for
                assert layers == 2 or (layers - 1) * one < want  # and no more than that
    assert wl.ring_layers(4 * gib, wl.matrix_bytes("bf16", 8192, 8192)) == 32
    assert wl.ring_layers(4 * gib, wl.matrix_bytes("mxfp4", 8192, 8192)) == math.ceil(4 * gib / (34 << 20))
    # larger than the 256 MiB Infinity Cache at the default, whatever the dtype
    assert all(wl.ring_layers(4 * gib, wl.matrix_bytes(d, 8192, 8192)) * wl.matrix_bytes(d, 8192, 8192) > 256 << 20
               for d in dc.KINDS)
    assert isinstance(np.int64(wl.ring_layers(gib, 1 << 20)).item(), int)
