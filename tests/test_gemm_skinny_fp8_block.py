"""CPU checks for the block-scaled fp8 skinny GEMM (native/kernels/gemm_skinny_fp8_block.hip): the configuration
table, the workspace query against the dispatcher, every argument the entry points refuse, and the workload's parser.
No GPU: the refused calls never reach the device."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def hip():
    from gpushare_scheduler_extender_amd.ops import hip as h

    h.lib()
    return h


def test_config_table_is_consistent(hip):
    L = hip.lib()
    cfgs = hip.skinny_gemm_fp8_block_cfgs()
    assert len(cfgs) >= 2 and len({name for name, *_ in cfgs.values()}) == len(cfgs)
    assert {32, 64} <= {bn for _, bn, *_ in cfgs.values()}
    for c, (name, bn, waves, inflight) in cfgs.items():
        assert L.gsx_skinny_gemm_fp8_block_cfg_name(c).decode() == name == f"{bn}/{waves}w-f{inflight}"
        assert 64 % bn == 0 and waves >= 1 and inflight >= 1
    for c in (-1, len(cfgs), 99):
        assert L.gsx_skinny_gemm_fp8_block_cfg_name(c) is None
        v = [ctypes.c_int(-7) for _ in range(3)]
        assert L.gsx_skinny_gemm_fp8_block_cfg_shape(c, *map(ctypes.byref, v)) != 0
        assert [x.value for x in v] == [-7] * 3


@pytest.mark.parametrize("n,k", [(64, 128), (192, 1664), (1024, 8192), (8192, 8192), (7168, 18432), (28672, 8192)])
def test_workspace_is_monotone_and_covers_the_dispatcher(hip, n, k):
    cfgs = hip.skinny_gemm_fp8_block_cfgs()
    last = 0
    for m in range(1, 129):
        have = hip.skinny_gemm_fp8_block_workspace_bytes(m, n, k)
        assert have >= last
        last = have
        cfg, splits = hip.skinny_gemm_fp8_block_pick(m, n, k)
        assert cfg in cfgs and n % cfgs[cfg][1] == 0 and 1 <= splits <= 16
        assert have >= (splits * m * n * 4 if splits > 1 else 0)
    assert hip.skinny_gemm_fp8_block_pick(128, 1024, 8192)[1] > 1  # the split of K is dispatched


# Addresses that are never dereferenced: every call below is refused before the first device call.
A, B, C, SA, SB, WS = 0x10000, 0x2000000, 0x4000000, 0x6000000, 0x6100000, 0x8000000


class _NoStream:
    handle = None


REFUSALS = [  # what differs from a good call, the text
    ({"m": 0}, "need 1 <= M <= 128"),
    ({"m": 129}, "need 1 <= M <= 128"),
    ({"n": 96}, "need N%64==0, K%128==0"),
    ({"k": 192}, "need N%64==0, K%128==0"),
    ({"a": 0}, "A, B, C, scale_a and scale_b must not be NULL"),
    ({"sb": 0}, "A, B, C, scale_a and scale_b must not be NULL"),
    ({"b": B + 8}, "operands and workspace must be 16-B aligned"),
    ({"sa": SA + 2}, "scale_a and scale_b must be 4-B aligned"),
    ({"stride": 1}, "need sa_stride >= K/128"),
    ({"splits": 3, "ws_bytes": 3 * 40 * 192 * 4 - 1}, "workspace too small: splits 3 needs 92160 bytes"),
    ({"splits": 0}, "need 1 <= splits <= 16"),
    ({"splits": 17}, "need 1 <= splits <= 16"),
    ({"splits": 2, "c": WS + 64}, "C must not overlap A, B, scale_a, scale_b or the workspace"),
    ({"cfg": 99}, "unknown config"),
]


@pytest.mark.parametrize("change,text", REFUSALS, ids=[f"{'-'.join(c)}-{t[:20]}" for c, t in REFUSALS])
def test_entry_points_refuse_by_name(hip, change, text):
    v = {"m": 40, "n": 192, "k": 256, "a": A, "b": B, "c": C, "sa": SA, "sb": SB, "stride": 2, "splits": 1, "cfg": 0,
         "ws_bytes": 1 << 20, **change}
    args = (_NoStream, v["a"], v["b"], v["c"], v["m"], v["n"], v["k"])
    tail = {"scale_a": v["sa"], "sa_stride": v["stride"], "scale_b": v["sb"], "workspace": WS,
            "workspace_bytes": v["ws_bytes"]}
    with pytest.raises(hip.HipError, match=f"gsx_skinny_gemm_fp8_block_nt_launch_cfg: {text}"):
        hip.skinny_gemm_fp8_block_nt_cfg(*args, v["cfg"], v["splits"], **tail)
    if not {"splits", "cfg"} & set(change):  # the dispatching call and its timing twin refuse the same, under its name
        with pytest.raises(hip.HipError, match=f"gsx_skinny_gemm_fp8_block_nt: {text}"):
            hip.skinny_gemm_fp8_block_nt(*args, **tail)
        with pytest.raises(hip.HipError, match=f"gsx_skinny_gemm_fp8_block_nt: {text}"):
            hip.time_skinny_gemm_fp8_block(*args, 1, **tail)


def test_dispatcher_refuses_a_short_workspace(hip):
    m, n, k = 128, 1024, 8192
    need = hip.skinny_gemm_fp8_block_workspace_bytes(m, n, k)
    assert need > 0
    with pytest.raises(hip.HipError,
                       match=f"gsx_skinny_gemm_fp8_block_nt: workspace too small: splits \\d+ needs {need} bytes"):
        hip.skinny_gemm_fp8_block_nt(_NoStream, A, B, C, m, n, k, SA, k // 128, SB, workspace=WS,
                                     workspace_bytes=need - 1)


def test_workload_parser_takes_block_scaled_decode_wide():
    from gsxtools import workload

    ap = workload.build_parser()
    got = ap.parse_args(["--workload", "decode-wide", "--dtype", "fp8-block", "--batch", "128"])
    assert (got.workload, got.batch, got.dtype) == ("decode-wide", 128, "fp8-block")
    with pytest.raises(SystemExit):
        ap.parse_args(["--workload", "decode", "--dtype", "fp8-block"])
