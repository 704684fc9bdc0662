"""CPU checks for the skinny GEMM (native/kernels/gemm_skinny.hip): the configuration table, the workspace query
against the dispatcher, every argument the entry points refuse, and the workload's parser.  No GPU: the refused calls
never reach the device."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def hip():
    from gpushare_scheduler_extender_amd.ops import hip as h

    h.lib()
    return h


def test_skinny_config_table_is_consistent(hip):
    L = hip.lib()
    cfgs = hip.skinny_gemm_cfgs()
    assert len(cfgs) >= 2 and len({name for name, *_ in cfgs.values()}) == len(cfgs)
    for c, (name, bn, waves, inflight) in cfgs.items():
        assert L.gsx_skinny_gemm_cfg_name(c).decode() == name == f"{bn}/{waves}w-f{inflight}"
        assert bn % 16 == 0 and (64 % bn == 0 or bn % 64 == 0) and waves >= 1 and inflight >= 1
    for c in (-1, len(cfgs), 99):
        assert L.gsx_skinny_gemm_cfg_name(c) is None
        v = [ctypes.c_int(-7) for _ in range(3)]
        assert L.gsx_skinny_gemm_cfg_shape(c, *map(ctypes.byref, v)) != 0 and [x.value for x in v] == [-7] * 3


@pytest.mark.parametrize("n,k", [(64, 64), (192, 832), (1024, 8192), (8192, 8192), (8192, 28672), (28672, 8192)])
def test_skinny_workspace_is_monotone_and_covers_the_dispatcher(hip, n, k):
    cfgs = hip.skinny_gemm_cfgs()
    last = 0
    for m in range(1, 129):
        have = hip.skinny_gemm_workspace_bytes(m, n, k)
        assert have >= last
        last = have
        for kind in ("bf16", "fp8"):
            if k % (64 if kind == "bf16" else 128):
                continue
            cfg, splits = hip.skinny_gemm_pick(kind, m, n, k)
            assert cfg in cfgs and n % cfgs[cfg][1] == 0 and 1 <= splits <= 16
            assert have >= (splits * m * n * 4 if splits > 1 else 0)
    assert any(hip.skinny_gemm_pick("bf16", m, 1024, 8192)[1] > 1 for m in (17, 128))  # the split of K is dispatched


# Addresses that are never dereferenced: every call below is refused before the first device call.
A, B, C, SA, SB, WS = 0x10000, 0x2000000, 0x4000000, 0x6000000, 0x6100000, 0x8000000


class _NoStream:
    handle = None


REFUSALS = [  # kind, what differs from a good call, the text
    ("bf16", {"m": 0}, "need 1 <= M <= 128"),
    ("fp8", {"m": 129}, "need 1 <= M <= 128"),
    ("bf16", {"n": 96}, "need N%64==0, K%64==0"),
    ("bf16", {"k": 96}, "need N%64==0, K%64==0"),
    ("fp8", {"k": 64}, "need N%64==0, K%128==0"),
    ("mxfp4", {}, "mxfp4 is not supported by the skinny GEMM"),
    ("bf16", {"a": A + 8}, "operands and workspace must be 16-B aligned"),
    ("fp8", {"sa": 0, "sb": 0, "mode": 2}, "scale_a and scale_b must not be NULL in this scale_mode"),
    ("bf16", {"splits": 3, "ws_bytes": 3 * 40 * 192 * 4 - 1}, "workspace too small: splits 3 needs 92160 bytes"),
    ("bf16", {"splits": 0}, "need 1 <= splits <= 16"),
    ("fp8", {"splits": 17}, "need 1 <= splits <= 16"),
]


@pytest.mark.parametrize("kind,change,text", REFUSALS, ids=[f"{k}-{t[:24]}" for k, _, t in REFUSALS])
def test_skinny_entry_points_refuse_by_name(hip, kind, change, text):
    v = {"m": 40, "n": 192, "k": 256, "a": A, "sa": 0, "sb": 0, "mode": 0, "splits": 1, "ws_bytes": 1 << 20, **change}
    args = (_NoStream, kind, v["a"], B, C, v["m"], v["n"], v["k"])
    tail = {"scale_a": v["sa"], "scale_b": v["sb"], "scale_mode": v["mode"], "workspace": WS,
            "workspace_bytes": v["ws_bytes"]}
    with pytest.raises(hip.HipError, match=f"gsx_skinny_gemm_nt_launch_cfg: {text}"):
        hip.skinny_gemm_nt_cfg(*args, 0, v["splits"], **tail)
    if "splits" not in change:  # the dispatching entry point and the timing twin refuse the same, under its name
        with pytest.raises(hip.HipError, match=f"gsx_skinny_gemm_nt: {text}"):
            hip.skinny_gemm_nt(*args, **tail)
        with pytest.raises(hip.HipError, match=f"gsx_skinny_gemm_nt: {text}"):
            hip.time_skinny_gemm(*args, 1, **tail)


def test_skinny_dispatcher_refuses_a_short_workspace_and_an_overlap(hip):
    m, n, k = 128, 1024, 8192
    need = hip.skinny_gemm_workspace_bytes(m, n, k)
    assert need > 0
    with pytest.raises(hip.HipError, match=f"gsx_skinny_gemm_nt: workspace too small: splits \\d+ needs {need} bytes"):
        hip.skinny_gemm_nt(_NoStream, "bf16", A, B, C, m, n, k, workspace=WS, workspace_bytes=need - 1)
    with pytest.raises(hip.HipError, match="gsx_skinny_gemm_nt: C must not overlap"):
        hip.skinny_gemm_nt(_NoStream, "bf16", A, B, WS + 64, m, n, k, workspace=WS, workspace_bytes=need)


def test_workload_parser_takes_decode_wide():
    from gsxtools import workload

    ap = workload.build_parser()
    got = ap.parse_args(["--workload", "decode-wide", "--batch", "128", "--dtype", "fp8"])
    assert (got.workload, got.batch, got.dtype) == ("decode-wide", 128, "fp8")
    for bad in (["--workload", "decode-wide", "--batch", "129"], ["--workload", "decode-wide", "--batch", "0"],
                ["--workload", "decode", "--batch", "17"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
