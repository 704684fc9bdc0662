"""``--workload moe`` of the sample workload: what its parser takes and what it refuses, before anything loads torch."""
import importlib.util
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BASE = ["--workload", "moe", "--kernel", "gsx", "--experts", "16", "--experts-active", "2", "--batch", "3", "--size",
        "256", "--ffn", "128"]


@pytest.fixture(scope="module")
def wl():
    spec = importlib.util.spec_from_file_location("gsx_sample_workload_moe", ROOT / "samples" / "workload" / "main.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("dtype", ["bf16", "fp8-block"])
def test_parser_accepts_the_moe_workload(wl, dtype):
    ns = wl.build_parser().parse_args([*BASE, "--dtype", dtype])
    assert (ns.workload, ns.dtype, ns.experts, ns.experts_active, ns.ffn) == ("moe", dtype, 16, 2, 128)


@pytest.mark.parametrize("args,text", [
    (["--experts", "0"], "--workload moe --experts 0: a multiple of 16 in 16..1024"),
    (["--dtype", "fp8-block", "--ffn", "192"], "--ffn 192: a multiple of 128"),
    (["--kernel", "torch"], "--workload moe runs on the library's kernels only"),
    (["--workload", "decode", "--dtype", "fp8-block"], "--workload decode --dtype fp8-block: block-scaled operands"),
])
def test_parser_refuses(wl, capsys, args, text):
    with pytest.raises(SystemExit) as e:
        wl.build_parser().parse_args([*BASE, *args])
    assert e.value.code == 2 and text in capsys.readouterr().err
