"""``--workload prefill-moe --dtype fp8-block`` of the sample workload: what its parser takes and what it refuses, before
anything loads torch."""
import importlib.util
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BASE = ["--workload", "prefill-moe", "--kernel", "gsx", "--dtype", "fp8-block", "--experts", "128", "--experts-active",
        "2", "--heads", "2", "--kv-heads", "1", "--context", "128", "--chunk", "128", "--batch", "1", "--ffn", "128"]


@pytest.fixture(scope="module")
def wl():
    spec = importlib.util.spec_from_file_location("gsx_sample_workload_pfb", ROOT / "samples" / "workload" / "main.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_parser_accepts_prefill_moe_with_fp8_block(wl):
    ns = wl.build_parser().parse_args(BASE)
    assert (ns.workload, ns.dtype, ns.experts, ns.ffn) == ("prefill-moe", "fp8-block", 128, 128)


@pytest.mark.parametrize("args,text", [
    (["--ffn", "192"], "--ffn 192: a multiple of 128"),
    (["--kernel", "torch"], "--dtype fp8-block needs the library's kernels"),
    (["--workload", "decode"], "--workload decode --dtype fp8-block: block-scaled operands"),
])
def test_parser_refuses(wl, capsys, args, text):
    with pytest.raises(SystemExit) as e:
        wl.build_parser().parse_args([*BASE, *args])
    assert e.value.code == 2 and text in capsys.readouterr().err
