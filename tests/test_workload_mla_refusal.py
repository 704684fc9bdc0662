"""What ``--mla`` of the sample workload refuses, known before torch loads (samples/workload/main.py)."""
import sys

import pytest

import gsxtools.workload  # noqa: F401  (loads main.py as gsx_sample_workload)

wl = sys.modules["gsx_sample_workload"]


@pytest.mark.parametrize("new_tokens", (1, 2, 4, 16))
def test_mla_takes_1_to_16_new_tokens(new_tokens):
    assert wl.mla_refusal("attn", "gsx", new_tokens, 128, wl.MLA_KV_HEADS_DEFAULT) is None


@pytest.mark.parametrize("args,text", [
    (("attn", "gsx", 0, 16, 8), "--mla --new-tokens 0: need 1 <= T <= 16"),
    (("attn", "gsx", 17, 16, 8), "--mla --new-tokens 17: need 1 <= T <= 16"),
    (("server", "gsx", 4, 16, 8), "--workload attn only"),
    (("attn", "torch", 4, 16, 8), "--kernel gsx"),
    (("attn", "gsx", 4, 16, 4), "leave --kv-heads alone"),
    (("attn", "gsx", 4, 129, 8), "need 1 <= Hq <= 128"),
])
def test_mla_refusals_by_name(args, text):
    assert text in wl.mla_refusal(*args)
