"""The checks of ``tests/workload_cases.py`` on the CPU: the checker that ``tests/test_gpu_workload.py`` holds the
workload's step functions to accepts a faithful simulation of every configuration and rejects every flawed one at the
stage the flaw corrupts."""
import dataclasses
import importlib.util
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import gemm_decode_cases as dc  # noqa: E402
from tests import kv_append_cases as kc  # noqa: E402
from tests import workload_cases as wc  # noqa: E402

names = pytest.mark.parametrize("name", [c.name for c in wc.CONFIGS])


@pytest.fixture(scope="module")
def main_py():
    import gsxtools.workload  # noqa: F401  (loads main.py as gsx_sample_workload)

    return sys.modules["gsx_sample_workload"]


@names
def test_the_step_functions_launch_the_reference_s_stages(main_py, name):
    """The workload's own step functions on tensors in host memory, the kernels' twins in place of the library: every
    launch they make is the reference's, pointer for pointer and scalar for scalar, and passes its check."""
    c = wc.config(name)
    initial, trace, ends, finite = wc.run_traced(main_py, c, seed=11)
    wc.check_trace(c, initial, trace, ends)
    assert finite is True and len(trace) == len(wc.stages(c))
    if c.workload == "prefill":
        assert all(np.array_equal(b, ends[1][n]) for n, b in ends[0].items())


MUTATIONS = {  # (old text, new text, which occurrence, configuration, the stage that has to be named)
    "the other weight slot": ("wi = i % w_layers\n", "wi = i % w_layers ^ 1\n", 0, "moe", "step 0, layer 0, norm1"),
    "a_div 1 on the up projection": ("xn.data_ptr(), active, wgu.data_ptr()", "xn.data_ptr(), 1, wgu.data_ptr()", 0,
                                     "moe", "step 0, layer 0, up"),
    "lens swapped": ("lens_in.data_ptr(), lens_out.data_ptr(), cos", "lens_out.data_ptr(), lens_in.data_ptr(), cos", 0,
                     "server-bf16", "step 0, layer 0, append"),
    "plan of layer 0": ("plans.data_ptr() + i * MOE_PLAN_INTS * 4", "plans.data_ptr()", 0, "moe",
                        "step 0, layer 1, route"),
    "the sampler's counter": ("seeds.data_ptr(), n,\n", "seeds.data_ptr(), 0,\n", 0, "generate", "step 1, sample"),
    "the window never restarts": ("k = count[0] % window\n", "k = count[0]\n", 0, "server-bf16",
                                  "step 40, layer 0, append"),
}


@pytest.mark.parametrize("what", list(MUTATIONS))
def test_a_mutated_main_py_is_rejected_at_its_stage(main_py, what):
    """The text of ``main.py`` with one expression changed, loaded as a module of its own: its step function fails,
    and the failure names the stage."""
    old, new, nth, name, stage = MUTATIONS[what]
    src = open(main_py.__file__, encoding="utf-8").read()
    parts = src.split(old)
    assert len(parts) > nth + 1, f"main.py no longer holds {old!r}: write this mutation anew"
    src = old.join(parts[:nth + 1]) + new + old.join(parts[nth + 1:])
    mod = importlib.util.module_from_spec(importlib.util.spec_from_loader("gsx_sample_workload_mutant", loader=None))
    mod.__file__ = main_py.__file__
    sys.modules[mod.__name__] = mod  # dataclasses and the like look the module up
    try:
        exec(compile(src, main_py.__file__, "exec"), mod.__dict__)
        with pytest.raises(wc.StageError, match=stage):
            wc.run_traced(mod, wc.config(name), seed=11)
    finally:
        del sys.modules[mod.__name__]


@names
def test_the_checker_accepts_the_simulation(name):
    """Every launch of the twins' run, with the configuration's own step count (the server's 42 steps wrap the
    window), passes its stage's check, the buffers after every step are what the launches wrote, the read-only
    buffers are untouched and the lengths end where they have to."""
    c, initial, trace, step_ends = wc.simulated(name)
    assert len(trace) == len(wc.stages(c)) and len(step_ends) == c.steps
    mem = wc.check_trace(c, initial, trace, step_ends)
    for n, b in step_ends[-1].items():
        assert np.array_equal(b, mem.b[n]), n
    if c.workload == "prefill":  # the lengths are constant: a step rewrites the same slots with the same values
        for n in step_ends[0]:
            assert np.array_equal(step_ends[0][n], step_ends[1][n]), n


def test_the_server_window_restarts():
    c, _, trace, _ = wc.simulated("server-bf16")
    appends = [la for la in trace if la.kernel == "kv_append"]
    per_step = c.layers
    assert c.window == 40 and c.start == 0 and c.context % c.page
    assert [appends[k * per_step].args["lens"][0] for k in (0, 1, 2, 39, 40, 41)] == \
        ["start", "lens0", "lens1", "lens0", "start", "lens0"]
    assert c.final_lens() == 2 and dataclasses.replace(c, steps=40).final_lens() == c.context


@pytest.mark.parametrize("flaw", wc.FLAWS)
def test_the_checker_rejects_a_flawed_workload_at_its_stage(flaw):
    name, (step, layer, label) = wc.flaw_cases()[flaw]
    c, initial, trace, step_ends = wc.simulate(wc.config(name), steps=step + 1, flaw=flaw)
    with pytest.raises(wc.StageError) as e:
        wc.check_trace(c, initial, trace, step_ends)
    st = e.value.stage
    assert (st.step, st.layer, st.label) == (step, layer, label), str(e.value)
    assert f"step {step}, " in str(e.value) and label in str(e.value)


def test_every_flaw_has_a_case_and_every_case_a_configuration():
    cases = wc.flaw_cases()
    assert sorted(cases) == sorted(wc.FLAWS)
    assert {n for n, _ in cases.values()} <= {c.name for c in wc.CONFIGS}


def test_a_write_outside_a_launch_and_a_written_input_are_found():
    c, initial, trace, step_ends = wc.simulated("layer-bf16")
    ends = [dict(s) for s in step_ends]
    ends[1]["wo"] = ends[1]["wo"].copy()
    ends[1]["wo"][5] ^= 1
    with pytest.raises(wc.StageError, match="after step 1 wo differs"):
        wc.check_trace(c, initial, trace, ends)
    with pytest.raises(wc.StageError, match="was never launched"):
        wc.check_trace(c, initial, trace[:-1])
    bad = list(trace)
    out = {p: b.copy() for p, b in trace[3].outputs.items()}
    out["o"][1] ^= 0x40  # one element of the first attention's output, far outside its bound
    bad[3] = wc.Launch(trace[3].kernel, trace[3].args, out)
    with pytest.raises(wc.StageError, match=r"step 0, layer 0, attn \(decode_attn\)"):
        wc.check_trace(c, initial, bad)


def test_every_named_buffer_is_addressed_by_some_stage():
    for workload in ("server", "layer", "generate", "prefill"):
        cs = [c for c in wc.CONFIGS if c.workload == workload]
        named = set().union(*(wc.buffer_shapes(c) for c in cs))
        assert named == set().union(*(wc.covered_buffers(c) for c in cs)), workload


def test_the_rope_tables_are_those_of_the_append_tests():
    """Two fp64 evaluations, each rounded once to fp32, of values in [-1, 1]."""
    for n in (40, 80):
        for mine, theirs in zip(wc.rope_tables(n), kc.real_tables(n)):
            assert mine.dtype == np.float32 and mine.shape == (n, 64)
            assert np.abs(mine.astype(np.float64) - theirs).max() <= 2.0 ** -23


def test_an_fp32_matmul_rounded_to_bf16_is_inside_the_gemm_bound_at_the_prefill_shapes():
    """``gemm_decode_cases.error_bound`` is one rounding to bf16 and K fp32 accumulations: it holds for any GEMM that
    accumulates in fp32, so also for the large GEMM on the prefill workload's general inputs."""
    c = wc.config("prefill-bf16")
    g = torch.Generator().manual_seed(3)
    for n, k in ((c.nqkv, c.hidden), (c.hidden, c.hidden), (2 * c.ffn, c.hidden), (c.hidden, c.ffn)):
        a = torch.randn(c.rows, k, generator=g).bfloat16()
        b = (torch.randn(n, k, generator=g) / k ** 0.5).bfloat16()
        got = (a.float() @ b.float().t()).bfloat16().double()
        ref, mag = a.double() @ b.double().t(), a.double().abs() @ b.double().abs().t()
        assert bool(((got - ref).abs() <= dc.error_bound(ref, mag, k)).all()), (n, k)


def test_the_extents_cover_what_the_stages_address():
    """Every pointer of every stage, with its extent, lies inside its buffer."""
    for c in wc.CONFIGS:
        sizes = {n: len(b) for n, b in wc.initial_buffers(c).items()}
        for st in wc.stages(c):
            ext = wc.extents(st.kernel, {**st.args, "ws_bytes": sizes.get("ws", 0)})
            for p in wc.POINTERS[st.kernel]:
                if st.args[p] is not None:
                    name, off = st.args[p]
                    assert off + ext[p] <= sizes[name], f"{c.name}, {st}: {p}"
