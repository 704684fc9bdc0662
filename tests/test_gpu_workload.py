"""The workload's step functions (``server_steps``, ``layer_steps``, ``generate_steps``, ``prefill_steps`` of
``samples/workload/main.py``) on a real MI355X, in this process, through the workload's OWN ctypes binding
(``Kernels``), not ``ops/hip.py``.

A tracing wrapper (``workload_cases.Tracer``) stands where the step functions expect their ``Kernels``.  For every
kernel method it resolves each pointer argument to ``(buffer name, byte offset)`` through ``step.buffers`` (an address
inside no buffer, or an extent past a buffer's end, fails), compares the launch with the stage
``workload_cases.stages`` has at that place (a launch that is not the reference's is never made: no wrong pointer
reaches the device), forwards the call, waits for the stream and downloads the launch's outputs.  After every step all
buffers are downloaded.  ``workload_cases.check_trace`` then holds every launch to its kernel's own contract, computed
from the inputs as the GPU had them, and every buffer after every step to what the launches wrote.
``tests/test_workload_cases.py`` checks the checker, and runs the same step functions on the kernels' twins.

Buffers the workload allocates without initialising them are filled with a poison byte first, so that two runs start
from the same bytes.
"""
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import workload_cases as wc  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 20240
names = pytest.mark.parametrize("name", [c.name for c in wc.CONFIGS])


@pytest.fixture(scope="module")
def workload():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    import gsxtools.workload  # noqa: F401  (loads main.py as gsx_sample_workload)

    m = sys.modules["gsx_sample_workload"]
    path = m.kernels_lib_path()
    assert path is not None, "libgsx_kernels.so is not built"
    kl = m.Kernels(path)
    gs = kl.stream(0)
    yield m, kl, gs
    kl.destroy(gs)


@pytest.fixture(scope="module")
def traced(workload):
    """``name -> (initial buffers, trace, buffers after every step, finite())`` of the traced run, made once."""
    m, kl, gs = workload
    done = {}

    def run(name):
        if name not in done:
            done[name] = wc.run_traced(m, wc.config(name), kl, gs, SEED)
        return done[name]

    return run


@names
def test_every_launch_of_the_workload_is_the_reference_s_and_passes_its_check(traced, name):
    """The trace has exactly the reference's stages in order, with its buffers, slots and scalars; every stage passes
    its kernel's contract on the inputs the GPU had; after every step every buffer holds what the launches wrote and
    nothing else; the read-only buffers end as they began; ``finite()`` is true and the lengths end at
    ``start + (steps mod window)``."""
    c = wc.config(name)
    initial, trace, ends, finite = traced(name)
    mem = wc.check_trace(c, initial, trace, ends)
    assert finite is True
    assert all(np.array_equal(b, mem.b[n]) for n, b in ends[-1].items())
    if c.workload == "prefill":  # constant lengths: the second step rewrites the first, byte for byte
        for n, b in ends[0].items():
            assert np.array_equal(b, ends[1][n]), f"{n} after step 2 is not what it was after step 1"
    else:
        last = ends[-1][f"lens{(c.steps - 1) % c.window % 2}"].view(np.int32).tolist()
        assert last == [c.final_lens()] * c.batch, last
    if c.workload == "generate":
        gathers = [la for la in trace if la.kernel == "embed_gather"]
        samples = [la for la in trace if la.kernel == "sample"]
        for k in range(1, c.steps):
            assert gathers[k].args["tokens"] == samples[k - 1].args["tokens_out"], f"step {k} gathers other tokens"


@names
def test_the_untraced_run_leaves_the_same_bytes(workload, traced, name):
    """The same seed, the library's own ``Kernels``, no wait between launches: after the same number of steps every
    buffer is byte-equal to the traced run's.  The kernels are deterministic by their own tests, so tracing did not
    change what ran."""
    m, kl, gs = workload
    c = wc.config(name)
    initial, _, ends, _ = traced(name)
    step, sync, finite = wc.build_steps(m, c, kl, gs, SEED)
    start = wc.download(step.buffers)
    for n, b in initial.items():
        assert np.array_equal(start[n], b), f"{n}: the two runs do not start from the same bytes"
    for _ in range(c.steps):
        step()
    sync()
    for n, b in wc.download(step.buffers).items():
        assert np.array_equal(b, ends[-1][n]), f"{n} differs from the traced run"
    assert finite() is True
