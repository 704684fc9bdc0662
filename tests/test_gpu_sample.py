"""The token sampler and the embedding gather (native/kernels/sample.hip) on a real MI355X.

Every token must equal the twin of ``tests/sample_cases.py``, which ``tests/test_sample_cases.py`` checks on the CPU.
``tokens_out`` lies between guards of a poison pattern, and the logits between guard bands and row padding of the
largest finite bf16 code, so a read outside a row changes the result and a write anywhere but ``tokens_out[0..M)`` is
seen.  No case holds a size from which a wrong kernel could form an address outside the test's own allocations.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import sample_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
GUARD = 64  # elements of a guard band, and tokens of a guard
BAND = 0x7F7F  # the largest finite bf16: a logit read from a band or from padding would be the maximum
POISON32 = np.int32(np.uint32(0xA5A5A5A5).astype(np.int64) - (1 << 32))


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    from gpushare_scheduler_extender_amd.ops import hip as h

    assert h.SO.exists()
    assert hasattr(h, "sample") and hasattr(h, "embed_gather"), "the bindings have no sample / embed_gather"
    return h


@pytest.fixture(scope="module")
def stream(hip):
    s = hip.Stream(0)
    yield s
    s.destroy()


def _up(a: np.ndarray) -> torch.Tensor:
    """A NumPy array on the device, bit for bit."""
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint16): np.int16, np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).cuda()


class Dev:
    """A case on the device: logits between guard bands, every row padded with the band's code, ``tokens_out``
    between poisoned guards."""

    def __init__(self, case: sc.Case):
        self.case = case
        v, m = case.v, case.m
        self.stride = 0 if case.shared else v + case.pad
        rows, width = (1, v) if case.shared else (m, v + case.pad)
        host = np.full(2 * GUARD + rows * width, BAND, np.uint16)
        host[GUARD:GUARD + rows * width].reshape(rows, width)[:, :v] = case.bits.reshape(rows, v)
        self.host = host
        self.logits = _up(host)
        self.t = None if case.temperature is None else _up(case.temperature)
        self.k = None if case.top_k is None else _up(case.top_k)
        self.p = None if case.top_p is None else _up(case.top_p)
        self.s = None if case.seeds is None else _up(case.seeds)
        self.out = torch.full((2 * GUARD + m,), int(POISON32), dtype=torch.int32, device="cuda")

    def args(self, s, m=None, row=0):
        c = self.case

        def at(t, size):
            return 0 if t is None else t.data_ptr() + size * row

        return (s, self.logits.data_ptr() + 2 * (GUARD + row * self.stride), self.stride, at(self.t, 4), at(self.k, 4),
                at(self.p, 4), at(self.s, 8), c.counter, self.out.data_ptr() + 4 * (GUARD + row),
                c.m if m is None else m, c.v)

    def tokens(self, what: str) -> np.ndarray:
        out = self.out.cpu().numpy()
        assert bool((out[:GUARD] == POISON32).all()) and bool((out[GUARD + self.case.m:] == POISON32).all()), \
            f"{what}: a guard of tokens_out"
        assert np.array_equal(self.logits.cpu().numpy().view(np.uint16), self.host), f"{what}: the logits were written"
        return out[GUARD:GUARD + self.case.m].copy()

    def untouched(self) -> bool:
        return bool((self.out == int(POISON32)).all())


def _check(hip, stream, cases):
    devs = [Dev(c) for c in cases]
    torch.cuda.synchronize()  # the uploads are torch's: `stream` does not wait for torch's stream
    for d in devs:
        hip.sample(*d.args(stream))
    stream.sync()
    for d in devs:
        got, want = d.tokens(d.case.name), d.case.expected()
        assert bool(((got >= 0) & (got < d.case.v)).all()), f"{d.case.name}: a token outside [0, V)"
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{d.case.name}: {bad.size} of {got.size} rows, first row {bad[0]}: " \
                              f"{got[bad[0]]} for {want[bad[0]]}"


# ---- 1. equality with the twin -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("v", sc.GRID_V)
def test_tokens_equal_the_twin_over_sizes(hip, stream, v):
    _check(hip, stream, [sc.grid_case(v, m) for m in sc.GRID_M])


def test_4096_draws_from_one_row(hip, stream):
    case = sc.many_draws_case()
    assert case.m == 4096 and case.shared
    _check(hip, stream, [case])
    assert np.unique(case.expected()).size > 10


ROW_CASES = sc.sample_cases()[1:]


@pytest.mark.parametrize("case", ROW_CASES, ids=[c.name for c in ROW_CASES])
def test_rows_parameters_and_counters(hip, stream, case):
    _check(hip, stream, [case])


@pytest.mark.parametrize("flaw", sc.FLAWS)
def test_the_kernel_has_none_of_the_flaws(hip, stream, flaw):
    """The cases that tell each wrong twin from the right one, on the kernel."""
    _check(hip, stream, sc.flaw_cases()[flaw])


# ---- 2. determinism and independence ------------------------------------------------------------------------------------

def test_two_runs_and_a_masked_stream_are_bit_equal(hip, stream):
    case = sc.grid_case(128256, 17)
    a, b, c = Dev(case), Dev(case), Dev(case)
    masked = hip.Stream(0, hip.mask_words(range(0, 64)))
    try:
        torch.cuda.synchronize()
        hip.sample(*a.args(stream))
        hip.sample(*b.args(stream))
        hip.sample(*c.args(masked))
        stream.sync()
        masked.sync()
    finally:
        masked.destroy()
    ta = a.tokens("first")
    assert np.array_equal(ta, b.tokens("second")) and np.array_equal(ta, c.tokens("masked"))
    assert np.array_equal(ta, case.expected())


def test_a_row_alone_equals_the_row_in_its_batch(hip, stream):
    case = sc.grid_case(2056, 17)
    a, c = Dev(case), Dev(case)
    torch.cuda.synchronize()
    hip.sample(*a.args(stream))
    rows = (0, 5, 16)
    for row in rows:
        hip.sample(*c.args(stream, m=1, row=row))
    stream.sync()
    ta = a.tokens("batch")
    alone = c.out.cpu().numpy()[GUARD:GUARD + case.m]
    for row in range(case.m):
        assert alone[row] == (ta[row] if row in rows else POISON32), f"row {row}"


# ---- 3. refusals, timing --------------------------------------------------------------------------------------------------

def test_refused_calls_write_nothing(hip, stream):
    case = sc.grid_case(2056, 3)  # stride 2056 + 0 padding: M % 3 == 0
    d = Dev(case)
    good = list(d.args(stream))
    torch.cuda.synchronize()
    logits, out = good[1], good[8]
    bad = [({9: 0}, "need M >= 1"), ({10: 0}, "need 8 <= V <= 262144 and V % 8 == 0"), ({10: 2052}, "need 8 <= V <= 262144"),
           ({10: 262152, 2: 262152}, "need 8 <= V <= 262144"), ({2: 2048}, "need logits_stride == 0, or logits_stride >= V"),
           ({2: 2060}, "need logits_stride == 0, or"), ({2: -2056}, "need logits_stride == 0, or"),
           ({1: 0}, "logits and tokens_out must not be NULL"), ({8: 0}, "logits and tokens_out must not be NULL"),
           ({6: 0}, "seeds may be NULL only when temperature is NULL"), ({1: logits + 8}, "logits must be 16-B aligned"),
           ({3: good[3] + 2}, "temperature, top_k, top_p and tokens_out must be 4-B aligned"),
           ({4: good[4] + 1}, "temperature, top_k, top_p and tokens_out must be 4-B"),
           ({5: good[5] + 2}, "temperature, top_k, top_p and tokens_out must be 4-B"),
           ({8: out + 2}, "temperature, top_k, top_p and tokens_out must be 4-B"),
           ({6: good[6] + 4}, "seeds must be 8-B aligned"),
           ({8: logits + 16}, "tokens_out must not overlap logits, temperature, top_k, top_p or seeds"),
           ({8: good[3]}, "tokens_out must not overlap"), ({8: good[4]}, "tokens_out must not overlap"),
           ({8: good[5] + 8}, "tokens_out must not overlap"), ({8: good[6] + 20}, "tokens_out must not overlap")]
    assert all(any(t.startswith(rule[:24]) for _, t in bad) for rule in sc.SAMPLE_REFUSALS)  # every rule is tried
    for change, text in bad:
        a = list(good)
        for k, v in change.items():
            a[k] = v
        for fn, tail in ((hip.sample, ()), (hip.time_sample, (2,))):
            with pytest.raises(hip.HipError, match=f"gsx_sample: {text}"):
                fn(*a, *tail)
    stream.sync()
    assert d.untouched()
    assert np.array_equal(d.logits.cpu().numpy().view(np.uint16), d.host)
    for t, h in ((d.t, case.temperature), (d.k, case.top_k), (d.p, case.top_p)):
        assert np.array_equal(t.cpu().numpy(), h)

    table = torch.zeros(16 * 24, dtype=torch.int16, device="cuda")
    tokens = torch.zeros(4, dtype=torch.int32, device="cuda")
    o = torch.full((4 * 24,), 0x5A5A, dtype=torch.int16, device="cuda")
    good = [stream, table.data_ptr(), 24, tokens.data_ptr(), o.data_ptr(), 24, 4, 16, 16]
    torch.cuda.synchronize()
    bad = [({6: 0}, "need M >= 1"), ({8: 0}, "need V >= 1"), ({7: 0}, "need H >= 8 and H % 8 == 0"),
           ({7: 12}, "need H >= 8 and H % 8 == 0"), ({2: 8}, "need table_stride >= H and table_stride % 8 == 0"),
           ({2: 20}, "need table_stride >= H"), ({5: 8}, "need out_stride >= H and out_stride % 8 == 0"),
           ({5: 28}, "need out_stride >= H"), ({1: 0}, "table, tokens and out must not be NULL"),
           ({3: 0}, "table, tokens and out must not"), ({4: 0}, "table, tokens and out must not"),
           ({1: good[1] + 8}, "table and out must be 16-B aligned"), ({4: good[4] + 8}, "table and out must be 16-B"),
           ({3: good[3] + 2}, "tokens must be 4-B aligned"), ({4: good[1] + 32}, "out must not overlap table or tokens"),
           ({4: good[3]}, "out must not overlap table or tokens")]
    for change, text in bad:
        a = list(good)
        for k, v in change.items():
            a[k] = v
        for fn, tail in ((hip.embed_gather, ()), (hip.time_embed_gather, (2,))):
            with pytest.raises(hip.HipError, match=f"gsx_embed_gather: {text}"):
                fn(*a, *tail)
    stream.sync()
    assert bool((o == 0x5A5A).all()) and not bool(table.any()) and not bool(tokens.any())


def test_timed_entry_points_leave_the_result(hip, stream):
    case = sc.grid_case(65544, 3)
    d = Dev(case)
    rng = np.random.default_rng(1)
    table = rng.integers(0, 65536, (32, 136), dtype=np.uint16)
    tok = np.array([31, 0, 7], np.int32)
    tb, tk = _up(table), _up(tok)
    o = torch.zeros((3, 136), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    ms = [hip.time_sample(*d.args(stream), 3),
          hip.time_embed_gather(stream, tb.data_ptr(), 136, tk.data_ptr(), o.data_ptr(), 136, 3, 136, 32, 3)]
    stream.sync()
    assert min(ms) > 0, ms
    assert np.array_equal(d.tokens("timed"), case.expected())
    assert np.array_equal(o.cpu().numpy().view(np.uint16), table[tok])


# ---- 4. gsx_embed_gather ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,table_pad,out_pad", [(8, 0, 0), (136, 8, 24), (8192, 16, 8)])
def test_embed_gather_byte_for_byte(hip, stream, h, table_pad, out_pad):
    """Rows between guard rows; tokens -1, V and INT_MAX give rows of zeros next to the guards."""
    rng = np.random.default_rng(h)
    v, ts, os_ = 300, h + table_pad, h + out_pad
    table = rng.integers(1, 65536, (v, ts), dtype=np.uint16)
    tok = np.array([-1, 5, v, 299, sc.INT_MAX, 0, 5, -2 ** 31, 123, v - 1, sc.INT_MAX], np.int32)
    m, g = tok.size, 2
    tb, tk = _up(table), _up(tok)
    o = torch.full((m + 2 * g, os_), 0x5A5A, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    hip.embed_gather(stream, tb.data_ptr(), ts, tk.data_ptr(), o.data_ptr() + 2 * g * os_, os_, m, h, v)
    stream.sync()
    out = o.cpu().numpy().view(np.uint16)
    assert bool((out[:g] == 0x5A5A).all()) and bool((out[g + m:] == 0x5A5A).all()), "a guard row"
    assert bool((out[g:g + m, h:] == 0x5A5A).all()), "the padding of a row"
    want = sc.embed_reference(table, tok, h)
    assert not want[[0, 2, 4, 7, 10]].any() and want[1].any()
    assert np.array_equal(out[g:g + m, :h], want)
    assert np.array_equal(tb.cpu().numpy().view(np.uint16), table)


def test_embed_gather_from_a_table_past_4_gib(hip, stream):
    """V x stride x 2 B = 4.3 GB: the rows read lie on either side of byte offsets 2^31 and 2^32."""
    h, ts, v = 16, 8192, 263000
    table = torch.empty((v, ts), dtype=torch.int16, device="cuda")  # only the rows that are read are initialised
    rows = [0, 2 ** 31 // (2 * ts) - 1, 2 ** 31 // (2 * ts), 2 ** 32 // (2 * ts) - 1, 2 ** 32 // (2 * ts), v - 1]
    rng = np.random.default_rng(2)
    vals = rng.integers(1, 65536, (len(rows), h), dtype=np.uint16)
    table[rows, :h] = _up(vals)
    tok = np.array(rows + [v], np.int32)
    tk = _up(tok)
    o = torch.full((tok.size + 2, h), 0x5A5A, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    hip.embed_gather(stream, table.data_ptr(), ts, tk.data_ptr(), o.data_ptr() + 2 * h, h, tok.size, h, v)
    stream.sync()
    out = o.cpu().numpy().view(np.uint16)
    assert bool((out[0] == 0x5A5A).all()) and bool((out[-1] == 0x5A5A).all())
    assert np.array_equal(out[1:-2], vals) and not out[-2].any()


# ---- 5. chained: embed, LM head, sample, without a host sync -----------------------------------------------------------

def test_33_steps_of_embed_lm_head_and_sample(hip, stream):
    """Each step's tokens feed the next step's gather through device memory; every step keeps its logits, and the twin
    is run on them afterwards.  Rows differ in their parameters; one row is greedy."""
    rng = np.random.default_rng(5)
    steps, m, h, v = 33, 3, 64, 528
    table = sc.bf16_bits(rng.standard_normal((v, h)).astype(np.float32))
    head = sc.bf16_bits(rng.standard_normal((v, h)).astype(np.float32) * np.float32(0.5))
    t = np.array([0.9, 0.0, 1.4], np.float32)
    k = np.array([40, 0, 0], np.int32)
    p = np.array([0.9, 1.0, 0.97], np.float32)
    seeds = sc.seeds_for(m, 77)
    tb, hd, td, kd, pd, sd = _up(table), _up(head), _up(t), _up(k), _up(p), _up(seeds)
    toks = torch.zeros((steps + 1, m), dtype=torch.int32, device="cuda")
    toks[0] = torch.tensor([1, 2, 3], dtype=torch.int32)
    x = torch.zeros((m, h), dtype=torch.int16, device="cuda")
    logits = torch.zeros((steps, m, v), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    for s in range(steps):
        hip.embed_gather(stream, tb.data_ptr(), h, toks[s].data_ptr(), x.data_ptr(), h, m, h, v)
        hip.decode_gemm_nt(stream, "bf16", x.data_ptr(), hd.data_ptr(), logits[s].data_ptr(), m, v, h)
        hip.sample(stream, logits[s].data_ptr(), v, td.data_ptr(), kd.data_ptr(), pd.data_ptr(), sd.data_ptr(), s,
                   toks[s + 1].data_ptr(), m, v)
    stream.sync()
    got = toks.cpu().numpy()
    lg = logits.cpu().numpy().view(np.uint16)
    assert np.unique(got[1:, 0]).size > 4 and bool(np.isfinite(sc.bf16_value(lg)).all())
    for s in range(steps):
        want = [sc.sample(lg[s, r], t[r], int(k[r]), p[r], int(seeds[r]), s) for r in range(m)]
        assert got[s + 1].tolist() == want, f"step {s}"
    # the logits of step s are those of the tokens of step s: the gather fed the GEMM
    ref = sc.bf16_value(table[got[5]]).astype(np.float64) @ sc.bf16_value(head).astype(np.float64).T
    assert float(np.abs(sc.bf16_value(lg[5]).astype(np.float64) - ref).max()) <= 2.0 ** -7 * float(np.abs(ref).max())


# ---- 6. the workload, end to end ---------------------------------------------------------------------------------------

def test_workload_generate_end_to_end():
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "gsxtools.workload", "--workload", "generate", "--batch", "4",
                        "--context", "512", "--heads", "8", "--kv-heads", "2", "--kv-gib", "0.003", "--weights-gib",
                        "0.05", "--vocab", "2048", "--iters", "70", "--json"],  # two layers of weights and of KV
                       env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["workload"] == "generate" and out["batch"] == 4 and out["vocab"] == 2048 and out["layers"] == 2
    assert out["tokens_per_s"] > 0 and out["bytes_per_step"] > 0 and out["iters"] >= 70
    assert out["activations_finite"] is True and out["tokens_in_range"] is True
    assert out["kernel"] == "gsx" and out["kernels_lib"].endswith("libgsx_kernels.so")
