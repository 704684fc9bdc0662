"""RoPE + KV append (native/kernels/kv_append.hip) on a real MI355X.

Problems and the NumPy twin of the contract are those of ``tests/kv_append_cases.py``, which
``tests/test_kv_append_cases.py`` checks on the CPU.  Every comparison is on raw bytes (the two NaN codes of e4m3 count
as one).  ``Q_out``, both caches with their three guard pages on either side, and ``lens_out`` are filled with a
poison pattern before a launch and compared WHOLE with the twin's, which starts from the same poison: a stray write
fails.  No case holds an index or a length from which a wrong kernel could form an address outside one of the test's
own allocations, except the lengths of -1 and -2^31 that the contract takes as 0: bad block-table entries are -3..-1
and num_pages..num_pages + 2, which lie in the guard pages, and the block table has a spare row.
"""
import dataclasses
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import kv_append_cases as kc  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
kinds = pytest.mark.parametrize("kind", kc.KINDS)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    from gpushare_scheduler_extender_amd.ops import hip as h

    assert h.SO.exists()
    assert hasattr(h, "kv_append"), "the bindings have no kv_append"
    return h


@pytest.fixture(scope="module")
def stream(hip):
    s = hip.Stream(0)
    yield s
    s.destroy()


def _up(a: np.ndarray) -> torch.Tensor:
    """A NumPy array on the device, bit for bit (unsigned 16-bit as int16)."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _poison(nbytes: int) -> torch.Tensor:
    return torch.full((nbytes,), kc.POISON8, dtype=torch.uint8, device="cuda")


def _down(t: torch.Tensor, dtype, shape) -> np.ndarray:
    return t.cpu().numpy().view(dtype).reshape(shape)


class Dev:
    """A problem's operands on the device and poisoned outputs; ``run`` launches (not synchronised), ``result`` reads
    everything the kernel may have written back."""

    def __init__(self, p: kc.Problem, place=None):
        self.p = p
        place = place or (lambda t, fill=0: t)
        esz = 2 if p.kind == "bf16" else 1
        self.page_bytes = p.hkv * p.page * kc.D * esz
        self.pages = kc.GUARD + p.num_pages + kc.GUARD
        self.qkv, self.table, self.lens, self.cos, self.sin = (
            place(_up(a)) for a in (p.qkv, p.table, p.seq_lens, p.cos, p.sin))
        self.q_out = place(_poison(p.b * p.t * p.hq * kc.D * 2))
        self.k, self.v = place(_poison(self.pages * self.page_bytes)), place(_poison(self.pages * self.page_bytes))
        self.lens_out = place(_poison(p.b * 4))

    def args(self, s, lens_out=True):
        p = self.p
        return (s, p.kind, self.qkv.data_ptr(), p.qkv_stride, self.q_out.data_ptr(),
                self.k.data_ptr() + kc.GUARD * self.page_bytes, self.v.data_ptr() + kc.GUARD * self.page_bytes,
                self.table.data_ptr(), self.lens.data_ptr(), self.lens_out.data_ptr() if lens_out else 0,
                self.cos.data_ptr(), self.sin.data_ptr(), p.rope_len, p.b, p.t, p.hq, p.hkv, kc.D, p.page, p.num_pages,
                p.table_stride, p.max_seq_len)

    def run(self, hip, s, lens_out=True):
        torch.cuda.synchronize()  # the uploads and fills are torch's: `s` does not wait for torch's stream
        hip.kv_append(*self.args(s, lens_out), self.p.k_inv, self.p.v_inv)
        return self

    def result(self) -> kc.Result:
        p = self.p
        cdt = np.uint16 if p.kind == "bf16" else np.uint8
        shape = (self.pages, p.hkv, p.page, kc.D)
        return kc.Result(_down(self.q_out, np.uint16, (p.b * p.t, p.hq, kc.D)), _down(self.k, cdt, shape),
                         _down(self.v, cdt, shape), _down(self.lens_out, np.int32, (p.b,)))


def _same(kind: str, got: np.ndarray, want: np.ndarray) -> np.ndarray:
    return kc.same_e4m3(got, want) if kind == "fp8" and got.dtype == np.uint8 else got == want


def assert_result(p: kc.Problem, got: kc.Result, want: kc.Result, what: str, lens_out=True):
    for name, g, w in (("Q_out", got.q_out, want.q_out), ("K_cache", got.k, want.k), ("V_cache", got.v, want.v)):
        bad = np.argwhere(~_same(p.kind, g, w))
        if len(bad):
            at = tuple(int(x) for x in bad[0])
            raise AssertionError(f"{what}: {len(bad)} of {g.size} elements of {name} differ; first at {at} "
                                 f"(token or page, head, [slot,] d): got {int(g[at]):#06x}, want {int(w[at]):#06x}")
    want_lens = want.lens_out if lens_out else np.full_like(want.lens_out, kc.POISON32)
    assert got.lens_out.tolist() == want_lens.tolist(), f"{what}: lens_out"


def _check(hip, stream, cases, what):
    """Every case launched first, compared afterwards."""
    runs = [(name, p, Dev(p).run(hip, stream)) for name, p in cases]
    stream.sync()
    for name, p, d in runs:
        assert_result(p, d.result(), kc.twin(p), f"{what}, {name}")


# ---- 1. addressing -----------------------------------------------------------------------------------------------------

@kinds
def test_kv_append_puts_every_token_into_its_slot(hip, stream, kind):
    """``kv_append_cases.addressing_cases``: identity table, elements that name their token, head row and d."""
    _check(hip, stream, kc.addressing_cases(kind), kind)


@kinds
def test_kv_append_without_lens_out_leaves_it_alone(hip, stream, kind):
    name, p = kc.addressing_cases(kind)[3]
    d = Dev(p).run(hip, stream, lens_out=False)
    stream.sync()
    assert_result(p, d.result(), kc.twin(p), f"{kind}, {name}, lens_out NULL", lens_out=False)


# ---- 2. dropped pages --------------------------------------------------------------------------------------------------

@kinds
def test_kv_append_drops_a_bad_page_index(hip, stream, kind):
    """Entries of -3..-1 and num_pages..num_pages + 2 under tokens that would be live: nothing is written for them
    anywhere (the guard pages on either side of the caches stay poison) and their Q_out rows are zero."""
    _check(hip, stream, kc.dropped_page_cases(kind), kind)


# ---- 3. rotation -------------------------------------------------------------------------------------------------------

@kinds
def test_kv_append_rotates_bit_for_bit(hip, stream, kind):
    """Random bf16 rows against a real cos / sin table with positions up to 4095, zeros of both signs, and the
    cancellation case, which a kernel that contracts a product into the subtraction fails."""
    _check(hip, stream, kc.rotation_cases(kind) + [("cancellation", kc.cancellation_problem(kind))], kind)


# ---- 4. every bf16 code ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("through,inv", [("v", 1.0), ("v", 1 / 3), ("k0", 1.0), ("k1", 1.0), ("k0", 0.5), ("k1", 0.5)],
                         ids=["v-1", "v-third", "k0-1", "k1-1", "k0-half", "k1-half"])
def test_kv_append_converts_every_bf16_code_to_e4m3(hip, stream, through, inv):
    """All 65,536 bf16 codes as V elements with v_inv_scale 1.0 and 1/3, and through K under the identity table with
    k_inv_scale 1.0 and 0.5: every midpoint between two e4m3 codes that bf16 holds, every saturating value, +-inf
    (+-448) and every NaN payload (a NaN code)."""
    p = kc.sweep_problem("fp8", through, float(np.float32(inv)))
    d = Dev(p).run(hip, stream)
    stream.sync()
    assert_result(p, d.result(), kc.twin(p), f"fp8, all codes through {through}, inverse scale {inv}")


def test_kv_append_copies_every_bf16_code_of_v(hip, stream):
    p = kc.sweep_problem("bf16", "v", 1.0)
    d = Dev(p).run(hip, stream)
    stream.sync()
    got = d.result()
    assert_result(p, got, kc.twin(p), "bf16, all codes through V")
    rows = np.stack([got.v[kc.GUARD + pp, 0, slot] for _, pp, slot in p.live()])
    assert np.array_equal(rows, kc.all_codes())


# ---- 5. guard bands and 16-B-only alignment ----------------------------------------------------------------------------

def _banded(t: torch.Tensor, fill: int = 0xC3):
    """``t`` 16 B past a 256-B boundary inside a byte allocation filled with ``fill``: the view."""
    raw = t.contiguous().view(torch.uint8).flatten()
    whole = torch.full((4096 + 16 + raw.numel() + 4096,), fill, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 256 == 0
    whole[4096 + 16:4096 + 16 + raw.numel()] = raw
    view = whole[4096 + 16:4096 + 16 + raw.numel()].view(t.dtype).view(t.shape)
    assert view.data_ptr() % 32 == 16
    view.whole = whole
    return view


@kinds
def test_kv_append_guard_bands_and_minimum_alignment(hip, stream, kind):
    """Every operand 16 B past a 256-B boundary between bands of 0xC3 bytes: the bands of all of them, inputs
    included, stay as they were, and the result is the twin's."""
    p = kc.make_problem(kind, 3, 5, 21, 3, 16, [14, 0, 29], pad=8, extra_stride=1,
                        **({} if kind == "bf16" else {"k_inv": 0.5, "v_inv": 2.0}))
    d = Dev(p, place=_banded)
    tensors = (d.qkv, d.table, d.lens, d.cos, d.sin, d.q_out, d.k, d.v, d.lens_out)
    inputs = [t.whole.clone() for t in tensors[:5]]
    d.run(hip, stream)
    stream.sync()
    assert_result(p, d.result(), kc.twin(p), f"{kind}, banded")
    for t in tensors:
        n = t.numel() * t.element_size()
        assert bool((t.whole[:4096 + 16] == 0xC3).all()) and bool((t.whole[4096 + 16 + n:] == 0xC3).all()), \
            f"{kind}: a band was written"
    for t, before in zip(tensors[:5], inputs):
        assert torch.equal(t.whole, before), f"{kind}: an input was written"


# ---- 6. a cache past 4 GiB ---------------------------------------------------------------------------------------------

def test_kv_append_cache_past_4_gib(hip, stream):
    """bf16, Hkv = 2, page 64: a page is 32 KiB, so page 131072 starts at byte 2^32.  The case's pages lie past that
    offset.  The touched pages and their neighbours are compared on the host with the twin of the same case at page
    base 0; everything else is compared with the fill on the device."""
    page_bytes = 2 * 64 * kc.D * 2
    first = (1 << 32) // page_bytes + 5
    small = kc.make_problem("bf16", 3, 70, 8, 2, 64, [0, 63, 100])
    table = small.table + np.int32(first)
    p = dataclasses.replace(small, table=table, num_pages=small.num_pages + first)
    pages = kc.GUARD + p.num_pages + kc.GUARD
    k, v = _poison(pages * page_bytes), _poison(pages * page_bytes)
    d = Dev(small)  # the small operands; the caches and the table are the large problem's
    d.p, d.k, d.v, d.pages, d.table = p, k, v, pages, _up(table)
    d.run(hip, stream)
    stream.sync()
    want = kc.twin(small)
    near = want.k.shape[0]  # GUARD + the small problem's pages + GUARD, which lie at page `first` of the large cache
    lo, hi = first * page_bytes, (first + near) * page_bytes
    assert lo + kc.GUARD * page_bytes > 1 << 32
    for name, cache, w in (("K_cache", k, want.k), ("V_cache", v, want.v)):
        got = cache[lo:hi].cpu().numpy().view(np.uint16).reshape(w.shape)
        assert np.array_equal(got, w), f"{name}: the pages past byte 2^32"
        for a, b in ((0, lo), (hi, cache.numel())):
            for at in range(a, b, 1 << 29):
                assert bool((cache[at:min(at + (1 << 29), b)] == kc.POISON8).all()), f"{name}: a write near byte {at}"
    assert np.array_equal(_down(d.q_out, np.uint16, want.q_out.shape), want.q_out)
    assert _down(d.lens_out, np.int32, (3,)).tolist() == want.lens_out.tolist()
    del k, v, d
    torch.cuda.empty_cache()


# ---- 7. determinism and the timing entry point -------------------------------------------------------------------------

@kinds
def test_kv_append_is_deterministic_and_placement_free(hip, stream, kind):
    """Two runs, and a run on a stream masked to CUs 0 .. 63, are bit-equal (and the twin's)."""
    _, p = kc.rotation_cases(kind)[1]
    masked = hip.Stream(0, hip.mask_words(range(0, 64)))
    try:
        runs = [Dev(p).run(hip, s) for s in (stream, stream, masked)]
        stream.sync()
        masked.sync()
    finally:
        masked.destroy()
    want = kc.twin(p)
    for i, d in enumerate(runs):
        assert_result(p, d.result(), want, f"{kind}, run {i}")


@kinds
def test_time_kv_append_leaves_the_result(hip, stream, kind):
    name, p = kc.addressing_cases(kind)[4]
    d = Dev(p)
    torch.cuda.synchronize()
    with pytest.raises(hip.HipError, match="gsx_kv_append: need D == 128"):
        hip.time_kv_append(*d.args(stream)[:17], 64, *d.args(stream)[18:], 3, p.k_inv, p.v_inv)
    assert bool((d.q_out == kc.POISON8).all())
    ms = hip.time_kv_append(*d.args(stream), 3, p.k_inv, p.v_inv)
    stream.sync()
    assert ms > 0, ms
    assert_result(p, d.result(), kc.twin(p), f"time_kv_append, {kind}, {name}")


# ---- 8. chained with the attention -------------------------------------------------------------------------------------

@kinds
def test_kv_append_chained_with_decode_attn(hip, stream, kind):
    """33 decode steps (T = 1, pages of 16, lengths that cross the 32-token tile, one sequence that reaches
    max_seq_len) launched back to back on one stream, each followed by the attention over the cache as it then is;
    lens_out ping-pongs between two buffers and nothing waits for the host.  The caches and the final lengths are the
    twin's, and the last attention is bit-equal to the attention over a cache uploaded from the twin."""
    problems, final = kc.chain_problem(kind)
    p0 = problems[0]
    d = Dev(p0)
    steps = len(problems)
    qkv = _up(np.stack([p.qkv for p in problems]))
    q_out = _poison(steps * p0.b * p0.hq * kc.D * 2)
    o = _poison(steps * p0.b * p0.hq * kc.D * 2)
    lens = [_poison(p0.b * 4), _poison(p0.b * 4)]
    ws_bytes = hip.decode_attn_workspace_bytes(p0.b, p0.hq, kc.D, p0.page, p0.max_seq_len)
    ws = torch.zeros(max(ws_bytes, 16), dtype=torch.uint8, device="cuda")
    step_q = p0.b * p0.hq * kc.D * 2
    k_scale, v_scale = 1.0 / p0.k_inv, 1.0 / p0.v_inv

    def attend(q_ptr, k, v, lens_ptr, o_ptr):
        hip.decode_attn(stream, kind, q_ptr, k.data_ptr() + kc.GUARD * d.page_bytes,
                        v.data_ptr() + kc.GUARD * d.page_bytes, d.table.data_ptr(), lens_ptr, o_ptr, p0.b, p0.hq,
                        p0.hkv, kc.D, p0.page, p0.num_pages, p0.table_stride, p0.max_seq_len, kc.D ** -0.5, k_scale,
                        v_scale, ws.data_ptr(), ws.numel())

    torch.cuda.synchronize()
    for i in range(steps):
        lens_in = d.lens if i == 0 else lens[(i - 1) % 2]
        args = list(d.args(stream))
        args[2], args[4] = qkv.data_ptr() + i * p0.qkv.nbytes, q_out.data_ptr() + i * step_q
        args[8], args[9] = lens_in.data_ptr(), lens[i % 2].data_ptr()
        hip.kv_append(*args, p0.k_inv, p0.v_inv)
        attend(args[4], d.k, d.v, lens[i % 2].data_ptr(), o.data_ptr() + i * step_q)
    stream.sync()
    want = kc.chain_twin(problems)
    got = d.result()
    got.q_out = _down(q_out, np.uint16, (steps, p0.b, p0.hq, kc.D))[-1]
    got.lens_out = _down(lens[(steps - 1) % 2], np.int32, (p0.b,))
    assert want.lens_out.tolist() == final
    assert_result(p0, got, want, f"{kind}, the chain")
    # the reference attention: the twin's cache and Q, uploaded
    rk, rv, rq = _up(want.k), _up(want.v), _up(want.q_out)
    ro = _poison(step_q)
    torch.cuda.synchronize()
    attend(rq.data_ptr(), rk, rv, lens[(steps - 1) % 2].data_ptr(), ro.data_ptr())
    stream.sync()
    last = o[(steps - 1) * step_q:]
    assert torch.equal(last, ro), f"{kind}: the attention over the appended cache is not the one over the twin's"
    rows = _down(last, np.uint16, (p0.b, p0.hq, kc.D))
    assert bool(np.isfinite(kc.bf16_value(rows)).all()) and bool(rows[:2].any())


# ---- 9. the workload, end to end ---------------------------------------------------------------------------------------

@kinds
def test_workload_server_end_to_end(kind):
    """``gsxtools.workload --workload server``: more steps than the window, so the lengths start again once."""
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "gsxtools.workload", "--workload", "server", "--kv-dtype", kind,
                        "--batch", "4", "--context", "512", "--heads", "8", "--kv-heads", "2", "--kv-gib", "0.01",
                        "--weights-gib", "0.01", "--iters", "70", "--json"],
                       env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["workload"] == "server" and out["batch"] == 4 and out["kv_dtype"] == kind and out["context"] == 512
    assert (out["heads"], out["kv_heads"], out["page"], out["window"]) == (8, 2, 16, 64)
    assert out["weight_layers"] >= 2 and out["kv_layers"] >= 2 and out["layers"] == max(out["weight_layers"],
                                                                                       out["kv_layers"])
    assert out["tbps"] > 0 and out["tokens_per_s"] > 0 and out["iters"] >= 70
    assert out["activations_finite"] is True
    assert out["kernel"] == "gsx" and out["kernels_lib"].endswith("libgsx_kernels.so")
