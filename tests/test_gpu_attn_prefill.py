"""The prefill attention (native/kernels/attn_prefill.hip) on a real MI355X.

Problems, the fp64 reference, the twin and the error bound are those of ``tests/attn_prefill_cases.py``, which
``tests/test_attn_prefill_cases.py`` checks on the CPU.  The staircase cases are compared on the raw 16 bits of every
element (the causal mask, the tiles, the pages); the count and random cases with the derived bound.  Every O lies
between guard rows of poison that have to stay poison, and starts as NaN, so a row that is not written shows.  One
case holds a page index above ``num_pages - 1`` and its caches reach three pages further than ``num_pages`` says; no
other index is out of range, so a wrong kernel fails a comparison and reads nothing outside an allocation.
"""
import ctypes
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import attn_decode_cases as ac  # noqa: E402
from tests import attn_prefill_cases as pc  # noqa: E402
from tests import kv_append_cases as kc  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
G = 4  # guard rows on either side of O
POISON8 = 0xA5
kinds = pytest.mark.parametrize("kind", pc.KINDS)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    from gpushare_scheduler_extender_amd.ops import hip as h

    assert h.SO.exists()
    assert hasattr(h, "prefill_attn"), "the bindings have no prefill attention"
    return h


@pytest.fixture(scope="module")
def stream(hip):
    s = hip.Stream(0)
    yield s
    s.destroy()


class Guarded:
    """``rows`` rows of ``hq * 128`` bf16 between G guard rows of poison bytes on either side; the rows themselves
    start as NaN (0xFFFF).  ``ptr`` is the address of row 0."""

    def __init__(self, rows: int, hq: int):
        self.rows, self.hq = rows, hq
        self.row_bytes = hq * pc.D * 2
        self.front = G * self.row_bytes
        self.body = rows * self.row_bytes
        self.t = torch.full((self.front + self.body + self.front,), POISON8, dtype=torch.uint8, device="cuda")
        self.t[self.front:self.front + self.body] = 0xFF
        self.ptr = self.t.data_ptr() + self.front
        assert self.ptr % 16 == 0

    def read(self, what: str) -> torch.Tensor:
        raw = self.t.cpu()
        assert bool((raw[:self.front] == POISON8).all()) and bool((raw[self.front + self.body:] == POISON8).all()), \
            f"{what}: a guard row of O was written"
        return raw[self.front:self.front + self.body].view(torch.bfloat16).reshape(self.rows, self.hq, pc.D)

    def untouched(self) -> bool:
        raw = self.t.cpu()
        body = raw[self.front:self.front + self.body]
        return bool((body == 0xFF).all()) and bool((raw[:self.front] == POISON8).all()) \
            and bool((raw[self.front + self.body:] == POISON8).all())


class Dev:
    """A problem's operands on the device; ``run`` launches into a fresh guarded O and returns it (not synchronised).
    The O keeps its Dev alive: torch's allocator knows nothing of the test's stream and would hand the operands of a
    launch that is still running to the next upload."""

    def __init__(self, p: pc.Problem, tensors=None):
        self.p = p
        self.t = tensors or tuple(t.cuda() for t in (p.q, p.k_cache, p.v_cache, p.block_table, p.seq_lens))
        torch.cuda.synchronize()  # the uploads are torch's: the test's stream does not wait for torch's

    def args(self, s, o: Guarded):
        p = self.p
        q, k, v, bt, sl = self.t
        return (s, p.kind, q.data_ptr(), k.data_ptr(), v.data_ptr(), bt.data_ptr(), sl.data_ptr(), o.ptr, p.b, p.t,
                p.hq, p.hkv, pc.D, p.page, p.num_pages, p.table_stride, p.max_seq_len, p.scale)

    def run(self, hip, s, how: str = "plain") -> Guarded:
        p = self.p
        o = Guarded(p.b * p.t, p.hq)
        o.keep = self  # the launch reads these tensors until the stream is synchronised: they live as long as its O
        torch.cuda.synchronize()
        if how == "plain":
            hip.prefill_attn(*self.args(s, o), p.k_scale, p.v_scale)
        elif how == "cfg":
            hip.prefill_attn_launch_cfg(*self.args(s, o), 0, p.k_scale, p.v_scale)
        else:
            assert how == "timed"
            assert hip.time_prefill_attn(*self.args(s, o), 2, p.k_scale, p.v_scale) > 0.0
        return o


def _run_all(hip, stream, cases, how="plain"):
    """Every problem launched first, read afterwards: ``[(name, problem, O)]``."""
    runs = [(name, p, Dev(p).run(hip, stream, how)) for name, p in cases]
    stream.sync()
    return [(name, p, o.read(name)) for name, p, o in runs]


def _assert_inside(p: pc.Problem, got: torch.Tensor, what: str):
    bound, ref, _ = pc.error_bound(p)
    err = np.abs(got.double().numpy() - ref)
    assert not np.isnan(err).any(), f"{what}: NaN in O"
    over = err > bound
    if over.any():
        n, h, d = (int(x) for x in np.argwhere(over)[0])
        raise AssertionError(f"{what}: {int(over.sum())} of {over.size} elements outside the bound; first at row {n}, "
                             f"head {h}, d {d}: got {float(got[n, h, d])}, reference {ref[n, h, d]}, bound "
                             f"{bound[n, h, d]}")
    print(f"{what}: worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")


def test_the_library_has_the_table_the_cases_use(hip):
    assert {i: (hip.prefill_attn_cfg_name(i), *hip.prefill_attn_cfg_shape(i)) for i in pc.CFGS} == pc.CFGS
    assert hip.prefill_attn_cfg_name(len(pc.CFGS)) is None and hip.prefill_attn_cfg_name(-1) is None
    with pytest.raises(hip.HipError):
        hip.prefill_attn_cfg_shape(len(pc.CFGS))


# ---- 1. staircase: the causal mask, tiles, pages ---------------------------------------------------------------------

@kinds
def test_prefill_staircase_returns_each_rows_own_token(hip, stream, kind):
    """Every T around one and two blocks of query rows from every base around a 16-token run and a tile, pages of 16,
    64 and 256: O is row ``pos`` of V, bit for bit."""
    for name, p, got in _run_all(hip, stream, pc.staircase_cases(kind)):
        ac.assert_bits_equal(got, p.want, f"{kind}, {name}")


@kinds
def test_prefill_dead_rows_clamped_lengths_and_pages(hip, stream, kind):
    """Rows at or past ``max_seq_len`` are zeros; a ``seq_lens`` above ``max_seq_len`` or below 0 is clamped; a wider
    table; a page index at or past ``num_pages`` reads the last page."""
    for name, p, got in _run_all(hip, stream, pc.dead_row_cases(kind)):
        ac.assert_bits_equal(got, p.want, f"{kind}, {name}")
        dead = [b * p.t + t for b, n in enumerate(p.live()) for t in range(n, p.t)]
        assert not ac.bits(got[dead]).any(), f"{kind}, {name}: a row that is not live is not zeros"


# ---- 2. counts and random data, inside the bound ---------------------------------------------------------------------

@kinds
def test_prefill_counts_every_visible_token_once(hip, stream, kind):
    for name, p, got in _run_all(hip, stream, pc.count_cases(kind)):
        _assert_inside(p, got, f"{kind}, count, {name}")


@kinds
def test_prefill_random_against_fp64(hip, stream, kind):
    for name, p, got in _run_all(hip, stream, pc.random_cases(kind)):
        _assert_inside(p, got, f"{kind}, random, {name}")


# ---- 3. T == 1 is the decode attention's problem ---------------------------------------------------------------------

@kinds
def test_prefill_t1_and_decode_attn_share_a_reference(hip, stream, kind):
    """Both lie inside their bounds of the same fp64 reference; the summation orders differ, so they need not be
    equal."""
    ws = torch.full(((16 << 20) // 4,), float("nan"), device="cuda", dtype=torch.float32)
    for name, p in pc.t1_cases(kind):
        d = Dev(p)
        mine = d.run(hip, stream)
        dp = p.as_decode()
        q, k, v, bt, _ = d.t
        lens = dp.seq_lens.cuda()
        other = Guarded(dp.b, dp.hq)
        torch.cuda.synchronize()
        hip.decode_attn(stream, dp.kind, q.data_ptr(), k.data_ptr(), v.data_ptr(), bt.data_ptr(), lens.data_ptr(),
                        other.ptr, dp.b, dp.hq, dp.hkv, pc.D, dp.page, dp.num_pages, dp.table_stride, dp.max_seq_len,
                        dp.scale, dp.k_scale, dp.v_scale, ws.data_ptr(), ws.numel() * 4)
        stream.sync()
        _assert_inside(p, mine.read(name), f"{kind}, prefill T 1, {name}")
        theirs = other.read(name)
        bound, _, _ = ac.error_bound(dp)
        err = np.abs(theirs.double().numpy() - ac.reference(dp))
        assert not (err > bound).any(), f"{kind}, decode, {name}"


# ---- 4. chained with the append ---------------------------------------------------------------------------------------

@kinds
def test_prefill_reads_what_kv_append_has_just_written(hip, stream, kind):
    """``kv_append(T)`` then ``prefill_attn`` on the same ``seq_lens``, one stream, no host sync between them.  The
    caches the append left are the twin's, bit for bit, and O lies inside the bound of the reference computed from
    them."""
    a = pc.chain_append_problem(kind)
    pages = kc.GUARD + a.num_pages + kc.GUARD
    esize = 2 if kind == "bf16" else 1
    page_bytes = a.hkv * a.page * kc.D * esize

    def up(x):
        x = np.ascontiguousarray(x)
        return torch.from_numpy(x.view(np.int16) if x.dtype == np.uint16 else x).cuda()

    qkv, table, lens, cos, sin = (up(x) for x in (a.qkv, a.table, a.seq_lens, a.cos, a.sin))
    q_out = torch.full((a.b * a.t * a.hq * kc.D * 2,), POISON8, dtype=torch.uint8, device="cuda")
    k = torch.full((pages * page_bytes,), POISON8, dtype=torch.uint8, device="cuda")
    v = torch.full((pages * page_bytes,), POISON8, dtype=torch.uint8, device="cuda")
    o = Guarded(a.b * a.t, a.hq)
    kp, vp = k.data_ptr() + kc.GUARD * page_bytes, v.data_ptr() + kc.GUARD * page_bytes
    torch.cuda.synchronize()
    hip.kv_append(stream, kind, qkv.data_ptr(), a.qkv_stride, q_out.data_ptr(), kp, vp, table.data_ptr(),
                  lens.data_ptr(), 0, cos.data_ptr(), sin.data_ptr(), a.rope_len, a.b, a.t, a.hq, a.hkv, kc.D, a.page,
                  a.num_pages, a.table_stride, a.max_seq_len, a.k_inv, a.v_inv)
    hip.prefill_attn(stream, kind, q_out.data_ptr(), kp, vp, table.data_ptr(), lens.data_ptr(), o.ptr, a.b, a.t, a.hq,
                     a.hkv, kc.D, a.page, a.num_pages, a.table_stride, a.max_seq_len, kc.D ** -0.5, 1.0 / a.k_inv,
                     1.0 / a.v_inv)
    stream.sync()
    want = kc.twin(a)
    cdt = np.uint16 if kind == "bf16" else np.uint8
    shape = (pages, a.hkv, a.page, kc.D)
    got_k, got_v = (x.cpu().numpy().view(cdt).reshape(shape) for x in (k, v))
    got_q = q_out.cpu().numpy().view(np.uint16).reshape(a.b * a.t, a.hq, kc.D)
    assert np.array_equal(got_q, want.q_out) and np.array_equal(got_v, want.v)
    assert bool(kc.same_e4m3(got_k, want.k).all()) if kind == "fp8" else np.array_equal(got_k, want.k)
    inner = slice(kc.GUARD, kc.GUARD + a.num_pages)
    p = pc.chained_problem(a, got_q, got_k[inner], got_v[inner])
    _assert_inside(p, o.read("chained"), f"{kind}, chained")


# ---- 5. determinism, batch and prefix independence --------------------------------------------------------------------

@kinds
def test_prefill_is_deterministic_and_a_sequence_alone_gives_the_same_bytes(hip, stream, kind):
    _, p = next((n, q) for n, q in pc.random_cases(kind) if q.b == 3 and q.t > 1)
    d = Dev(p)
    first, second, by_cfg = d.run(hip, stream), d.run(hip, stream), d.run(hip, stream, "cfg")
    singles = []
    for b in range(p.b):  # the same device tensors at the sequence's own addresses
        q, k, v, bt, sl = d.t
        rows = p.t * p.hq * pc.D
        one = Dev(pc.alone(p, b), (q.view(-1)[b * rows:(b + 1) * rows], k, v, bt[b:b + 1], sl[b:b + 1]))
        singles.append(one.run(hip, stream))
    stream.sync()
    a = first.read("first")
    assert torch.equal(ac.bits(a), ac.bits(second.read("second"))), "two launches differ"
    assert torch.equal(ac.bits(a), ac.bits(by_cfg.read("cfg"))), "the table's entry and the dispatcher differ"
    for b, o in enumerate(singles):
        assert torch.equal(ac.bits(o.read(f"alone {b}")), ac.bits(a[b * p.t:(b + 1) * p.t])), \
            f"sequence {b} alone differs from its rows in the batch"


@kinds
def test_prefill_rows_do_not_depend_on_the_chunk_they_came_in(hip, stream, kind):
    """A chunk as T rows, and the same rows as two launches (T1, then T2 from ``base + T1``): equal bytes, with the cut
    inside a wave's rows, at a wave's edge and at a block's edge."""
    _, p = next((n, q) for n, q in pc.random_cases(kind) if q.b == 3 and q.t > pc.Q_ROWS)
    whole = Dev(p).run(hip, stream)
    stream.sync()
    a = whole.read("whole").reshape(p.b, p.t, p.hq, pc.D)
    for t1 in (17, 32, pc.Q_ROWS):
        parts = [Dev(x).run(hip, stream) for x in pc.split_chunk(p, t1)]
        stream.sync()
        got1 = parts[0].read("first part").reshape(p.b, t1, p.hq, pc.D)
        got2 = parts[1].read("second part").reshape(p.b, p.t - t1, p.hq, pc.D)
        assert torch.equal(ac.bits(got1), ac.bits(a[:, :t1])), f"{kind}: rows before the cut at {t1}"
        assert torch.equal(ac.bits(got2), ac.bits(a[:, t1:])), f"{kind}: rows behind the cut at {t1}"


# ---- 6. the timed entry point -----------------------------------------------------------------------------------------

@kinds
def test_timed_prefill_leaves_the_result(hip, stream, kind):
    name, p = pc.dead_row_cases(kind)[0]
    (_, _, got), = _run_all(hip, stream, [(name, p)], "timed")
    ac.assert_bits_equal(got, p.want, f"{kind}, timed, {name}")


# ---- 7. refusals ------------------------------------------------------------------------------------------------------

def _raw_call(hip, s, which: str, a: dict):
    vp = ctypes.c_void_p
    args = [s.handle, a["kind"], *(vp(a[x]) for x in ("Q", "K", "V", "block_table", "seq_lens", "O")), a["B"], a["T"],
            a["Hq"], a["Hkv"], a["D"], a["page"], a["num_pages"], a["table_stride"], a["max_seq_len"], a["scale"],
            a["k_scale"], a["v_scale"]]
    L = hip.lib()
    if which == "plain":
        return L.gsx_prefill_attn(*args)
    if which == "cfg":
        return L.gsx_prefill_attn_launch_cfg(*args, 0)
    ms = ctypes.c_float(-1.0)
    rc = L.gsx_event_time_prefill_attn(*args, 3, ctypes.byref(ms))
    assert ms.value == -1.0
    return rc


def test_prefill_refuses_by_name_and_writes_nothing(hip, stream):
    """Every rule of the contract, through the plain, the timed and the table's entry point.  O is a real guarded
    buffer wherever the rule leaves it alone, and stays as it was; the other addresses are never dereferenced: a
    refusal comes before the first device call."""
    o = Guarded(pc.GOOD["B"] * pc.GOOD["T"], pc.GOOD["Hq"])
    delta = o.ptr - pc.GOOD["O"]
    refused = [(a, why) for a, why in pc.edges() if why is not None]
    assert len(refused) >= 40
    for a, why in refused:
        a = dict(a)
        for x in ("Q", "O"):  # what stands in a fixed relation to GOOD's O moves with it
            if a[x] and abs(a[x] - pc.GOOD["O"]) < (1 << 30):
                a[x] += delta
        for which, who in (("plain", "gsx_prefill_attn"), ("timed", "gsx_prefill_attn"),
                           ("cfg", "gsx_prefill_attn_launch_cfg")):
            assert _raw_call(hip, stream, which, a) != 0, (why, which)
            assert hip.lib().gsx_last_error().decode() == f"{who}: {why}", (why, which)
    stream.sync()
    assert o.untouched()
    vp = ctypes.c_void_p
    assert hip.lib().gsx_prefill_attn_launch_cfg(stream.handle, 0, *(vp(pc.GOOD[x]) for x in
                                                 ("Q", "K", "V", "block_table", "seq_lens", "O")), 2, 3, 8, 2, 128, 16,
                                                 9, 4, 64, 0.1, 1.0, 1.0, 1) != 0
    assert hip.lib().gsx_last_error().decode() == "gsx_prefill_attn_launch_cfg: unknown config"
    for fn in (hip.prefill_attn, hip.time_prefill_attn, hip.prefill_attn_launch_cfg):
        with pytest.raises(ValueError, match="attention cache kind 'fp4'"):
            fn(stream, "fp4", *([0] * 6), 1, 1, 8, 2, 128, 16, 1, 1, 16, 0.1, 1)


# ---- 8. the workload end to end -----------------------------------------------------------------------------------------

@kinds
def test_prefill_workload_end_to_end(kind):
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "gsxtools.workload", "--workload", "prefill", "--batch", "2", "--chunk", "128",
           "--context", "256", "--heads", "8", "--kv-heads", "2", "--weights-gib", "0.05", "--kv-gib", "0.01",
           "--iters", "20", "--json", "--kernel", "gsx", "--kv-dtype", kind]
    r = subprocess.run(cmd, env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["activations_finite"] is True
    assert (out["workload"], out["batch"], out["chunk"], out["context"], out["heads"], out["kv_heads"],
            out["kv_dtype"], out["page"], out["ffn"]) == ("prefill", 2, 128, 256, 8, 2, kind, 16, 3584)
    assert out["iters"] >= 20 and out["layers"] == max(out["weight_layers"], out["kv_layers"]) >= 2
    assert out["tflops"] > 0 and out["tbps"] > 0
    assert out["tokens_per_s"] == pytest.approx(out["iters"] * 2 * 128 / out["seconds"])
    assert out["kernel"] == "gsx" and out["kernels_lib"].endswith("libgsx_kernels.so")
