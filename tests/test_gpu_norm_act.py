"""Fused residual add + RMSNorm and SwiGLU (native/kernels/norm_act.hip) on a real MI355X.

Problems, the fp64 reference, the bound delta and the checks are those of ``tests/norm_act_cases.py``, which
``tests/test_norm_act_cases.py`` checks on the CPU: a result passes when every element lies in the interval the bound
allows it, ``R_out`` byte for byte.  Every output (``Y``, ``scale_out``, ``R_out``) lies between three guard rows on
either side and has its padding behind every row; all of it is filled with a poison pattern before a launch and
everything outside the rows' own elements is compared with the poison afterwards, so a stray write fails.  No case
holds a size from which a wrong kernel could form an address outside the test's own allocations.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import kv_append_cases as kc  # noqa: E402
from tests import norm_act_cases as nc  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
kinds = pytest.mark.parametrize("kind", nc.KINDS)
G = nc.GUARD_ROWS


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    from gpushare_scheduler_extender_amd.ops import hip as h

    assert h.SO.exists()
    assert hasattr(h, "add_rmsnorm") and hasattr(h, "silu_mul"), "the bindings have no add_rmsnorm / silu_mul"
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


class Guarded:
    """``rows`` rows of ``stride`` elements of ``esize`` bytes between G guard rows on either side (the front guard
    rounded up to 16 B, so that row 0 is 16-B aligned), all poison, or holding ``init`` (bits ``[rows][stride]``) in
    the rows.  ``ptr`` is the address of row 0."""

    def __init__(self, rows: int, stride: int, esize: int, init: np.ndarray | None = None):
        self.rows, self.stride, self.esize = rows, stride, esize
        self.front = -(-G * stride * esize // 16) * 16
        self.body = rows * stride * esize
        self.t = torch.full((self.front + self.body + G * stride * esize,), nc.POISON8, dtype=torch.uint8,
                            device="cuda")
        if init is not None:
            assert init.shape == (rows, stride) and init.itemsize == esize
            self.t[self.front:self.front + self.body] = _up(init).view(torch.uint8).flatten()
        self.ptr = self.t.data_ptr() + self.front
        assert self.ptr % 16 == 0

    def read(self, cols: int, what: str, before: np.ndarray | None = None) -> np.ndarray:
        """The rows' first ``cols`` elements; everything else must be what it was (poison, or ``before``'s padding)."""
        dt = {1: np.uint8, 2: np.uint16, 4: np.uint32}[self.esize]
        raw = self.t.cpu().numpy()
        assert bool((raw[:self.front] == nc.POISON8).all()) and bool((raw[self.front + self.body:] == nc.POISON8).all()), \
            f"{what}: a guard row"
        a = raw[self.front:self.front + self.body].view(dt).reshape(self.rows, self.stride)
        poison = dt(int.from_bytes(bytes([nc.POISON8]) * self.esize, "little"))
        assert bool((a[:, cols:] == (poison if before is None else before[:, cols:])).all()), \
            f"{what}: the padding of a row"
        return a[:, :cols].copy()

    def row_bytes(self, row: int) -> np.ndarray:
        lo = self.front + row * self.stride * self.esize
        return self.t[lo:lo + self.stride * self.esize].cpu().numpy()

    def untouched(self) -> bool:
        return bool((self.t == nc.POISON8).all())


class NormDev:
    def __init__(self, p: nc.NormProblem, kind: str):
        self.p, self.kind = p, kind
        self.x, self.w = _up(p.x), _up(p.w)
        self.r = Guarded(p.m, p.rs, 2, p.r) if p.r is not None else None
        if p.r_out == "inplace":
            self.r_out = self.r
        else:
            self.r_out = Guarded(p.m, p.rs, 2) if p.r_out == "new" else None
        self.y = Guarded(p.m, p.y_stride, 2 if kind == "bf16" else 1)
        self.scale = Guarded(p.m, 1, 4) if kind == "fp8" else None

    def args(self, s, m=None, row=0):
        p = self.p
        return (s, self.kind, self.x.data_ptr() + row * p.x_stride * 2, p.x_stride,
                self.r.ptr + row * p.rs * 2 if self.r else 0, self.r_out.ptr + row * p.rs * 2 if self.r_out else 0,
                p.rs, self.w.data_ptr(), self.y.ptr + row * p.y_stride * self.y.esize, p.y_stride,
                self.scale.ptr + 4 * row if self.scale else 0, p.m if m is None else m, p.h, p.eps)

    def run(self, hip, s):
        torch.cuda.synchronize()  # the uploads and fills are torch's: `s` does not wait for torch's stream
        hip.add_rmsnorm(*self.args(s))
        return self

    def result(self, what: str) -> nc.Result:
        p = self.p
        out = nc.Result(self.y.read(p.h, f"{what}: Y"))
        if self.scale:
            out.scale = self.scale.read(1, f"{what}: scale_out").view(np.float32)[:, 0]
        if self.r_out:
            out.r_out = self.r_out.read(p.h, f"{what}: R_out", p.r if p.r_out == "inplace" else None)
        if self.r and self.r is not self.r_out:
            assert np.array_equal(self.r.read(p.rs, f"{what}: R_in"), p.r), f"{what}: R_in was written"
        return out


class SiluDev:
    def __init__(self, p: nc.SiluProblem, kind: str):
        self.p, self.kind = p, kind
        self.gu = _up(p.gu)
        self.y = Guarded(p.m, p.y_stride, 2 if kind == "bf16" else 1)
        self.scale = Guarded(p.m, 1, 4) if kind == "fp8" else None

    def args(self, s, m=None, row=0):
        p = self.p
        return (s, self.kind, self.gu.data_ptr() + row * p.gu_stride * 2, p.gu_stride,
                self.y.ptr + row * p.y_stride * self.y.esize, p.y_stride,
                self.scale.ptr + 4 * row if self.scale else 0, p.m if m is None else m, p.i)

    def run(self, hip, s):
        torch.cuda.synchronize()
        hip.silu_mul(*self.args(s))
        return self

    def result(self, what: str) -> nc.Result:
        out = nc.Result(self.y.read(self.p.i, f"{what}: Y"))
        if self.scale:
            out.scale = self.scale.read(1, f"{what}: scale_out").view(np.float32)[:, 0]
        return out


def _check_norm(hip, stream, kind, cases):
    """Every case launched first, compared afterwards."""
    runs = [(name, p, NormDev(p, kind).run(hip, stream)) for name, p in cases]
    stream.sync()
    for name, p, d in runs:
        nc.check_norm(p, kind, d.result(f"{kind}, {name}"), f"{kind}, {name}")


def _check_silu(hip, stream, kind, cases):
    runs = [(name, p, SiluDev(p, kind).run(hip, stream)) for name, p in cases]
    stream.sync()
    for name, p, d in runs:
        nc.check_silu(p, kind, d.result(f"{kind}, {name}"), f"{kind}, {name}")


# ---- 1. one-hot rows ---------------------------------------------------------------------------------------------------

@kinds
def test_add_rmsnorm_counts_every_element_once(hip, stream, kind):
    """``norm_act_cases.norm_one_hot``: a single nonzero element per row at a boundary column.  Dropped, the row's sum
    of squares is 0 and the result inf or NaN; counted twice, it is off by sqrt 2."""
    _check_norm(hip, stream, kind, [(f"one-hot H{h}", nc.norm_one_hot(h)) for h in (8, 2040, 2048, 2056, 4104, 16384)])


@kinds
def test_silu_mul_counts_every_element_once(hip, stream, kind):
    """A single nonzero gate per row at a boundary column: it alone is not zero, and in the e4m3 kind it is the row's
    amax, 0x7e or 0xfe."""
    sizes = (8, 2040, 2048, 2056, 4104, 16384) + ((32768,) if kind == "fp8" else ())
    _check_silu(hip, stream, kind, [(f"one-hot I{i}", nc.silu_one_hot(i)) for i in sizes])


# ---- 2. exact cases ----------------------------------------------------------------------------------------------------

@kinds
def test_exact_cases_are_exact(hip, stream, kind):
    """Powers of two whose results are bf16 values and e4m3 codes: equal bytes, whatever delta."""
    p, y, scale = nc.norm_exact(kind)
    dn = NormDev(p, kind).run(hip, stream)
    q, qy, qscale = nc.silu_exact(kind)
    ds = SiluDev(q, kind).run(hip, stream)
    stream.sync()
    for what, got, want, ws in (("norm", dn.result("norm"), y, scale), ("silu", ds.result("silu"), qy, qscale)):
        assert np.array_equal(got.y, want), f"{kind}, {what}: Y"
        if kind == "fp8":
            assert np.array_equal(got.scale, ws), f"{kind}, {what}: scale_out {got.scale} != {ws}"
    assert np.array_equal(dn.result("norm").r_out, nc.norm_h_bits(p))


# ---- 3. random cases ---------------------------------------------------------------------------------------------------

@kinds
def test_add_rmsnorm_random_cases_lie_in_their_intervals(hip, stream, kind):
    """Gaussian rows over H in {8, 2040, 2048, 2056, 4104, 8192, 16384}, M in {1, 3, 17}, strides equal to and larger
    than the row, with and without R_in and R_out and in place; R_out byte for byte."""
    _check_norm(hip, stream, kind, nc.norm_random_cases())


@kinds
def test_silu_mul_random_cases_lie_in_their_intervals(hip, stream, kind):
    _check_silu(hip, stream, kind, nc.silu_random_cases(kind))


def test_silu_mul_more_rows_than_the_grid_has(hip, stream):
    """bf16, 65537 rows of 8: the row loop of the 2-D grid takes a second turn."""
    rng = np.random.default_rng(5)
    p = nc.make_silu(kc.bf16_round((3 * rng.standard_normal((65537, 8))).astype(np.float32)),
                     rng.standard_normal((65537, 8)).astype(np.float32))
    _check_silu(hip, stream, "bf16", [("M65537 I8", p)])


# ---- 4. the residual variants -------------------------------------------------------------------------------------------

@kinds
def test_add_rmsnorm_residual_variants(hip, stream, kind):
    """One problem with R_in NULL, R_out NULL, R_out == R_in and both apart: ``R_out = bf16(x + r)`` byte for byte,
    ``R_in`` unchanged unless it is the output, and without R_in the result is the norm of ``x`` itself."""
    rng = np.random.default_rng(9)
    m, h = 3, 2056
    x = rng.standard_normal((m, h)).astype(np.float32)
    r = (rng.standard_normal((m, h)) * 2.0 ** rng.integers(-6, 4, (m, h))).astype(np.float32)
    w = (1 + 0.25 * rng.standard_normal(h)).astype(np.float32)
    cases = [("apart", nc.make_norm(x, r, w, nc.EPS, r_out="new", pad=8)),
             ("in place", nc.make_norm(x, r, w, nc.EPS, r_out="inplace", pad=8)),
             ("R_out NULL", nc.make_norm(x, r, w, nc.EPS, r_out=None, pad=8)),
             ("R_in NULL", nc.make_norm(x, None, w, nc.EPS, r_out="new", pad=8)),
             ("both NULL", nc.make_norm(x, None, w, nc.EPS, r_out=None))]
    runs = [(name, p, NormDev(p, kind).run(hip, stream)) for name, p in cases]
    stream.sync()
    got = {}
    for name, p, d in runs:
        got[name] = d.result(f"{kind}, {name}")
        nc.check_norm(p, kind, got[name], f"{kind}, {name}")
    for name in ("in place", "R_out NULL"):
        assert np.array_equal(got[name].y, got["apart"].y), name
    assert np.array_equal(got["in place"].r_out, got["apart"].r_out)
    assert np.array_equal(got["R_in NULL"].r_out, cases[3][1].x[:, :h])  # a raw copy
    assert np.array_equal(got["R_in NULL"].y, got["both NULL"].y)


# ---- 5. determinism ----------------------------------------------------------------------------------------------------

@kinds
def test_results_do_not_depend_on_the_launch_or_the_batch(hip, stream, kind):
    """Two launches give equal bytes, and a row run alone (M = 1 at the row's addresses) the bytes it has in the
    batch."""
    _, pn = nc.norm_random_cases()[7]  # M 17, H 16384
    _, ps = nc.silu_random_cases(kind)[6]  # M 17, I 16384
    for p, dev in ((pn, NormDev), (ps, SiluDev)):
        a, b, c = dev(p, kind), dev(p, kind), dev(p, kind)
        call = hip.add_rmsnorm if dev is NormDev else hip.silu_mul
        torch.cuda.synchronize()
        call(*a.args(stream))
        call(*b.args(stream))
        rows = (0, 2, 16)  # rows of e4m3 that start 16-B aligned whatever the padding
        for row in rows:
            call(*c.args(stream, m=1, row=row))
        stream.sync()
        ra, rb = a.result("first"), b.result("second")
        assert np.array_equal(ra.y, rb.y)
        for row in rows:
            assert np.array_equal(c.y.row_bytes(row), a.y.row_bytes(row)), f"row {row} alone"
        if kind == "fp8":
            assert np.array_equal(ra.scale, rb.scale)
            assert all(np.array_equal(c.scale.row_bytes(row), a.scale.row_bytes(row)) for row in rows)
        if dev is NormDev:
            assert np.array_equal(ra.r_out, rb.r_out)


# ---- 6. refusals write nothing ------------------------------------------------------------------------------------------

@kinds
def test_refused_calls_write_nothing(hip, stream, kind):
    """Every rule of ``tests/test_norm_act_cases.py`` again on real buffers: refused by name, and the outputs stay
    poison.  (The rules' edges are checked there, on the CPU.)"""
    _, p = nc.norm_random_cases()[3]  # M 3, H 2056, strides with padding, R_in NULL, R_out new
    d = NormDev(p, kind)
    good = list(d.args(stream))
    torch.cuda.synchronize()
    y_ptr, x_ptr = good[8], good[2]
    bad = [({1: "fp4"}, None), ({11: 0}, "need M >= 1"), ({12: 2052}, "need 8 <= H <= 16384 and H % 8 == 0"),
           ({12: 16392}, "need 8 <= H <= 16384"), ({3: 2048}, "need x_stride >= H"), ({6: 2052}, "need r_stride >= H"),
           ({9: 2050}, "need y_stride >= H"), ({2: 0}, "X, W and Y must not be NULL"), ({7: 0}, "X, W and Y must not"),
           ({8: 0}, "X, W and Y must not"), ({8: y_ptr + 8}, "X, R_in, R_out, W and Y must be 16-B aligned"),
           ({10: 0 if kind == "fp8" else y_ptr}, "scale_out must be NULL with GSX_ACT_OUT_BF16"),
           ({13: -1.0}, "eps must be finite and >= 0"), ({13: float("nan")}, "eps must be finite"),
           ({8: x_ptr}, "Y must not overlap X, R_in or W"), ({5: x_ptr}, "R_out must not overlap X, W, Y or scale_out"),
           ({5: y_ptr}, "R_out must not overlap")]
    for change, text in bad:
        a = list(good)
        for k, v in change.items():
            a[k] = v
        for fn, tail in ((hip.add_rmsnorm, ()), (hip.time_add_rmsnorm, (2,))):
            if text is None:
                with pytest.raises(ValueError, match="output kind 'fp4'"):
                    fn(*a, *tail)
            else:
                with pytest.raises(hip.HipError, match=f"gsx_add_rmsnorm: {text}"):
                    fn(*a, *tail)
    stream.sync()
    assert d.y.untouched() and d.r_out.untouched() and (d.scale is None or d.scale.untouched())

    _, q = nc.silu_random_cases(kind)[3]  # M 3, I 2056, padded
    e = SiluDev(q, kind)
    good = list(e.args(stream))
    torch.cuda.synchronize()
    y_ptr, gu_ptr = good[4], good[2]
    bad = [({7: 0}, "need M >= 1"), ({8: 2052}, "need I >= 8 and I % 8 == 0"), ({3: 4104}, "need gu_stride >= 2 I"),
           ({5: 2048}, "need y_stride >= I"), ({2: 0}, "GU and Y must not be NULL"), ({4: 0}, "GU and Y must not"),
           ({2: gu_ptr + 8}, "GU and Y must be 16-B aligned"),
           ({6: 0 if kind == "fp8" else y_ptr}, "scale_out must be NULL with GSX_ACT_OUT_BF16"),
           ({4: gu_ptr + 4096}, "Y must not overlap GU")]
    if kind == "fp8":
        bad += [({8: 32776, 3: 65552, 5: 32776}, "need I <= 32768 with GSX_ACT_OUT_FP8_ROW"),
                ({6: y_ptr}, "scale_out must not overlap GU or Y")]
    for change, text in bad:
        a = list(good)
        for k, v in change.items():
            a[k] = v
        for fn, tail in ((hip.silu_mul, ()), (hip.time_silu_mul, (2,))):
            with pytest.raises(hip.HipError, match=f"gsx_silu_mul: {text}"):
                fn(*a, *tail)
    stream.sync()
    assert e.y.untouched() and (e.scale is None or e.scale.untouched())


@kinds
def test_timed_entry_points_leave_the_result(hip, stream, kind):
    _, p = nc.norm_random_cases()[4]
    d = NormDev(p, kind)
    _, q = nc.silu_random_cases(kind)[5]
    e = SiluDev(q, kind)
    torch.cuda.synchronize()
    ms = [hip.time_add_rmsnorm(*d.args(stream), 3), hip.time_silu_mul(*e.args(stream), 3)]
    stream.sync()
    assert min(ms) > 0, ms
    nc.check_norm(p, kind, d.result("timed norm"), f"time_add_rmsnorm, {kind}")
    nc.check_silu(q, kind, e.result("timed silu"), f"time_silu_mul, {kind}")


# ---- 7. chained with the fp8 decode GEMM --------------------------------------------------------------------------------

def test_fp8_norm_output_feeds_the_decode_gemm(hip, stream):
    """An e4m3 norm output and its ``scale_out`` as ``A`` and ``scale_a`` of ``decode_gemm_nt("fp8", .., SCALE_ROW)`` at
    3 x 48 x 256, back to back on one stream.  The reference is rebuilt from the codes and scales read back."""
    rng = np.random.default_rng(11)
    m, n, k = 3, 48, 256
    x = rng.standard_normal((m, k)).astype(np.float32) * np.array([[1.0], [64.0], [2.0 ** -6]], np.float32)
    r = rng.standard_normal((m, k)).astype(np.float32)
    p = nc.make_norm(x, r, (1 + 0.25 * rng.standard_normal(k)).astype(np.float32), nc.EPS, r_out="inplace")
    d = NormDev(p, "fp8")
    wq = kc.e4m3_encode(rng.standard_normal((n, k)).astype(np.float32))
    sb = rng.uniform(0.05, 0.15, n).astype(np.float32)
    wq_d, sb_d = _up(wq), _up(sb)
    c = Guarded(m, n, 2)
    torch.cuda.synchronize()
    hip.add_rmsnorm(*d.args(stream))
    hip.decode_gemm_nt(stream, "fp8", d.y.ptr, wq_d.data_ptr(), c.ptr, m, n, k, d.scale.ptr, sb_d.data_ptr(),
                       hip.SCALE_ROW)
    stream.sync()
    got = d.result("chain")
    nc.check_norm(p, "fp8", got, "chain: the norm")
    ref = (nc.e4m3_value(got.y) @ nc.e4m3_value(wq).T) * got.scale.astype(np.float64)[:, None] * sb[None]
    out = kc.bf16_value(c.read(n, "chain: C")).astype(np.float64)
    assert bool(np.isfinite(out).all()) and float(np.abs(ref).max()) > 1
    assert bool((np.abs(out - ref) <= 1e-2 + 2.0 ** -7 * np.abs(ref)).all()), float(np.abs(out - ref).max())
    # and it is the normalised activations times the weights, to what e4m3 keeps of them
    full = nc.norm_reference(p) @ (nc.e4m3_value(wq) * sb[:, None]).T
    assert float(np.abs(out - full).max()) <= 0.08 * float(np.abs(full).max())


# ---- 8. the workload, end to end ---------------------------------------------------------------------------------------

@kinds
def test_workload_layer_end_to_end(kind):
    """``gsxtools.workload --workload layer``: more steps than the window, so the lengths start again once."""
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "gsxtools.workload", "--workload", "layer", "--kv-dtype", kind,
                        "--batch", "4", "--context", "512", "--heads", "8", "--kv-heads", "2", "--kv-gib", "0.01",
                        "--weights-gib", "0.05", "--iters", "70", "--json"],
                       env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["workload"] == "layer" and out["batch"] == 4 and out["kv_dtype"] == kind and out["context"] == 512
    assert (out["heads"], out["kv_heads"], out["page"], out["window"], out["ffn"]) == (8, 2, 16, 64, 3584)
    assert out["weight_layers"] >= 2 and out["kv_layers"] >= 2 and out["layers"] == max(out["weight_layers"],
                                                                                       out["kv_layers"])
    assert out["tbps"] > 0 and out["tokens_per_s"] > 0 and out["iters"] >= 70
    assert out["activations_finite"] is True
    assert out["kernel"] == "gsx" and out["kernels_lib"].endswith("libgsx_kernels.so")
