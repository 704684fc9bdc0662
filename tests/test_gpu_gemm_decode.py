"""The decode GEMM (native/kernels/gemm_decode.hip), bit for bit on a real MI355X.

Operands and references are those of the three GEMM families' case modules, brought to the kernel's shape (M <= 16)
by ``tests/gemm_decode_cases.py``; ``tests/test_gemm_decode_cases.py`` checks that step on the CPU.  Every comparison
is on the raw 16 bits of every element with no tolerance, except the one derived bound of section 6, whose operands
are random.  Every test runs each operand kind on each configuration of the table and on the dispatching entry point
(``None``).
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

torch = pytest.importorskip("torch")

from tests import gemm_cases as gc  # noqa: E402
from tests import gemm_decode_cases as dc  # noqa: E402
from tests import gemm_fp8_cases as gf  # noqa: E402
from tests import gemm_mxfp4_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
ROOT = Path(__file__).resolve().parents[1]
KIND_CFG = [(kind, cfg) for kind in dc.KINDS for cfg in dc.ALL]
kind_cfg = pytest.mark.parametrize("kind,cfg", KIND_CFG,
                                   ids=[f"{k}-{'dispatch' if c is None else c}" for k, c in KIND_CFG])


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    from gpushare_scheduler_extender_amd.ops import hip as h

    assert h.SO.exists()
    assert hasattr(h, "decode_gemm_cfgs"), "the bindings have no decode GEMM"
    assert h.decode_gemm_cfgs() == dc.CFGS
    return h


@pytest.fixture(scope="module")
def stream(hip):
    s = hip.Stream(0)
    yield s
    s.destroy()


class Dev:
    """A problem's operands on the device; ``launch`` runs rows ``r0 .. r0 + m - 1`` of its A into ``c``."""

    def __init__(self, p: dc.Problem, tensors=None):
        self.p = p
        self.a, self.b, self.sa, self.sb = tensors or (None if t is None else t.cuda() for t in (p.a, p.b, p.sa, p.sb))

    def launch(self, hip, s, c, cfg, r0=0, m=None):
        p = self.p
        m = p.m - r0 if m is None else m
        assert 1 <= m <= 16 and r0 + m <= p.m and c.shape == (m, p.n) and c.dtype == torch.bfloat16
        assert c.is_contiguous() and self.a.is_contiguous() and self.b.is_contiguous()
        a = self.a.data_ptr() + r0 * self.a.stride(0) * self.a.element_size()
        sa = sb = 0
        if self.sa is not None:
            sb = self.sb.data_ptr()
            per_row = p.kind == "mxfp4" or p.mode == gf.SCALE_ROW
            sa = self.sa.data_ptr() + (r0 * self.sa.stride(0) * self.sa.element_size() if per_row else 0)
        args = (s, p.kind, a, self.b.data_ptr(), c.data_ptr(), m, p.n, p.k)
        if cfg is None:
            hip.decode_gemm_nt(*args, sa, sb, p.mode)
        else:
            hip.decode_gemm_nt_cfg(*args, cfg, sa, sb, p.mode)


class _Addr:
    """Stands in for a tensor where only its address is used."""

    def __init__(self, addr):
        self.addr = addr

    def data_ptr(self):
        return self.addr


def _nan_c(m, n):
    return torch.full((m, n), NAN, device="cuda", dtype=torch.bfloat16)


def _strips17(cfg) -> int:
    """N of 17 strips of the configuration: odd, more than the 8 XCDs and no multiple of them."""
    return 17 * (16 if cfg is None else dc.CFGS[cfg][1])


def _takes(cfg, n) -> bool:
    return cfg is None or n % dc.CFGS[cfg][1] == 0


def _assert_equal(got, want, what, zeros_by_value=False, zero_cols=(), zero_rows=()):
    """Bit for bit; ``zeros_by_value``: a zero of either sign wherever ``want`` is a zero, or only in the listed
    columns and rows."""
    got = got.cpu()
    if zero_rows:
        got, want, zero_cols = got.t().contiguous(), want.t().contiguous(), tuple(zero_rows)
    if zeros_by_value:
        mc.assert_bits_equal(got, want, what, zeros_by_value=True)
    else:
        gc.assert_bits_equal(got, want, what, zero_by_value_cols=zero_cols)


# ---- 1. the K split, exactly ----------------------------------------------------------------------------------------

MS = (1, 2, 5, 8, 15, 16)
STRIPS = (1, 3, 17)  # one strip, three, and 17: odd, more than the 8 XCDs and no multiple of them
MANY_STRIPS = 16480  # N of 1030 strips of 16 at one K-tile: more workgroups than the chip holds at once


@kind_cfg
def test_decode_k_split_exact(hip, stream, kind, cfg):
    """Every K-tile count that changes what a wave does (``gemm_decode_cases.k_tile_counts``: waves without a tile,
    ragged rounds, the short path, the first counts that reach the steady loop, long loops) at every M of ``MS`` and
    1, 3 and 17 strips (N = 16, 48, 272 for strips of 16 columns), and N = 16480 at one K-tile.  The operands are the
    exact generators' with 16 rows of A; M rows of them are the problem.  C starts as NaN and has exactly M rows."""
    bn = _strips17(cfg) // 17
    shapes = [(bn * strips, nk) for nk in dc.k_tile_counts(cfg, kind) for strips in STRIPS] + [(MANY_STRIPS, 1)]
    for n, nk in shapes:
        assert _takes(cfg, n)
        k = nk * dc.BK[kind]
        p = dc.exact_problem(kind, n, k)
        d = Dev(p)
        cs = [_nan_c(m, n) for m in MS]
        torch.cuda.synchronize()
        for m, c in zip(MS, cs):
            d.launch(hip, stream, c, cfg, 0, m)
        stream.sync()
        for m, c in zip(MS, cs):
            _assert_equal(c, p.want[:m], f"{kind} cfg {cfg} at {m}x{n}x{k} ({nk} K-tiles)")


# ---- 2. every operand code and every k position, on A's path and on B's --------------------------------------------

def _code_cases(kind):
    """``(name, problem, how zeros compare)`` as the families' own GPU tests compare them."""
    if kind == "bf16":
        rc = gc.rounding_case()
        return [("rounding", dc.bf16_problem(rc.a, rc.b, rc.want), {"zero_cols": (rc.zero_col,)})]
    if kind == "fp8":
        a, b, want = gf.code_sweep()
        sweep = dc.Problem("fp8", a, b, want)
        a, b, want = gf.k_slot_case()
        return [("code sweep", sweep, {"zeros_by_value": True}), ("k slots", dc.Problem("fp8", a, b, want), {})]
    return [("code sweep", dc.mxfp4_problem(mc.code_sweep()), {"zeros_by_value": True}),
            ("k slots", dc.mxfp4_problem(mc.k_slot_case()), {}),
            ("scale slots 512", dc.mxfp4_problem(mc.scale_slot_case(512)), {}),
            ("scale slots 1792", dc.mxfp4_problem(mc.scale_slot_case(1792)), {}),
            ("e8m0 sweep", dc.mxfp4_problem(mc.e8m0_sweep()), {})]


def _sliced_product(hip, s, d: Dev, cfg):
    """Every 16-row slice of the problem's A, each into its rows of one C: the whole product."""
    c = _nan_c(d.p.m, d.p.n)
    torch.cuda.synchronize()
    for r0 in range(0, d.p.m, 16):
        d.launch(hip, s, c[r0:r0 + 16], cfg, r0, 16)
    s.sync()
    return c


@kind_cfg
def test_decode_codes_and_k_positions(hip, stream, kind, cfg):
    """The families' cases that tell operand codes, k positions and scale bytes apart (fp8: every e4m3 code, k slots;
    mxfp4: every e2m1 code at every position, k slots, scale slots at two and seven K-tiles, every e8m0 code; bf16:
    the rounding case with its infinities and NaNs).  Each runs as all its 16-row slices, as one ragged slice of 5
    rows, and transposed, again as all 16-row slices: the case's A is then the kernel's B."""
    for name, p, zeros in _code_cases(kind):
        d = Dev(p)
        what = f"{kind} cfg {cfg}, {name}"
        _assert_equal(_sliced_product(hip, stream, d, cfg), p.want, what, **zeros)
        c = _nan_c(5, p.n)
        torch.cuda.synchronize()
        d.launch(hip, stream, c, cfg, 32, 5)
        stream.sync()
        _assert_equal(c, p.want[32:37], what + ", rows 32..36", **zeros)
        t = p.transposed()
        tz = {"zero_rows": zeros["zero_cols"]} if "zero_cols" in zeros else zeros
        _assert_equal(_sliced_product(hip, stream, Dev(t, (d.b, d.a, d.sb, d.sa)), cfg), t.want,
                      what + ", transposed", **tz)


# ---- 3. fp8 scale modes ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", dc.ALL)
@pytest.mark.parametrize("m", [5, 16])
def test_decode_fp8_scale_modes(hip, stream, m, cfg):
    """NONE (the pointers are not looked at), TENSOR and ROW with random 24-bit scales of both signs, 4-B aligned and
    no more: ``bf16((acc * sa[row]) * sb[col])`` with the two multiplies in that order, on 17 strips and five
    K-tiles."""
    n, k = _strips17(cfg), 640
    a, b, acc = gf.exact_case(16, n, k)
    a, acc = a[:m], acc[:m]
    ops = (a.cuda(), b.cuda())
    sa_h, sb_h = gf.row_scales(m, 21), gf.row_scales(n, 23)
    sa, sb = (torch.cat([torch.full((1,), NAN), t]).cuda()[1:] for t in (sa_h, sb_h))
    assert sa.data_ptr() % 8 == 4 and sb.data_ptr() % 8 == 4
    ta, tb = torch.tensor([-(2.0 ** -3)]), torch.tensor([1.5])
    for p, scales in ((dc.fp8_problem(a, b, acc), None),
                      (dc.fp8_problem(a, b, acc, ta, tb, gf.SCALE_TENSOR), (ta.cuda(), tb.cuda())),
                      (dc.fp8_problem(a, b, acc, sa_h, sb_h, gf.SCALE_ROW), (sa, sb))):
        c = _nan_c(m, n)
        torch.cuda.synchronize()
        # mode NONE with made-up addresses: they must not be read
        Dev(p, (*ops, *(scales or (_Addr(4), _Addr(12))))).launch(hip, stream, c, cfg)
        stream.sync()
        _assert_equal(c, p.want, f"fp8 cfg {cfg}, M = {m}, scale mode {p.mode}")


# ---- 4. guard bands and 16-B-only alignment -----------------------------------------------------------------------

def _banded_bytes(t, fill):
    whole, view = mc.banded(dc.as_bytes(t), fill, "cuda")
    return whole, view.view(t.dtype) if t.dtype != torch.uint8 else view


@kind_cfg
def test_decode_guard_bands_and_minimum_alignment(hip, stream, kind, cfg):
    """M = 5 on 17 strips and five K-tiles with every array 16 B past a 32-B boundary between poisoned bands: bf16 NaN
    around A and B, the e4m3 NaN code, 0x77 (two +6.0) around the e2m1 operands, 0xFF around the scales (the e8m0 NaN
    code; an fp32 NaN).  A and scale_a end right after row 4, so a read of row 5 is a read of NaN codes; C's band
    starts right after row 4 and has to stay as it was; nothing else may be written either."""
    m, n, k = 5, _strips17(cfg), 5 * dc.BK[kind]
    p = dc.exact_problem(kind, n, k).rows(0, m)
    if kind == "fp8":
        p = dc.fp8_problem(p.a, p.b, p.acc, gf.row_scales(m, 31), gf.row_scales(n, 33), gf.SCALE_ROW)
    if kind == "bf16":
        (wa, a), (wb, b) = gc.banded(p.a, gc.BF16_QNAN, "cuda"), gc.banded(p.b, gc.BF16_QNAN, "cuda")
    elif kind == "fp8":
        (wa, a), (wb, b) = gf.banded(p.a, "cuda"), gf.banded(p.b, "cuda")
    else:
        (wa, a), (wb, b) = mc.banded(p.a.numpy(), mc.A_BAND, "cuda"), mc.banded(p.b.numpy(), mc.A_BAND, "cuda")
    wholes, sa, sb = [wa, wb], None, None
    if p.sa is not None:
        (wsa, sa), (wsb, sb) = _banded_bytes(p.sa, 0xFF), _banded_bytes(p.sb, 0xFF)
        wholes += [wsa, wsb]
    wc, c = gc.banded(torch.full((m, n), NAN, dtype=torch.bfloat16), gc.C_BAND, "cuda")
    for t in (a, b, c, sa, sb):
        assert t is None or t.data_ptr() % 32 == 16
    before = [w.clone() for w in wholes]
    torch.cuda.synchronize()
    Dev(p, (a, b, sa, sb)).launch(hip, stream, c, cfg)
    stream.sync()
    for band in gc.bands_of(wc, c.numel()):
        changed = (band.to(torch.int32) & 0xFFFF) != gc.C_BAND
        assert not bool(changed.any()), f"{kind} cfg {cfg}: {int(changed.sum())} elements of a band of C were written"
    for w, w0 in zip(wholes, before):
        assert torch.equal(w, w0), f"{kind} cfg {cfg}: an operand, a scale array or a band of theirs was written"
    assert bool(torch.isfinite(p.want.float()).all())
    _assert_equal(c, p.want, f"{kind} cfg {cfg} at {m}x{n}x{k}")


# ---- 5. B past 4 GiB ------------------------------------------------------------------------------------------------

def test_decode_b_past_4_gib(hip, stream):
    """bf16, M = 1, K = 65536: a row of B is 2^17 bytes, so row 32768 starts at byte 2^32 and N = 32800 makes B just
    over 4 GiB.  A strip is 16 whole rows and cannot straddle that offset; compared are the strips on either side of
    it (rows 32752 .. 32767 end at it, rows 32768 .. 32783 begin at it), the first strip and the last.  B is made on
    the device from the formula of ``gemm_cases.exact_operands``; the reference is the CPU's for those rows."""
    m, n, k = 1, 32768 + 32, 65536
    need = n * k * 2 + (1 << 30)
    free, _ = hip.mem_info(0)
    if free < need:
        pytest.skip(f"{free >> 20} MiB free on the device, {need >> 20} MiB needed")
    a_h = gc.exact_operands(m, 16, k)[0]
    b = torch.empty((n, k), dtype=torch.bfloat16, device="cuda")
    for r in range(0, n, 256):
        rows = torch.arange(r, min(n, r + 256), device="cuda", dtype=torch.int64)
        b[r:r + len(rows)] = dc.exact_b_rows(rows, k)
    strips = {"first": 0, "ending at 2^32": 32752, "starting at 2^32": 32768, "last": n - 16}
    assert (32768 * k * 2, b.numel() * 2 > 1 << 32) == (1 << 32, True)
    want = {name: gc.reference(a_h, b[r:r + 16].cpu()) for name, r in strips.items()}
    a, c = a_h.cuda(), _nan_c(m, n)
    d = Dev(dc.bf16_problem(a_h, b, c), (a, b, None, None))
    for cfg in dc.ALL:
        c.fill_(NAN)
        torch.cuda.synchronize()
        d.launch(hip, stream, c, cfg)
        stream.sync()
        assert not bool(torch.isnan(c).any()), f"cfg {cfg}: elements of C were not written, or NaN was computed"
        for name, r in strips.items():
            _assert_equal(c[:, r:r + 16], want[name], f"cfg {cfg}, the strip {name} (rows {r} .. {r + 15} of B)")
    del b, d
    torch.cuda.empty_cache()


# ---- 6. determinism, placement, and the bound for general inputs ---------------------------------------------------

def _random_problem(kind, m, n, k):
    """Random normal operands: ``(problem without a reference, fp64 A, fp64 B)``."""
    g = torch.Generator().manual_seed(20261)
    x, y = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g)
    none = torch.empty(0, dtype=torch.bfloat16)
    if kind == "bf16":
        a, b = x.bfloat16(), y.bfloat16()
        return dc.Problem(kind, a, b, none), a.double(), b.double()
    if kind == "fp8":
        a, b = x.to(gf.FP8), y.to(gf.FP8)
        return dc.Problem(kind, a, b, none), a.double(), b.double()
    ops = []
    for t in (x, y):
        q, s = mc.quant_twin(mc.bf16_bits(t.bfloat16().double().numpy()))
        ops.append((q, s, torch.from_numpy(mc.dequant(mc.unpack(q), s))))
    (qa, sa, a64), (qb, sb, b64) = ops
    return dc.Problem(kind, torch.from_numpy(qa), torch.from_numpy(qb), none, torch.from_numpy(sa),
                      torch.from_numpy(sb)), a64, b64


@kind_cfg
def test_decode_is_deterministic_placement_free_and_within_the_bound(hip, stream, kind, cfg):
    """Random normal operands (mxfp4: quantised by the quantiser's NumPy twin), M = 16, 17 strips, K = 4096.  Two
    runs are bit-equal, a run on a stream masked to CUs 0 .. 63 is bit-equal to them, and every element is within
    ``gemm_decode_cases.error_bound`` of the fp64 product: one rounding to bf16 plus fp32 accumulation in any order."""
    m, n, k = 16, _strips17(cfg), 4096
    p, a64, b64 = _random_problem(kind, m, n, k)
    d = Dev(p)
    masked = hip.Stream(0, hip.mask_words(range(0, 64)))
    out = []
    try:
        assert masked.mask(8)[:2] == [0xFFFFFFFF, 0xFFFFFFFF]
        for s in (stream, stream, masked):
            c = _nan_c(m, n)
            torch.cuda.synchronize()
            d.launch(hip, s, c, cfg)
            s.sync()
            out.append(c.cpu())
    finally:
        masked.destroy()
    assert torch.equal(gc.bits(out[0]), gc.bits(out[1])), f"{kind} cfg {cfg}: two runs differ"
    assert torch.equal(gc.bits(out[0]), gc.bits(out[2])), f"{kind} cfg {cfg}: the masked stream's result differs"
    ref, mag = a64 @ b64.t(), a64.abs() @ b64.abs().t()
    err, bound = (out[0].double() - ref).abs(), dc.error_bound(ref, mag, k)
    worst = float((err / bound).max())
    print(f"{kind} cfg {cfg}: largest error / bound = {worst:.4f}")
    assert bool((err <= bound).all()), f"{kind} cfg {cfg}: error up to {worst:.3f} of the bound"


# ---- 7. the timing entry point ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", dc.KINDS)
def test_time_decode_gemm_leaves_the_product_in_c(hip, stream, kind):
    n, k = 272, 33 * dc.BK[kind]  # the dispatching entry point: strips of 16
    p = dc.exact_problem(kind, n, k).rows(0, 5)
    d = Dev(p)
    c = _nan_c(5, n)
    torch.cuda.synchronize()
    ms = hip.time_decode_gemm(stream, kind, d.a.data_ptr(), d.b.data_ptr(), c.data_ptr(), 5, n, k, 3,
                              0 if d.sa is None else d.sa.data_ptr(), 0 if d.sb is None else d.sb.data_ptr(), p.mode)
    stream.sync()
    assert ms > 0, ms
    _assert_equal(c, p.want, f"time_decode_gemm, {kind}")


# ---- 8. the workload, end to end ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", dc.KINDS)
def test_workload_decode_end_to_end(dtype):
    """``gsxtools.workload --workload decode``: a ring of at least two weight matrices, a positive rate of weight
    bytes, and the library's kernel named as the one that ran."""
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "gsxtools.workload", "--workload", "decode", "--dtype", dtype, "--size",
                        "1024", "--batch", "4", "--weights-gib", "0.25", "--iters", "20", "--json"],
                       env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["workload"] == "decode" and out["batch"] == 4 and out["dtype"] == dtype and out["size"] == 1024
    assert out["layers"] >= 2 and out["tbps"] > 0 and out["tflops"] > 0 and out["iters"] >= 20
    assert out["kernel"] == "gsx" and out["kernels_lib"].endswith("libgsx_kernels.so")
    per_matrix = {"bf16": 2.0, "fp8": 1.0, "mxfp4": 0.5 + 1 / 32}[dtype] * 1024 * 1024
    assert out["layers"] * per_matrix >= 0.25 * (1 << 30)
