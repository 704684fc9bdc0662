"""The MoE decode kernels (native/kernels/moe.hip, the grouped form of gemm_decode.hip) on a real MI355X.

The router's ids and plan, the grouped GEMM on the exact generators' operands and the combine are compared bit for
bit with the twins of ``tests/moe_cases.py`` (``tests/test_moe_cases.py`` checks those on the CPU); the router's
weights with the bound derived in ``gsx_kernels.h``.  Every output sits between guard bands that have to survive.
"""
import dataclasses
import functools
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import gemm_cases as gc  # noqa: E402
from tests import gemm_decode_cases as dc  # noqa: E402
from tests import gemm_fp8_cases as gf  # noqa: E402
from tests import gemm_mxfp4_cases as mx  # noqa: E402
from tests import moe_cases as mo  # noqa: E402
from tests import norm_act_cases as nc  # noqa: E402
from tests import sample_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
FILL = 0xA5
LEAD = gc.BAND + 16
KIND_CFG = [(kind, cfg) for kind in dc.KINDS for cfg in mo.ALL]
kind_cfg = pytest.mark.parametrize("kind,cfg", KIND_CFG,
                                   ids=[f"{k}-{'dispatch' if c is None else c}" for k, c in KIND_CFG])


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    from gpushare_scheduler_extender_amd.ops import hip as h

    assert h.SO.exists()
    assert hasattr(h, "moe_route") and hasattr(h, "moe_gemm_nt") and hasattr(h, "moe_combine"), \
        "the bindings have no MoE entry points"
    assert h.moe_gemm_cfgs() == mo.CFGS
    return h


@pytest.fixture(scope="module")
def stream(hip):
    s = hip.Stream(0)
    yield s
    s.destroy()


class Banded:
    """``payload`` (any NumPy array) on the device between two bands of ``FILL`` bytes, 16-B aligned and no more."""

    def __init__(self, payload: np.ndarray):
        self.shape, self.dtype = payload.shape, payload.dtype
        self.whole, self.view = mx.banded(np.ascontiguousarray(payload).view(np.uint8).reshape(-1), FILL, "cuda")

    def ptr(self) -> int:
        return self.view.data_ptr()

    def get(self) -> np.ndarray:
        return self.view.cpu().numpy().view(self.dtype).reshape(self.shape)

    def assert_bands(self, what: str):
        n = self.view.numel()
        for band in (self.whole[:LEAD], self.whole[LEAD + n:]):
            assert bool((band == FILL).all()), f"{what}: a guard band was written"


# ---- 1. the router -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _route_groups():
    return {"grid": mo.grid_cases(), "equal and two-valued": mo.equal_and_two_valued_cases(),
            "shared and distinct": mo.shared_and_distinct_cases(), "special values": mo.special_value_cases()}


def _run_route(hip, stream, c: mo.RouteCase, timed=False):
    logits = np.full((c.m, c.e + c.pad), mo.NAN, np.uint16)
    logits[:, :c.e] = c.bits
    lg = Banded(logits)
    ids = Banded(np.full((c.m, c.topk), -7, np.int32))
    w = Banded(np.full((c.m, c.topk), np.nan, np.float32))
    plan = Banded(np.full(mo.PLAN_INTS, -7, np.int32))
    torch.cuda.synchronize()
    args = (stream, lg.ptr(), c.e + c.pad, ids.ptr(), w.ptr(), plan.ptr(), c.m, c.e, c.topk)
    if timed:
        assert hip.time_moe_route(*args, 3) > 0
    else:
        hip.moe_route(*args)
    return lg, ids, w, plan, logits


def _check_route(c: mo.RouteCase, run):
    lg, ids, w, plan, logits = run
    want_ids, w64, want_plan = mo.route(c.bits, c.topk)
    for name, b in (("logits", lg), ("ids", ids), ("weights", w), ("plan", plan)):
        b.assert_bands(f"{c.name}: {name}")
    assert np.array_equal(lg.get(), logits), f"{c.name}: the logits were written"
    got_ids, got_w, got_plan = ids.get(), w.get().astype(np.float64), plan.get()
    assert got_ids.min() >= 0 and got_ids.max() < c.e, f"{c.name}: an id outside [0, E)"
    assert np.array_equal(got_ids, want_ids), f"{c.name}: ids {got_ids.tolist()} != {want_ids.tolist()}"
    assert np.array_equal(got_plan, want_plan), f"{c.name}: the plan differs at {np.flatnonzero(got_plan != want_plan)[:8]}"
    bound = mo.weight_bound(c.bits, want_ids, w64)
    err = np.abs(got_w - w64)
    assert not np.isnan(got_w).any() and (err <= bound).all(), \
        f"{c.name}: a weight is off by {err.max()!r}, up to {np.max(err / np.maximum(bound, 1e-300)):.3f} of its bound"
    exact = bound == 0
    assert np.array_equal(got_w[exact], w64[exact]), f"{c.name}: a weight that is exactly 0 or 1 is not"


@pytest.mark.parametrize("group", ["grid", "equal and two-valued", "shared and distinct", "special values"])
def test_route_ids_plan_and_weights(hip, stream, group):
    """Every case of ``moe_cases.route_cases``: ids and the 516-int plan equal the twin's, the weights lie within the
    header's bound of the fp64 softmax and are exactly 0 or 1 where the contract says so, the padding of the logits
    holds NaN, and every array sits between guard bands."""
    cases = _route_groups()[group]
    runs = [_run_route(hip, stream, c) for c in cases]
    stream.sync()
    for c, run in zip(cases, runs):
        _check_route(c, run)


def test_time_moe_route_leaves_the_result(hip, stream):
    c = mo.grid_cases()[-1]
    run = _run_route(hip, stream, c, timed=True)
    stream.sync()
    _check_route(c, run)


# ---- 2. the grouped GEMM, exactly ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=8)
def _base(kind: str, rows: int, k: int) -> dc.Problem:
    return dc.exact_problem(kind, rows, k)


class GroupedDev:
    """A base problem's B and scales on the device, once; ``launch`` runs one routing of it into a banded C of NaN."""

    def __init__(self, kind: str, e: int, n: int, k: int, spare_experts: int = 0):
        self.kind, self.e, self.n, self.k = kind, e, n, k
        self.base = _base(kind, (e + spare_experts) * n, k)
        self.b = self.base.b.cuda()
        self.sb = None if self.base.sb is None else self.base.sb.cuda()
        self.sb_row = gf.row_scales((e + spare_experts) * n, 43).cuda() if kind == "fp8" else None

    def problem(self, ids, a_div, fp8_row=False) -> mo.Grouped:
        g = mo.grouped_problem(self.kind, ids, self.e, self.n, self.k, a_div, fp8_row,
                               base=_base(self.kind, self.e * self.n, self.k))
        return g

    def launch(self, hip, s, g: mo.Grouped, cfg, plan=None, c_rows=None, b=None, sb=None, timed=False):
        pairs = g.m * g.topk
        c = Banded(np.full((c_rows or pairs, g.n), mo.NAN, np.uint16))
        a = g.a.cuda()
        sa = None if g.sa is None else g.sa.cuda()
        sb = sb if sb is not None else self.sb_row if g.mode == gf.SCALE_ROW else self.sb
        plan_d = torch.from_numpy(np.ascontiguousarray(g.plan if plan is None else plan)).cuda()
        torch.cuda.synchronize()
        args = (s, g.kind, a.data_ptr(), g.a_div, (self.b if b is None else b).data_ptr(), c.ptr(), plan_d.data_ptr(),
                g.m, g.topk, g.e, g.n, g.k)
        sc_ = (0 if sa is None else sa.data_ptr(), 0 if sa is None else sb.data_ptr(), g.mode)
        if timed:
            assert hip.time_moe_gemm(*args, 3, *sc_) > 0
        elif cfg is None:
            hip.moe_gemm_nt(*args, *sc_)
        else:
            hip.moe_gemm_nt_cfg(*args, cfg, *sc_)
        c.keep = (a, sa, plan_d)
        return c


def _want_bits(g: mo.Grouped, rows=None) -> np.ndarray:
    want = gc.bits(g.want).numpy().astype(np.uint16)
    if rows is None:
        return want
    out = np.full((rows, g.n), mo.NAN, np.uint16)
    out[:len(want)] = want
    return out


def _assert_c(c: Banded, want: np.ndarray, what: str):
    c.assert_bands(what)
    got = c.get()
    bad = np.argwhere(got != want)
    assert not len(bad), (f"{what}: {len(bad)} of {got.size} elements differ, first at {bad[0].tolist()}: got "
                          f"{int(got[tuple(bad[0])]):#06x}, want {int(want[tuple(bad[0])]):#06x}")


def _ns(cfg) -> tuple:
    return (32, 64, 96) if cfg == 3 else (16, 48, 96)


@kind_cfg
def test_moe_gemm_exact(hip, stream, kind, cfg):
    """E = 8: every N of one, three and six strips (32, 64, 96 for the 32-column row), every K-tile count of
    ``moe_cases.nk_counts``, every routing of ``moe_cases.routings`` and both ``a_div``; fp8 with scales per row on
    every other routing.  E = 256 at the smallest N and W + 1 K-tiles.  C starts as NaN between guard bands: the P
    rows are the CPU reference's bits (which are finite, so every row was written) and nothing else was touched."""
    shapes = [(8, n, nk) for n in _ns(cfg) for nk in mo.nk_counts(cfg, kind)]
    shapes.append((256, _ns(cfg)[0], (16 if cfg is None else mo.CFGS[cfg][2]) + 1))
    for e, n, nk in shapes:
        d = GroupedDev(kind, e, n, nk * dc.BK[kind])
        runs = []
        for i, (name, ids) in enumerate(mo.routings(e)):
            for a_div in (ids.shape[1], 1):
                g = d.problem(ids, a_div, fp8_row=kind == "fp8" and i % 2 == 1)
                runs.append((f"{kind} cfg {cfg}, E={e} N={n} {nk} K-tiles, {name}, a_div={a_div}", g,
                             d.launch(hip, stream, g, cfg)))
        stream.sync()
        for what, g, c in runs:
            assert bool(torch.isfinite(g.want.float()).all())
            _assert_c(c, _want_bits(g), what)


@pytest.mark.parametrize("kind", dc.KINDS)
def test_time_moe_gemm_leaves_the_product_in_c(hip, stream, kind):
    d = GroupedDev(kind, 8, 48, 9 * dc.BK[kind])
    g = d.problem(mo.routings(8)[-1][1], 1)
    c = d.launch(hip, stream, g, None, timed=True)
    stream.sync()
    _assert_c(c, _want_bits(g), f"time_moe_gemm, {kind}")


# ---- 3. random operands: the plain kernel is the yardstick ---------------------------------------------------------

def _random_operands(kind, rows, k, seed):
    """``(operand, scales or None)`` on the device: random normal bf16 / e4m3, or random e2m1 codes with e8m0 codes
    around 127."""
    g = torch.Generator().manual_seed(seed)
    if kind == "mxfp4":
        q = torch.randint(0, 256, (rows, k // 2), generator=g, dtype=torch.uint8)
        s = torch.randint(120, 135, (rows, k // 32), generator=g, dtype=torch.uint8)
        return q.cuda(), s.cuda()
    x = torch.randn(rows, k, generator=g)
    return (x.bfloat16() if kind == "bf16" else x.to(gf.FP8)).cuda(), None


@kind_cfg
def test_moe_gemm_random_operands_match_the_plain_kernel(hip, stream, kind, cfg):
    """Random operands are not order-independent, so for each active expert the plain kernel runs that expert's rows,
    gathered contiguously in plan order, on the decode configuration the grouped one names (the dispatching entry
    points against each other): the same bits.  Both ``a_div``; fp8 with a scale per row and per (expert, column)."""
    e, n, k = 8, 96, 40 * dc.BK[kind]
    b, sb = _random_operands(kind, e * n, k, 1)
    for a_div_is_topk in (True, False):
        ids = mo.routings(e)[-1][1]  # random, M = 11, topk = 8
        m, topk = ids.shape
        a_div = topk if a_div_is_topk else 1
        pairs, a_rows = m * topk, -(-m * topk // a_div)
        a, sa = _random_operands(kind, a_rows, k, 2)
        mode = gf.SCALE_NONE
        if kind == "fp8":
            sa, sb, mode = gf.row_scales(a_rows, 5).cuda(), gf.row_scales(e * n, 7).cuda(), gf.SCALE_ROW
        plan = mo.plan_of(ids, e)
        plan_d = torch.from_numpy(plan).cuda()
        c = torch.full((pairs, n), float("nan"), device="cuda", dtype=torch.bfloat16)
        torch.cuda.synchronize()
        args = (stream, kind, a.data_ptr(), a_div, b.data_ptr(), c.data_ptr(), plan_d.data_ptr(), m, topk, e, n, k)
        scales = (0 if sa is None else sa.data_ptr(), 0 if sb is None else sb.data_ptr(), mode)
        if cfg is None:
            hip.moe_gemm_nt(*args, *scales)
        else:
            hip.moe_gemm_nt_cfg(*args, cfg, *scales)
        n_active, _, _, expert, begin, count, rows = mo.plan_fields(plan)
        plain = []
        for s in range(n_active):
            x, prs = int(expert[s]), rows[begin[s]:begin[s] + count[s]]
            src = torch.from_numpy(prs // a_div).cuda()
            ga = a[src].contiguous()
            gsa = None if sa is None else sa[src].contiguous()
            cs = torch.full((len(prs), n), float("nan"), device="cuda", dtype=torch.bfloat16)
            xb = b[x * n:(x + 1) * n]
            xsb = None if sb is None else sb[x * n:(x + 1) * n]
            torch.cuda.synchronize()
            pargs = (stream, kind, ga.data_ptr(), xb.data_ptr(), cs.data_ptr(), len(prs), n, k)
            pscales = (0 if gsa is None else gsa.data_ptr(), 0 if xsb is None else xsb.data_ptr(), mode)
            if cfg is None:
                hip.decode_gemm_nt(*pargs, *pscales)
            else:
                hip.decode_gemm_nt_cfg(*pargs, mo.CFGS[cfg][4], *pscales)
            plain.append((prs, cs, (ga, gsa)))
        stream.sync()
        got = gc.bits(c.cpu())
        for prs, cs, _ in plain:
            assert torch.equal(got[torch.from_numpy(prs.astype(np.int64))], gc.bits(cs.cpu())), \
                f"{kind} cfg {cfg}, a_div={a_div}: pairs {prs.tolist()} differ from the plain kernel's rows"
        assert not bool(torch.isnan(c).any()), f"{kind} cfg {cfg}: rows of C were not written"


# ---- 4. inactive experts are not read ------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", dc.KINDS)
def test_moe_gemm_never_reads_inactive_experts(hip, stream, kind):
    """Every inactive expert's matrix and scales hold NaN codes (bf16 0x7FC0, e4m3 0x7F, e8m0 0xFF, fp32 NaN): the
    result is the exact one, on every configuration and the dispatching entry point."""
    e, n, k = 8, 96, 9 * dc.BK[kind]
    d = GroupedDev(kind, e, n, k)
    ids = np.array([[1, 6], [6, 3], [1, 3]], np.int32)
    g = d.problem(ids, 2, fp8_row=kind == "fp8")
    dead = torch.ones(e, dtype=torch.bool)
    dead[[1, 3, 6]] = False
    dead_rows = dead.repeat_interleave(n).cuda()
    b = d.b.clone()
    code = {"bf16": 0x7FC0, "fp8": 0x7F, "mxfp4": 0x77}[kind]
    (b.view(torch.int16) if kind == "bf16" else b.view(torch.uint8))[dead_rows] = code
    sb = None
    if kind == "fp8":
        sb = d.sb_row.clone()
        sb[dead_rows] = float("nan")
    elif kind == "mxfp4":
        sb = d.sb.clone()
        sb[dead_rows] = 0xFF
    runs = [(cfg, d.launch(hip, stream, g, cfg, b=b, sb=sb)) for cfg in mo.ALL if cfg != 3 or n % 32 == 0]
    stream.sync()
    for cfg, c in runs:
        _assert_c(c, _want_bits(g), f"{kind} cfg {cfg}, NaN in the inactive experts")


# ---- 5. B past 4 GiB -------------------------------------------------------------------------------------------------

def test_moe_gemm_b_past_4_gib(hip, stream):
    """bf16, N = 64, K = 65536: an expert is 8 MiB and 520 experts are just over 4 GiB.  B is allocated uninitialised;
    expert 0 and the last are written, from the formula of ``gemm_cases.exact_operands``, and routed to.  The last
    expert's rows (and the first's) are the CPU reference's."""
    e, n, k = 520, 64, 65536
    need = e * n * k * 2 + (1 << 30)
    free, _ = hip.mem_info(0)
    if free < need:
        pytest.skip(f"{free >> 20} MiB free on the device, {need >> 20} MiB needed")
    assert e * n * k * 2 > 1 << 32
    b = torch.empty((e * n, k), dtype=torch.bfloat16, device="cuda")
    for x in (0, e - 1):
        rows = torch.arange(x * n, (x + 1) * n, device="cuda", dtype=torch.int64)
        b[x * n:(x + 1) * n] = dc.exact_b_rows(rows, k)
    ids = np.array([[0, e - 1], [e - 1, 0], [e - 1, 0]], np.int32)
    a_h = gc.exact_operands(3, 16, k)[0]
    a = a_h.cuda()
    want = torch.empty(6, n, dtype=torch.bfloat16)
    for p, x in enumerate(ids.reshape(-1)):
        want[p] = gc.reference(a_h[p // 2:p // 2 + 1], b[int(x) * n:(int(x) + 1) * n].cpu())[0]
    plan_d = torch.from_numpy(mo.plan_of(ids, e)).cuda()
    for cfg in mo.ALL:
        c = torch.full((6, n), float("nan"), device="cuda", dtype=torch.bfloat16)
        torch.cuda.synchronize()
        args = (stream, "bf16", a.data_ptr(), 2, b.data_ptr(), c.data_ptr(), plan_d.data_ptr(), 3, 2, e, n, k)
        hip.moe_gemm_nt(*args) if cfg is None else hip.moe_gemm_nt_cfg(*args, cfg)
        stream.sync()
        gc.assert_bits_equal(c, want, f"cfg {cfg}, experts 0 and {e - 1} of a B of {e * n * k * 2 >> 20} MiB")
    del b
    torch.cuda.empty_cache()


# ---- 6. hand-written plans -------------------------------------------------------------------------------------------

def _bad_plans(ids, e):
    """``(name, plan, pairs that must still be written: {pair: expert})``.  The routing has three slots."""
    good = mo.plan_of(ids, e)
    flat = ids.reshape(-1)
    p = len(flat)
    n_active, _, _, expert, begin, count, rows = mo.plan_fields(good)
    keep_all = {q: int(flat[q]) for q in range(p)}
    S = mo.MAX_PAIRS
    out = []

    def variant(name, edit, keep):
        plan = good.copy()
        edit(plan)
        out.append((name, plan, keep))

    def without_slot(s):
        gone = set(rows[begin[s]:begin[s] + count[s]].tolist())
        return {q: x for q, x in keep_all.items() if q not in gone}

    variant("expert -1", lambda pl: pl.__setitem__(4 + 0, -1), without_slot(0))
    variant("expert E", lambda pl: pl.__setitem__(4 + 1, e), without_slot(1))
    variant("expert E + 100", lambda pl: pl.__setitem__(4 + 1, e + 100), without_slot(1))
    # the last slot's: clamped to 16, and the rows behind its run are unused (-1), so nothing more is written
    variant("count 17", lambda pl: pl.__setitem__(4 + 2 * S + 2, 17), keep_all)
    variant("count -1", lambda pl: pl.__setitem__(4 + 2 * S + 2, -1), without_slot(2))
    variant("n_active 129", lambda pl: pl.__setitem__(0, 129), keep_all)
    variant("n_active 0", lambda pl: pl.__setitem__(0, 0), {})

    def far_begin(pl):  # slot 1 begins at 127 with count 4: rows[127] is one of its pairs, 128 .. 130 are outside
        pl[4 + S + 1], pl[4 + 2 * S + 1] = 127, 4
        pl[4 + 3 * S + 127] = rows[begin[1]]
    keep = without_slot(1)
    keep[int(rows[begin[1]])] = int(expert[1])
    variant("begin 127, count 4", far_begin, keep)
    variant("begin -3", lambda pl: pl.__setitem__(4 + S + 0, -3),
            {**without_slot(0), **{int(rows[r - 3]): int(expert[0]) for r in range(3, int(count[0]))
                                   if int(flat[rows[r - 3]]) == int(expert[0])}})
    first = int(rows[begin[0]])

    def pair(v):
        return lambda pl: pl.__setitem__(4 + 3 * S + int(begin[0]), v)
    for v in (p, p + 5, -1, 1 << 30, -(1 << 31)):
        variant(f"pair {v}", pair(v), {q: x for q, x in keep_all.items() if q != first})
    return out


@pytest.mark.parametrize("kind", dc.KINDS)
def test_moe_gemm_survives_hand_written_plans(hip, stream, kind):
    """Plans that break each safety rule.  C has P spare rows behind its P rows and guard bands around, B and scale_b
    one spare expert, and the plan sits in front of 16 ints that look like pairs: a kernel that ignored a rule would
    land in memory this test owns and fail an assertion here.  Exactly the pairs that remain valid are written, with
    their expert's product; every other row of C stays NaN."""
    e, n, k = 8, 48, 9 * dc.BK[kind]
    ids = np.array([[2, 5], [5, 7], [2, 5], [7, 2], [5, 2]], np.int32)
    d = GroupedDev(kind, e, n, k, spare_experts=1)
    pairs = ids.size
    base16 = _base(kind, (e + 1) * n, k)
    for a_div in (2, 1):
        g = mo.grouped_problem(kind, ids, e + 1, n, k, a_div, base=base16)
        g = dataclasses.replace(g, e=e)
        runs = []
        for name, plan, keep in _bad_plans(ids, e):
            long_plan = np.concatenate([plan, np.arange(16, dtype=np.int32) % pairs])
            want = np.full((2 * pairs, n), mo.NAN, np.uint16)
            for q, x in keep.items():
                want[q] = gc.bits(base16.want[(q // a_div) % 16, x * n:(x + 1) * n]).numpy().astype(np.uint16)
            for cfg in (None, 0, 2):
                c = d.launch(hip, stream, g, cfg, plan=long_plan, c_rows=2 * pairs)
                runs.append((f"{kind} cfg {cfg}, a_div={a_div}, {name}", c, want))
        stream.sync()
        for what, c, want in runs:
            _assert_c(c, want, what)


# ---- 7. the combine ----------------------------------------------------------------------------------------------------

def _run_combine(hip, stream, c: mo.CombineCase, timed=False):
    ys, os_ = c.h + c.y_pad, c.h + c.out_pad
    y = np.full((c.m * c.topk, ys), mo.NAN, np.uint16)
    y[:, :c.h] = c.y
    out0 = np.full((c.m, os_), 0x5A5A, np.uint16)
    yb, wb, ob = Banded(y), Banded(c.w.astype(np.float32)), Banded(out0)
    torch.cuda.synchronize()
    args = (stream, yb.ptr(), ys, wb.ptr(), ob.ptr(), os_, c.m, c.topk, c.h)
    if timed:
        assert hip.time_moe_combine(*args, 3) > 0
    else:
        hip.moe_combine(*args)
    return yb, wb, ob


def _check_combine(c: mo.CombineCase, run):
    yb, wb, ob = run
    for b in run:
        b.assert_bands(c.name)
    got, want = ob.get(), mo.combine(c.y, c.w)
    assert (got[:, c.h:] == 0x5A5A).all(), f"{c.name}: the padding of out was written"
    got = got[:, :c.h]
    nan = (want & 0x7FFF) > 0x7F80
    assert (((got & 0x7FFF) > 0x7F80) == nan).all(), f"{c.name}: NaN where none is due, or none where one is"
    bad = np.argwhere((got != want) & ~nan)
    assert not len(bad), (f"{c.name}: {len(bad)} of {got.size} elements differ, first at {bad[0].tolist()}: got "
                          f"{int(got[tuple(bad[0])]):#06x}, want {int(want[tuple(bad[0])]):#06x}")


def test_combine_is_the_twin_bit_for_bit(hip, stream):
    """Every case of ``moe_cases.combine_cases``: topk 1, 2, 8 by H 8, 136, 4096, padded strides, weights 0 and 1, the
    FMA case, the case where the order of j matters; out between guard bands, its padding untouched."""
    cases = mo.combine_cases()
    runs = [_run_combine(hip, stream, c) for c in cases]
    stream.sync()
    for c, run in zip(cases, runs):
        _check_combine(c, run)


def test_time_moe_combine_leaves_the_result(hip, stream):
    c = mo.combine_cases()[4]
    run = _run_combine(hip, stream, c, timed=True)
    stream.sync()
    _check_combine(c, run)


# ---- 8. buffers that only touch, and refused calls --------------------------------------------------------------------

def test_outputs_that_touch_their_inputs_are_taken_and_refused_calls_write_nothing(hip, stream):
    """ids, weights and plan directly behind the logits and behind each other in one allocation: accepted and right.
    One byte of overlap is refused, and a refused call leaves every output as it was."""
    c = mo.grid_cases()[10]
    lg_bytes, pb, plb = c.m * c.e * 2, c.m * c.topk * 4, mo.PLAN_INTS * 4
    assert lg_bytes % 16 == 0
    buf = torch.full((lg_bytes + 2 * pb + plb,), FILL, dtype=torch.uint8, device="cuda")
    buf[:lg_bytes] = torch.from_numpy(c.bits.view(np.uint8).reshape(-1)).cuda()
    at = buf.data_ptr()
    ids_p, w_p, plan_p = at + lg_bytes, at + lg_bytes + pb, at + lg_bytes + 2 * pb
    before = buf.clone()
    torch.cuda.synchronize()
    with pytest.raises(hip.HipError, match="must not overlap"):
        hip.moe_route(stream, at, c.e, ids_p - 4, w_p, plan_p, c.m, c.e, c.topk)
    with pytest.raises(hip.HipError, match="need 1 <= M <= 16"):
        hip.moe_route(stream, at, c.e, ids_p, w_p, plan_p, 17, c.e, c.topk)
    stream.sync()
    assert torch.equal(buf, before), "a refused call wrote"
    hip.moe_route(stream, at, c.e, ids_p, w_p, plan_p, c.m, c.e, c.topk)
    stream.sync()
    host = buf.cpu().numpy()
    want_ids, _, want_plan = mo.route(c.bits, c.topk)
    assert np.array_equal(host[lg_bytes:lg_bytes + pb].view(np.int32).reshape(c.m, c.topk), want_ids)
    assert np.array_equal(host[lg_bytes + 2 * pb:].view(np.int32), want_plan)
    assert np.array_equal(host[:lg_bytes], before.cpu().numpy()[:lg_bytes])


# ---- 9. the chain ------------------------------------------------------------------------------------------------------

def test_moe_mlp_chain_stage_by_stage(hip, stream):
    """M = 5, hidden = 128, ffn = 64, E = 16, topk = 2: router GEMM, route, up, SwiGLU, down, combine.  Every stage is
    checked against its own reference applied to the GPU's output of the stage before: bits for the router GEMM and
    the up projection (the exact generators' operands), ids, plan and the combine; the header's bounds for the router
    weights and SwiGLU; the decode GEMM's bound for general inputs (``gemm_decode_cases.error_bound``) for the down
    projection, whose A is SwiGLU's output."""
    m, hidden, ffn, e, topk = 5, 128, 64, 16, 2
    pairs = m * topk
    xn_h, _ = gc.exact_operands(m, 16, hidden)
    rbase = _base("bf16", e, hidden)            # the router [E][hidden]
    ubase = _base("bf16", e * 2 * ffn, hidden)  # wgu [E][2 ffn][hidden]
    g = torch.Generator().manual_seed(9)
    wdown_h = (torch.randn(e * hidden, ffn, generator=g) / 8).bfloat16()
    assert torch.equal(xn_h, rbase.a[:m]) and torch.equal(xn_h, ubase.a[:m])
    xn, router, wgu, wdown = xn_h.cuda(), rbase.b.cuda(), ubase.b.cuda(), wdown_h.cuda()
    dev = lambda shape, dt: torch.full(shape, -1 if dt == torch.int32 else float("nan"), device="cuda", dtype=dt)  # noqa: E731
    bf = torch.bfloat16
    logits, ids, tw, plan = dev((m, e), bf), dev((m, topk), torch.int32), dev((m, topk), torch.float32), \
        dev((mo.PLAN_INTS,), torch.int32)
    gu, act, y, out = dev((pairs, 2 * ffn), bf), dev((pairs, ffn), bf), dev((pairs, hidden), bf), dev((m, hidden), bf)
    torch.cuda.synchronize()
    hip.decode_gemm_nt(stream, "bf16", xn.data_ptr(), router.data_ptr(), logits.data_ptr(), m, e, hidden)
    hip.moe_route(stream, logits.data_ptr(), e, ids.data_ptr(), tw.data_ptr(), plan.data_ptr(), m, e, topk)
    hip.moe_gemm_nt(stream, "bf16", xn.data_ptr(), topk, wgu.data_ptr(), gu.data_ptr(), plan.data_ptr(), m, topk, e,
                    2 * ffn, hidden)
    hip.silu_mul(stream, "bf16", gu.data_ptr(), 2 * ffn, act.data_ptr(), ffn, 0, pairs, ffn)
    hip.moe_gemm_nt(stream, "bf16", act.data_ptr(), 1, wdown.data_ptr(), y.data_ptr(), plan.data_ptr(), m, topk, e,
                    hidden, ffn)
    hip.moe_combine(stream, y.data_ptr(), hidden, tw.data_ptr(), out.data_ptr(), hidden, m, topk, hidden)
    stream.sync()
    # the router GEMM, exactly
    gc.assert_bits_equal(logits, rbase.want[:m], "the router GEMM")
    lbits = gc.bits(logits.cpu()).numpy().astype(np.uint16)
    # the route, from the GPU's logits
    want_ids, w64, want_plan = mo.route(lbits, topk)
    got_ids, got_w = ids.cpu().numpy(), tw.cpu().numpy().astype(np.float64)
    assert np.array_equal(got_ids, want_ids) and np.array_equal(plan.cpu().numpy(), want_plan), "the route"
    assert (np.abs(got_w - w64) <= mo.weight_bound(lbits, want_ids, w64)).all(), "the router's weights"
    # the up projection, exactly, from the GPU's ids
    want_gu = torch.stack([ubase.want[p // topk, int(x) * 2 * ffn:(int(x) + 1) * 2 * ffn]
                           for p, x in enumerate(got_ids.reshape(-1))])
    gc.assert_bits_equal(gu, want_gu, "the up projection")
    # SwiGLU, from the GPU's gu: the contract covers |g| <= 64
    gu_bits = gc.bits(gu.cpu()).numpy().astype(np.uint16)
    assert float(np.abs(sc.bf16_value(gu_bits[:, :ffn])).max()) <= 64
    act_bits = gc.bits(act.cpu()).numpy().astype(np.uint16)
    nc.check_silu(nc.SiluProblem(gu_bits, ffn), "bf16", nc.Result(act_bits), "SwiGLU")
    # the down projection, from the GPU's act: the bound for general inputs
    a64 = act.cpu().double()
    y_h = y.cpu()
    for p, x in enumerate(got_ids.reshape(-1)):
        w64_ = wdown_h[int(x) * hidden:(int(x) + 1) * hidden].double()
        ref, mag = a64[p:p + 1] @ w64_.t(), a64[p:p + 1].abs() @ w64_.abs().t()
        err = (y_h[p:p + 1].double() - ref).abs()
        assert bool((err <= dc.error_bound(ref, mag, ffn)).all()), f"the down projection, pair {p}"
    # the combine, exactly, from the GPU's y and weights
    want_out = mo.combine(gc.bits(y_h).numpy().astype(np.uint16), tw.cpu().numpy())
    assert np.array_equal(gc.bits(out.cpu()).numpy().astype(np.uint16), want_out), "the combine"


# ---- 10. the workload, end to end --------------------------------------------------------------------------------------

@pytest.mark.parametrize("workload", ["layer", "generate"])
def test_workload_moe_end_to_end(workload):
    """``gsxtools.workload --workload layer / generate --experts 16 --experts-active 2``: finite activations, tokens in
    range, and between 2 and 6 experts hit per layer (3 tokens that pick 2 of 16 each).  The rings are kept to a few
    layers, as in the other workload tests."""
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    extra = ["--vocab", "512"] if workload == "generate" else []
    r = subprocess.run([sys.executable, "-m", "gsxtools.workload", "--workload", workload, "--experts", "16",
                        "--experts-active", "2", "--heads", "2", "--kv-heads", "1", "--ffn", "64", "--context", "64",
                        "--batch", "3", "--iters", "10", "--json", "--weights-gib", "0.01", "--kv-gib", "0.0005", *extra],
                       env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["workload"] == workload and out["experts"] == 16 and out["experts_active"] == 2 and out["ffn"] == 64
    assert out["activations_finite"] is True and out["kernel"] == "gsx" and out["tbps"] > 0
    assert 2 <= out["experts_hit_mean"] <= 6, out["experts_hit_mean"]
    assert "last step" in out["tbps_basis"]
    if workload == "generate":
        assert out["tokens_in_range"] is True and out["vocab"] == 512
