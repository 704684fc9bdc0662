"""NumPy twins and cases for the MoE decode kernels (native/kernels/moe.hip and the grouped form of gemm_decode.hip).

Plain Python on NumPy and torch, no GPU.  The contracts are in ``native/kernels/gsx_kernels.h``:

* :func:`route` is the router's twin.  Selection, ids and the plan are exact; the weights are an fp64 reference, and
  :func:`weight_bound` is the header's ``delta`` around it.  The key order is the sampler's (``tests/sample_cases``).
* :func:`combine` is the combine's twin, fp32 operation by operation.
* :func:`grouped_problem` is the grouped product: a gather around the three GEMM families' exact generators and
  references (``tests/gemm_decode_cases``), so the kernel is held to the CPU's result bit for bit.

``FLAWS`` are twins that are wrong on purpose; :func:`flaw_cases` names, for each, cases of the GPU test's own lists
on which it must differ from the right twin.  ``tests/test_moe_cases.py`` checks all of this on the CPU.
"""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np
import torch

from tests import gemm_decode_cases as dc
from tests import gemm_fp8_cases as gf
from tests import sample_cases as sc

F32 = np.float32
MAX_PAIRS = 128
PLAN_INTS = 4 + 4 * MAX_PAIRS
NAN, PINF, NINF, NEG_ZERO = 0x7FC0, 0x7F80, 0xFF80, 0x8000
U = 2.0 ** -24
# the library's table (gsx_moe_gemm_cfg_name / _cfg_shape): name, columns of a strip, waves, K-tiles in flight, and the
# decode configuration of that shape
CFGS = {0: ("16/4w-f4", 16, 4, 4, 0), 1: ("16/8w-f4", 16, 8, 4, 1), 2: ("16/16w-f4", 16, 16, 4, 3),
        3: ("32/8w-f4", 32, 8, 4, 4)}
ALL = [*CFGS, None]  # None: the dispatching entry point
ROUTE_FLAWS = ("ties_high", "nan_above_inf", "neg_zero_below", "ids_index_order", "plan_by_pair")
COMBINE_FLAWS = ("fma", "reverse")
FLAWS = ROUTE_FLAWS + COMBINE_FLAWS


# ---- the router ---------------------------------------------------------------------------------------------------------

def route_keys(bits, flaw: str | None = None) -> np.ndarray:
    """The sampler's key; the flaw ``nan_above_inf`` lifts every NaN above +inf."""
    key = sc.keys(bits, "neg_zero_below" if flaw == "neg_zero_below" else None)
    if flaw == "nan_above_inf":
        b = np.asarray(bits).astype(np.int64)
        key = np.where((b & 0x7FFF) > 0x7F80, 0x10000, key)
    return key


def select(bits: np.ndarray, topk: int, flaw: str | None = None) -> np.ndarray:
    """``ids[M][topk]``: the topk largest keys of every row in descending key order, the lowest index first among
    equal keys."""
    key = route_keys(bits, flaw)
    idx = np.arange(bits.shape[1])
    out = np.empty((bits.shape[0], topk), np.int32)
    for m, row in enumerate(key):
        order = np.lexsort((-idx if flaw == "ties_high" else idx, -row))  # by key descending, then by index
        ids = order[:topk]
        out[m] = np.sort(ids) if flaw == "ids_index_order" else ids
    return out


def weights64(bits: np.ndarray, ids: np.ndarray) -> np.ndarray:
    """The exact softmax over the selected logits, in fp64, with the contract's special cases: a non-finite logit at
    ``first`` gives (1, 0, ..); a -inf or NaN logit weighs nothing."""
    out = np.zeros(ids.shape, np.float64)
    for m in range(ids.shape[0]):
        l = sc.bf16_value(bits[m, ids[m]]).astype(np.float64)
        if not np.isfinite(l[0]):
            out[m, 0] = 1.0
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            p = np.where(np.isfinite(l), np.exp(np.where(np.isfinite(l), l - l[0], 0.0)), 0.0)
        out[m] = p / p.sum()
    return out


def weight_bound(bits: np.ndarray, ids: np.ndarray, w64: np.ndarray) -> np.ndarray:
    """How far a weight may be from ``w64``: ``delta(x_j) w_j`` with ``delta = (3 |x_j| + 3.2 (topk - 1) + 4) 2^-24``
    and ``x_j = l_j - l_first`` where the exact weight is at least 2^-100, and 2^-99 below.  A weight the contract
    makes exactly 0 or 1 has the bound 0."""
    topk = ids.shape[1]
    out = np.zeros(ids.shape, np.float64)
    for m in range(ids.shape[0]):
        l = sc.bf16_value(bits[m, ids[m]]).astype(np.float64)
        if not np.isfinite(l[0]) or topk == 1:
            continue
        for j in range(topk):
            if not np.isfinite(l[j]):
                continue
            delta = (3.0 * abs(l[j] - l[0]) + 3.2 * (topk - 1) + 4.0) * U
            out[m, j] = delta * w64[m, j] if w64[m, j] >= 2.0 ** -100 else 2.0 ** -99
    return out


def plan_of(ids: np.ndarray, e: int, flaw: str | None = None) -> np.ndarray:
    """The plan of ``ids[M][topk]``: header, slot_expert, slot_begin, slot_count, rows."""
    flat = ids.reshape(-1)
    p = len(flat)
    assert p <= MAX_PAIRS
    plan = np.zeros(PLAN_INTS, np.int32)
    expert, begin, count, rows = (plan[4 + i * MAX_PAIRS:4 + (i + 1) * MAX_PAIRS] for i in range(4))
    expert[:], rows[:] = -1, -1
    active = sorted(set(flat.tolist()), key=(lambda x: flat.tolist().index(x)) if flaw == "plan_by_pair" else None)
    at = 0
    for s, x in enumerate(active):
        mine = np.flatnonzero(flat == x)
        expert[s], begin[s], count[s] = x, at, len(mine)
        rows[at:at + len(mine)] = mine
        at += len(mine)
    plan[:4] = len(active), p, e, 0
    return plan


def route(bits: np.ndarray, topk: int, flaw: str | None = None):
    """``(ids, w64, plan)`` for logits ``bits[M][E]`` (bf16 codes)."""
    ids = select(bits, topk, flaw)
    return ids, weights64(bits, ids), plan_of(ids, bits.shape[1], flaw)


def plan_fields(plan: np.ndarray):
    """``(n_active, P, E, slot_expert, slot_begin, slot_count, rows)``."""
    return (int(plan[0]), int(plan[1]), int(plan[2]),
            *(plan[4 + i * MAX_PAIRS:4 + (i + 1) * MAX_PAIRS] for i in range(4)))


# ---- the definitions again, slowly ---------------------------------------------------------------------------------

def _rank(code: int) -> tuple:
    """A bf16 code as something Python orders: NaN below everything, -0 equal to +0."""
    v = float(sc.bf16_value(np.array([code], np.uint16))[0])
    return (0, 0.0) if math.isnan(v) else (1, 0.0 if v == 0 else v)


def brute_select(bits: np.ndarray, topk: int) -> np.ndarray:
    """Repeated maximum: the best remaining index is the first that no other remaining index beats."""
    out = np.empty((bits.shape[0], topk), np.int32)
    for m in range(bits.shape[0]):
        left = list(range(bits.shape[1]))
        for j in range(topk):
            best = left[0]
            for i in left[1:]:
                if _rank(int(bits[m, i])) > _rank(int(bits[m, best])):
                    best = i
            out[m, j] = best
            left.remove(best)
    return out


def brute_plan(ids: np.ndarray, e: int) -> np.ndarray:
    """Expert by expert, pair by pair."""
    flat = [int(x) for x in ids.reshape(-1)]
    plan = [0] * PLAN_INTS
    for i in range(MAX_PAIRS):
        plan[4 + i], plan[4 + 3 * MAX_PAIRS + i] = -1, -1
    slot = at = 0
    for x in range(e):
        pairs = [p for p, v in enumerate(flat) if v == x]
        if not pairs:
            continue
        plan[4 + slot], plan[4 + MAX_PAIRS + slot], plan[4 + 2 * MAX_PAIRS + slot] = x, at, len(pairs)
        for p in pairs:
            plan[4 + 3 * MAX_PAIRS + at] = p
            at += 1
        slot += 1
    plan[:4] = [slot, len(flat), e, 0]
    return np.array(plan, np.int32)


def brute_weights(bits: np.ndarray, ids: np.ndarray) -> np.ndarray:
    """The softmax with ``math.exp`` and ``math.fsum``."""
    out = np.zeros(ids.shape, np.float64)
    for m in range(ids.shape[0]):
        l = [float(sc.bf16_value(np.array([bits[m, i]], np.uint16))[0]) for i in ids[m]]
        if not math.isfinite(l[0]):
            out[m, 0] = 1.0
            continue
        p = [math.exp(v - l[0]) if math.isfinite(v) else 0.0 for v in l]
        out[m] = [v / math.fsum(p) for v in p]
    return out


# ---- the combine ---------------------------------------------------------------------------------------------------------

def combine(y_bits: np.ndarray, w: np.ndarray, flaw: str | None = None) -> np.ndarray:
    """``out[M][H]`` bf16 codes from ``y_bits[M * topk][H]`` and ``w[M][topk]`` (fp32): ``acc = fl(w_0 y_0)``, then
    ``acc = fl(acc + fl(w_j y_j))`` in the order of j, and one rounding to bf16.  Flaws: ``fma`` rounds
    ``acc + w_j y_j`` once (in fp64 the product is exact); ``reverse`` starts from the last j."""
    m, topk = w.shape
    y = sc.bf16_value(y_bits).reshape(m, topk, -1)
    w = w.astype(F32)
    order = range(topk - 1, -1, -1) if flaw == "reverse" else range(topk)
    acc = None
    with np.errstate(invalid="ignore", over="ignore"):
        for j in order:
            if acc is None:
                acc = (w[:, j, None] * y[:, j]).astype(F32)
            elif flaw == "fma":
                acc = (acc.astype(np.float64) + w[:, j, None].astype(np.float64) * y[:, j].astype(np.float64)).astype(F32)
            else:
                acc = (acc + (w[:, j, None] * y[:, j]).astype(F32)).astype(F32)
    return sc.bf16_bits(acc).reshape(m, -1)


def brute_combine(y_bits: np.ndarray, w: np.ndarray) -> np.ndarray:
    """Element by element with NumPy fp32 scalars."""
    m, topk = w.shape
    h = y_bits.shape[1]
    out = np.empty((m, h), np.uint16)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(m):
            for c in range(h):
                acc = None
                for j in range(topk):
                    prod = F32(w[r, j]) * F32(sc.bf16_value(np.array([y_bits[r * topk + j, c]], np.uint16))[0])
                    acc = prod if acc is None else F32(acc + prod)
                out[r, c] = sc.bf16_bits(np.array([acc], F32))[0]
    return out


# ---- router cases ---------------------------------------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class RouteCase:
    name: str
    bits: np.ndarray  # [M][E] bf16 codes
    topk: int
    pad: int = 0      # columns of padding behind every row, filled with NaN

    @property
    def m(self) -> int:
        return self.bits.shape[0]

    @property
    def e(self) -> int:
        return self.bits.shape[1]


def _rows(row, m):
    return np.tile(np.asarray(row, np.uint16), (m, 1))


def random_logits(rng, m, e, sigma=2.0) -> np.ndarray:
    return sc.bf16_bits(rng.normal(0.0, sigma, (m, e)).astype(F32))


GRID_E, GRID_K, GRID_M = (8, 16, 128, 1024), (1, 2, 8), (1, 5, 16)


def grid_cases() -> list[RouteCase]:
    rng = np.random.default_rng(4101)
    return [RouteCase(f"random E={e} topk={k} M={m}", random_logits(rng, m, e), k)
            for e in GRID_E for k in GRID_K for m in GRID_M]


def equal_and_two_valued_cases() -> list[RouteCase]:
    """All logits equal; two-valued rows whose upper group has topk - 1, topk or topk + 1 members, so that the tie of
    the lower (or the upper) group straddles the topk-th place."""
    out = [RouteCase(f"all equal E={e} topk={k}", _rows(np.full(e, 0x3F80), 3), k) for e in (8, 128) for k in (1, 2, 8)]
    for e, k in ((16, 2), (128, 8), (1024, 8)):
        for hi in (k - 1, k, k + 1):
            row = np.full(e, 0x3F00, np.uint16)  # 0.5
            row[np.linspace(3, e - 2, hi).astype(int)] = 0x3F80  # 1.0
            out.append(RouteCase(f"two-valued E={e} topk={k}, {hi} high", _rows(row, 2), k))
    return out


def shared_and_distinct_cases() -> list[RouteCase]:
    """Every row identical (one expert set with 16 rows each) and rows that hit P distinct experts."""
    rng = np.random.default_rng(4102)
    out = [RouteCase("16 identical rows, topk 8", _rows(random_logits(rng, 1, 128)[0], 16), 8),
           RouteCase("16 identical rows, topk 1", _rows(random_logits(rng, 1, 16)[0], 16), 1)]
    for m, k, e in ((16, 8, 128), (16, 8, 1024), (5, 2, 16), (8, 1, 8)):
        bits = np.full((m, e), 0xC000, np.uint16)  # -2
        perm = rng.permutation(e)[:m * k].reshape(m, k)
        for r in range(m):
            bits[r, perm[r]] = sc.bf16_bits(np.linspace(1.0, 2.0, k).astype(F32))
        out.append(RouteCase(f"{m * k} distinct experts of {e}", bits, k))
    return out


def special_value_cases() -> list[RouteCase]:
    e = 16
    base = np.full(e, 0xBF80, np.uint16)  # -1
    zeros = base.copy()
    zeros[[2, 5, 9]] = NEG_ZERO, 0, NEG_ZERO  # -0 at 2 ties +0 at 5: the lowest index first
    inf_first = base.copy()
    inf_first[[4, 7]] = PINF, 0x4000
    all_ninf = np.full(e, NINF, np.uint16)
    nan_row = np.full(e, NAN, np.uint16)
    nan_mixed = base.copy()
    nan_mixed[[0, 3, 8]] = NAN, PINF, 0xFFC0  # NaN of both signs below everything, +inf first
    nan_and_ninf = np.full(e, NINF, np.uint16)
    nan_and_ninf[[1, 6]] = NAN, 0x3F80
    few = np.full(e, NINF, np.uint16)
    few[[3, 11]] = 0x3F80, 0x4000  # two finite logits, then -inf by index
    few_nan = np.full(e, NAN, np.uint16)
    few_nan[[12, 13]] = 0x4000, NINF  # one finite, one -inf, then NaN by index
    out = [RouteCase("-0 and +0", _rows(zeros, 2), 2), RouteCase("-0 and +0, topk 8", _rows(zeros, 2), 8),
           RouteCase("+inf first", _rows(inf_first, 2), 2), RouteCase("all -inf", _rows(all_ninf, 2), 2),
           RouteCase("a row of NaN", _rows(nan_row, 2), 2), RouteCase("NaN of both signs, +inf", _rows(nan_mixed, 2), 8),
           RouteCase("NaN among -inf", _rows(nan_and_ninf, 1), 2),
           RouteCase("fewer than topk finite", _rows(few, 3), 8), RouteCase("one finite, -inf, NaN", _rows(few_nan, 3), 8)]
    for gap in (0.0, 1.0, 40.0):
        row = np.full(e, 0xC2C8, np.uint16)  # -100
        row[[3, 10]] = sc.bf16_bits(np.array([5.0, 5.0 - gap], F32))
        out.append(RouteCase(f"gap {gap:g}", _rows(row, 2), 2))
    slope = sc.bf16_bits(np.linspace(3.0, -37.0, 8).astype(F32))  # gaps up to 40 inside one softmax of 8
    out.append(RouteCase("a slope of 40 over 8", _rows(slope, 2), 8))
    rng = np.random.default_rng(4103)
    out.append(RouteCase("padded stride, NaN in the padding", random_logits(rng, 5, 24), 2, pad=8))
    out.append(RouteCase("padded stride, E = 1024", random_logits(rng, 16, 1024), 8, pad=16))
    return out


def route_cases() -> list[RouteCase]:
    """Everything the GPU test runs."""
    return [*grid_cases(), *equal_and_two_valued_cases(), *shared_and_distinct_cases(), *special_value_cases()]


# ---- combine cases ---------------------------------------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class CombineCase:
    name: str
    y: np.ndarray  # [M * topk][H] bf16 codes
    w: np.ndarray  # [M][topk] fp32
    y_pad: int = 0
    out_pad: int = 0

    @property
    def m(self) -> int:
        return self.w.shape[0]

    @property
    def topk(self) -> int:
        return self.w.shape[1]

    @property
    def h(self) -> int:
        return self.y.shape[1]


def _softmax_w(rng, m, topk) -> np.ndarray:
    x = rng.normal(0, 1, (m, topk))
    p = np.exp(x - x.max(1, keepdims=True))
    return (p / p.sum(1, keepdims=True)).astype(F32)


@functools.lru_cache(maxsize=None)
def _find_fma_case() -> tuple[np.ndarray, np.ndarray]:
    """``(y_bits[8][8], w[4][2])``: four rows on which one rounding of ``acc + w_1 y_1`` gives another bf16 than two,
    found by search over 2^20 random draws, as the sampler's FMA case is: the fp32 sums must differ and lie on either
    side of a rounding boundary of bf16."""
    rng = np.random.default_rng(4104)
    n = 1 << 20
    w = _softmax_w(rng, n, 2)
    y = sc.bf16_bits(rng.normal(0, 1, (2 * n, 1)).astype(F32))
    rows = np.flatnonzero(combine(y, w)[:, 0] != combine(y, w, "fma")[:, 0])[:4]
    if len(rows) < 4:
        raise AssertionError("no rows found whose sum an FMA changes")
    pairs = np.stack([2 * rows, 2 * rows + 1], 1).reshape(-1)
    return np.tile(y[pairs], (1, 8)), w[rows]


def fma_case() -> CombineCase:
    y, w = _find_fma_case()
    return CombineCase("an FMA changes the sum", y, w)


def order_case() -> CombineCase:
    """2^24 + 1 + 1 - 2^24 with weights of 1: from the front each 1 is lost in fl(2^24 + 1) = 2^24 and the sum is 0;
    from the back every partial sum is exact and the sum is 2."""
    big, one = 0x4B80, 0x3F80  # 2^24 and 1
    y = np.array([[big] * 8, [one] * 8, [one] * 8, [0xCB80] * 8], np.uint16)  # 2^24, 1, 1, -2^24
    w = np.ones((1, 4), F32)
    return CombineCase("the order of j matters", y, w)


def combine_cases() -> list[CombineCase]:
    rng = np.random.default_rng(4105)
    out = []
    for topk in (1, 2, 8):
        for h in (8, 136, 4096):
            m = 5 if h < 4096 else 3
            y = sc.bf16_bits(rng.normal(0, 1, (m * topk, h)).astype(F32))
            out.append(CombineCase(f"random topk={topk} H={h}", y, _softmax_w(rng, m, topk)))
    y = sc.bf16_bits(rng.normal(0, 1, (16 * 8, 136)).astype(F32))
    out.append(CombineCase("M = 16, padded strides", y, _softmax_w(rng, 16, 8), y_pad=8, out_pad=24))
    w01 = np.zeros((4, 2), F32)
    w01[:, 0] = 1.0
    w01[2] = 0.0, 1.0
    w01[3] = 0.0, 0.0
    y = sc.bf16_bits(rng.normal(0, 1, (8, 136)).astype(F32))
    y[1, :8] = NAN  # 0 * NaN is NaN: a weight of 0 does not hide its row
    out.append(CombineCase("weights 0 and 1", y, w01))
    return [*out, fma_case(), order_case()]


def flaw_cases() -> dict[str, list]:
    """For every flaw, cases of :func:`route_cases` or :func:`combine_cases` on which the flawed twin must differ."""
    by_name = {c.name: c for c in [*route_cases(), *combine_cases()]}
    pick = lambda *names: [by_name[n] for n in names]  # noqa: E731
    return {"ties_high": pick("all equal E=8 topk=2", "two-valued E=16 topk=2, 1 high"),
            "nan_above_inf": pick("NaN of both signs, +inf", "NaN among -inf"),
            "neg_zero_below": pick("-0 and +0"),
            "ids_index_order": pick("10 distinct experts of 16", "fewer than topk finite"),
            "plan_by_pair": pick("128 distinct experts of 1024", "random E=128 topk=8 M=16"),
            "fma": pick("an FMA changes the sum"), "reverse": pick("the order of j matters")}


# ---- the grouped product ---------------------------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class Grouped:
    """One grouped product: ``a`` has ``ceil(P / a_div)`` rows, ``b`` is ``[E * N][K]`` (the experts back to back),
    ``want[P][N]`` the bf16 result; ``sa`` per row of A and ``sb`` per row of ``b`` as the kind takes them."""
    kind: str
    a: torch.Tensor
    b: torch.Tensor
    want: torch.Tensor
    ids: np.ndarray  # [M][topk]
    plan: np.ndarray
    a_div: int
    e: int
    n: int
    sa: torch.Tensor | None = None
    sb: torch.Tensor | None = None
    mode: int = gf.SCALE_NONE

    @property
    def m(self) -> int:
        return self.ids.shape[0]

    @property
    def topk(self) -> int:
        return self.ids.shape[1]

    @property
    def k(self) -> int:
        return self.a.shape[1] * (2 if self.kind == "mxfp4" else 1)


def grouped_problem(kind: str, ids: np.ndarray, e: int, n: int, k: int, a_div: int, fp8_row: bool = False,
                    base: dc.Problem | None = None) -> Grouped:
    """The exact generators' case with 16 rows of A and ``e * n`` rows of B (``base``, made here if not given):
    expert x is rows ``x n .. x n + n - 1``.  Row r of the grouped A is row ``r % 16`` of the case's, so the wanted
    row of pair p against expert x is row ``(p // a_div) % 16`` of the case's result, columns ``x n ..``: a gather,
    nothing is computed here.  ``fp8_row`` adds random 24-bit scales per row of A and per (expert, column)."""
    m, topk = ids.shape
    pairs = m * topk
    base = dc.exact_problem(kind, e * n, k) if base is None else base
    assert base.kind == kind and base.n == e * n and base.k == k and base.m == dc.MAX_M
    a_rows = -(-pairs // a_div)
    src = np.arange(a_rows) % dc.MAX_M
    sa, sb, mode, want16 = base.sa, base.sb, base.mode, base.want
    if kind == "fp8" and fp8_row:
        sa16, sb, mode = gf.row_scales(dc.MAX_M, 41), gf.row_scales(e * n, 43), gf.SCALE_ROW
        want16 = gf.scaled(base.acc, sa16, sb)
        sa = sa16[src].contiguous()
    elif kind == "mxfp4":
        sa = base.sa[src].contiguous()
    want = torch.empty(pairs, n, dtype=torch.bfloat16)
    for p, x in enumerate(ids.reshape(-1)):
        want[p] = want16[src[p // a_div], int(x) * n:(int(x) + 1) * n]
    return Grouped(kind, base.a[src].contiguous(), base.b, want, ids, plan_of(ids, e), a_div, e, n, sa, sb, mode)


def routings(e: int) -> list[tuple[str, np.ndarray]]:
    """``(name, ids[M][topk])``: one pair; 16 rows on one expert; P experts with a row each; every expert full (with
    8 experts); three random routings."""
    rng = np.random.default_rng(4106 + e)
    out = [("M=1 topk=1", np.array([[e - 3]], np.int32)),
           ("16 rows on one expert", np.full((16, 1), e // 2 + 1, np.int32)),
           ("a row each", rng.permutation(e)[:min(e, 24) // 3 * 3].reshape(-1, 3).astype(np.int32))]
    if e == 8:
        out.append(("every expert full", np.tile(np.arange(8, dtype=np.int32), (16, 1))))
    for m, topk in ((5, 2), (16, 4), (11, 8)):
        topk = min(topk, e)
        ids = np.stack([rng.permutation(e)[:topk] for _ in range(m)]).astype(np.int32)
        out.append((f"random M={m} topk={topk}", ids))
    return out


def nk_counts(cfg, kind: str) -> list[int]:
    """K-tile counts for the grouped kernel's tests: 1, W - 1 and W + 1 (waves without a tile, a ragged round),
    2 F W (the steady loop is first entered by every wave) and one long loop, 4 F W + 3, as far as the kind's exact
    generator reaches; the dispatching entry point takes the counts of every configuration it can pick."""
    if cfg is None:
        return sorted({nk for c in CFGS for nk in nk_counts(c, kind)})
    _, _, w, f, _ = CFGS[cfg]
    return sorted(nk for nk in {1, w - 1, w + 1, 2 * f * w, 4 * f * w + 3} if nk * dc.BK[kind] <= dc.MAX_K[kind])


MOE_ROUTE_REFUSALS = ("need 1 <= M <= 16", "need 8 <= E <= 1024 and E % 8 == 0", "need 1 <= topk <= min\\(8, E\\)",
                      "need logits_stride >= E and logits_stride % 8 == 0",
                      "logits, topk_ids, topk_w and plan must not be NULL", "logits must be 16-B aligned",
                      "topk_ids, topk_w and plan must be 4-B aligned",
                      "topk_ids, topk_w and plan must not overlap logits or each other")
