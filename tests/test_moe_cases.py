"""The MoE twins and cases (tests/moe_cases.py) on the CPU: the twins against definitions written a second, slower way,
the flawed twins against the cases that must catch them, what the three entry points refuse by name, and the tools'
parsers.  No GPU."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import gemm_decode_cases as dc  # noqa: E402
from tests import gemm_fp8_cases as gf  # noqa: E402
from tests import moe_cases as mo  # noqa: E402
from tests import sample_cases as sc  # noqa: E402


@pytest.fixture(scope="module")
def hip():
    from gpushare_scheduler_extender_amd.ops import hip as h

    h.lib()
    assert hasattr(h, "moe_route") and hasattr(h, "moe_gemm_nt") and hasattr(h, "moe_combine"), \
        "the bindings have no MoE entry points"
    return h


# ---- the twins against brute force ---------------------------------------------------------------------------------

def test_router_twin_agrees_with_the_slow_definitions():
    """Selection and ids by repeated maximum (rows of up to 128 logits; the rows of 1024 by their first and last
    row), the plan expert by expert, the weights with ``math.exp`` and ``math.fsum``."""
    for c in mo.route_cases():
        ids, w64, plan = mo.route(c.bits, c.topk)
        rows = range(c.m) if c.e <= 128 else (0, c.m - 1)
        for r in rows:
            assert (ids[r] == mo.brute_select(c.bits[r:r + 1], c.topk)[0]).all(), (c.name, r)
        assert (plan == mo.brute_plan(ids, c.e)).all(), c.name
        np.testing.assert_allclose(w64, mo.brute_weights(c.bits, ids), rtol=1e-14, atol=0, err_msg=c.name)
        assert ids.min() >= 0 and ids.max() < c.e and all(len(set(r)) == c.topk for r in ids.tolist()), c.name
        live = ~np.isnan(w64).any(1)
        np.testing.assert_allclose(w64[live].sum(1), 1.0, rtol=1e-14, err_msg=c.name)


def test_plan_invariants():
    """Slots in ascending expert order, runs that tile rows[0, P) in slot order, ascending pairs inside a run, unused
    slots {-1, 0, 0} and unused rows -1; at most 16 rows an expert."""
    for c in mo.route_cases():
        ids, _, plan = mo.route(c.bits, c.topk)
        n, p, e, expert, begin, count, rows = mo.plan_fields(plan)
        assert (p, e, plan[3]) == (c.m * c.topk, c.e, 0) and 1 <= n <= min(p, e)
        assert list(expert[:n]) == sorted(set(ids.reshape(-1).tolist())), c.name
        assert (expert[n:] == -1).all() and (begin[n:] == 0).all() and (count[n:] == 0).all() and (rows[p:] == -1).all()
        at = 0
        for s in range(n):
            assert begin[s] == at and 1 <= count[s] <= 16
            run = rows[at:at + count[s]]
            assert list(run) == sorted(run) and (ids.reshape(-1)[run] == expert[s]).all()
            at += count[s]
        assert at == p and sorted(rows[:p]) == list(range(p))


def test_the_cases_reach_what_they_are_named_for():
    by_name = {c.name: c for c in mo.route_cases()}
    assert len(by_name) == len(mo.route_cases())
    assert {(c.e, c.topk, c.m) for c in mo.grid_cases()} == \
        {(e, k, m) for e in mo.GRID_E for k in mo.GRID_K for m in mo.GRID_M}
    n_active = {name: int(mo.route(c.bits, c.topk)[2][0]) for name, c in by_name.items()}
    assert n_active["16 identical rows, topk 8"] == 8 and n_active["16 identical rows, topk 1"] == 1
    assert n_active["128 distinct experts of 128"] == 128 and n_active["128 distinct experts of 1024"] == 128
    _, _, plan = mo.route(by_name["16 identical rows, topk 8"].bits, 8)
    assert (mo.plan_fields(plan)[5][:8] == 16).all()
    ids, w, _ = mo.route(by_name["+inf first"].bits, 2)
    assert ids[0, 0] == 4 and w[0].tolist() == [1.0, 0.0]
    ids, w, _ = mo.route(by_name["all -inf"].bits, 2)
    assert ids[0].tolist() == [0, 1] and w[0].tolist() == [1.0, 0.0]
    ids, w, _ = mo.route(by_name["a row of NaN"].bits, 2)
    assert ids[0].tolist() == [0, 1] and w[0].tolist() == [1.0, 0.0]
    ids, w, _ = mo.route(by_name["fewer than topk finite"].bits, 8)
    assert ids[0].tolist() == [11, 3, 0, 1, 2, 4, 5, 6] and (w[0, 2:] == 0).all() and w[0, 0] > w[0, 1] > 0
    ids, w, _ = mo.route(by_name["one finite, -inf, NaN"].bits, 8)
    assert ids[0].tolist() == [12, 13, 0, 1, 2, 3, 4, 5] and w[0].tolist() == [1.0] + [0.0] * 7
    ids, _, _ = mo.route(by_name["-0 and +0"].bits, 2)
    assert ids[0].tolist() == [2, 5]
    for gap in (0.0, 1.0, 40.0):
        _, w, _ = mo.route(by_name[f"gap {gap:g}"].bits, 2)
        assert math.isclose(w[0, 1] / w[0, 0], math.exp(-gap), rel_tol=1e-12)
    for c in mo.equal_and_two_valued_cases():
        if c.name.startswith("two-valued"):
            ids, _, _ = mo.route(c.bits, c.topk)
            hi = int(c.name.split(",")[1].split()[0])
            assert (c.bits[0, ids[0]] == 0x3F80).sum() == min(hi, c.topk)


def test_weight_bound_is_the_headers():
    """(3 |x| + 3.2 (topk - 1) + 4) 2^-24 relative; 2^-99 absolute below 2^-100; 0 where the contract is exact."""
    by_name = {c.name: c for c in mo.route_cases()}
    c = by_name["gap 40"]
    ids, w, _ = mo.route(c.bits, 2)
    b = mo.weight_bound(c.bits, ids, w)
    assert b[0, 1] == (3 * 40 + 3.2 + 4) * 2.0 ** -24 * w[0, 1] and b[0, 0] == (3.2 + 4) * 2.0 ** -24 * w[0, 0]
    c = by_name["+inf first"]
    ids, w, _ = mo.route(c.bits, 2)
    assert (mo.weight_bound(c.bits, ids, w) == 0).all()
    c = by_name["fewer than topk finite"]
    ids, w, _ = mo.route(c.bits, 8)
    assert (mo.weight_bound(c.bits, ids, w)[:, 2:] == 0).all()
    c = by_name["random E=16 topk=1 M=5"]
    ids, w, _ = mo.route(c.bits, 1)
    assert (w == 1.0).all() and (mo.weight_bound(c.bits, ids, w) == 0).all()
    far = np.full((1, 8), 0xC2C8, np.uint16)  # -100
    far[0, 0] = 0x42C8  # 100: the others weigh e^-200 < 2^-100
    ids, w, _ = mo.route(far, 2)
    assert 0 < w[0, 1] < 2.0 ** -100 and mo.weight_bound(far, ids, w)[0, 1] == 2.0 ** -99


def test_combine_twin_agrees_with_the_slow_definition():
    for c in mo.combine_cases():
        cut = CombineCut(c)
        assert (mo.combine(cut.y, cut.w) == mo.brute_combine(cut.y, cut.w)).all(), c.name


class CombineCut:
    """The first 3 rows and 16 columns of a case: the scalar definition is slow."""

    def __init__(self, c):
        m, h = min(c.m, 3), min(c.h, 16)
        self.w = c.w[:m]
        self.y = c.y[:m * c.topk, :h]


def test_combine_cases_reach_what_they_are_named_for():
    cases = {c.name: c for c in mo.combine_cases()}
    assert {(c.topk, c.h) for c in cases.values()} >= {(k, h) for k in (1, 2, 8) for h in (8, 136, 4096)}
    c = cases["the order of j matters"]
    assert sc.bf16_value(mo.combine(c.y, c.w))[0, 0] == 0.0 and sc.bf16_value(mo.combine(c.y, c.w, "reverse"))[0, 0] == 2.0
    c = cases["weights 0 and 1"]
    out = mo.combine(c.y, c.w)
    assert (out[0, 8:] == c.y[0, 8:]).all() and (out[2] == c.y[5]).all()
    assert (np.isnan(sc.bf16_value(out[0, :8]))).all()  # 1 * y + 0 * NaN
    c = cases["an FMA changes the sum"]
    assert (mo.combine(c.y, c.w) != mo.combine(c.y, c.w, "fma")).all()


# ---- the flawed twins --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flaw", mo.FLAWS)
def test_every_flawed_twin_is_caught_by_its_cases(flaw):
    """Every case listed for a flaw is one of the GPU test's, and the flawed twin differs from the right one on it."""
    gpu_runs = {c.name for c in [*mo.route_cases(), *mo.combine_cases()]}
    cases = mo.flaw_cases()[flaw]
    assert cases and set(mo.flaw_cases()) == set(mo.FLAWS)
    for c in cases:
        assert c.name in gpu_runs
        if flaw in mo.ROUTE_FLAWS:
            ids, _, plan = mo.route(c.bits, c.topk)
            fids, _, fplan = mo.route(c.bits, c.topk, flaw)
            assert (ids != fids).any() or (plan != fplan).any(), (flaw, c.name)
        else:
            assert (mo.combine(c.y, c.w) != mo.combine(c.y, c.w, flaw)).any(), (flaw, c.name)


# ---- the grouped product ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", dc.KINDS)
def test_grouped_problem_is_the_families_reference_gathered(kind):
    """For both ``a_div`` and every routing: row p of the wanted result is the family's reference of the row of A the
    pair reads against its expert's matrix, computed here from the grouped problem's own operands."""
    e, n, k = 8, 48, 2 * dc.BK[kind]
    for name, ids in mo.routings(e):
        for a_div in (ids.shape[1], 1):
            for row_scales in ((False, True) if kind == "fp8" else (False,)):
                g = mo.grouped_problem(kind, ids, e, n, k, a_div, row_scales)
                pairs = ids.size
                assert g.a.shape[0] == -(-pairs // a_div) and g.b.shape[0] == e * n and g.want.shape == (pairs, n)
                for p, x in enumerate(ids.reshape(-1)):
                    r, cols = p // a_div, slice(int(x) * n, (int(x) + 1) * n)
                    per_row = kind == "mxfp4" or g.mode == gf.SCALE_ROW
                    one = dc.Problem(kind, g.a[r:r + 1], g.b[cols], g.want[p:p + 1],
                                     None if g.sa is None else g.sa[r:r + 1] if per_row else g.sa,
                                     None if g.sb is None else g.sb[cols], g.mode)
                    assert torch.equal(one.reference().view(torch.int16), g.want[p:p + 1].view(torch.int16)), \
                        (kind, name, a_div, p)


def test_routings_and_tile_counts():
    for e in (8, 256):
        for name, ids in mo.routings(e):
            assert ids.dtype == np.int32 and 1 <= ids.shape[0] <= 16 and 1 <= ids.shape[1] <= 8, name
            assert ids.min() >= 0 and ids.max() < e and all(len(set(r)) == ids.shape[1] for r in ids.tolist()), name
    names = [n for n, _ in mo.routings(8)]
    assert "every expert full" in names and len([n for n in names if n.startswith("random")]) == 3
    assert mo.nk_counts(1, "bf16") == [1, 7, 9, 64, 131] and mo.nk_counts(2, "mxfp4") == [1, 15, 17, 128]
    assert set(mo.nk_counts(None, "fp8")) == {nk for c in mo.CFGS for nk in mo.nk_counts(c, "fp8")}


def test_cfg_table_is_the_librarys(hip):
    assert hip.moe_gemm_cfgs() == mo.CFGS
    dcfgs = hip.decode_gemm_cfgs()
    for name, bn, waves, inflight, d in mo.CFGS.values():
        assert dcfgs[d] == (name, bn, waves, inflight)
    assert (hip.MOE_MAX_PAIRS, hip.MOE_PLAN_INTS) == (mo.MAX_PAIRS, mo.PLAN_INTS) == (128, 516)


# ---- what the entry points refuse --------------------------------------------------------------------------------------

# Addresses that are never dereferenced: every call below is refused before the first device call.
LG, IDS, TW, PLAN, A, B, C, SA, SB, Y, OUT = (0x10000000 * i for i in range(1, 12))


class _NoStream:
    """Stands in for ``hip.Stream``: the calls under test never get as far as using one."""
    handle = None


ROUTE_GOOD = {"lg": LG, "ls": 136, "ids": IDS, "tw": TW, "plan": PLAN, "m": 16, "e": 128, "topk": 8}


def _route_call(hip, v, timed=False):
    args = (_NoStream, v["lg"], v["ls"], v["ids"], v["tw"], v["plan"], v["m"], v["e"], v["topk"])
    return hip.time_moe_route(*args, 1) if timed else hip.moe_route(*args)


@pytest.mark.parametrize("timed", [False, True], ids=["launch", "timed"])
def test_moe_route_rejects_bad_arguments_by_name(hip, timed):
    def rej(text, **kw):
        with pytest.raises(hip.HipError, match=f"gsx_moe_route: {text}"):
            _route_call(hip, {**ROUTE_GOOD, **kw}, timed)

    for m in (0, -1, 17):
        rej("need 1 <= M <= 16", m=m)
    for e in (0, 4, 12, 1032, 2048, -8):
        rej("need 8 <= E <= 1024 and E % 8 == 0", e=e, ls=4096)
    for topk in (0, -1, 9):
        rej(r"need 1 <= topk <= min\(8, E\)", topk=topk)
    for ls in (120, 132, 0):
        rej("need logits_stride >= E and logits_stride % 8 == 0", ls=ls)
    for name in ("lg", "ids", "tw", "plan"):
        rej("logits, topk_ids, topk_w and plan must not be NULL", **{name: 0})
    rej("logits must be 16-B aligned", lg=LG + 8)
    for name in ("ids", "tw", "plan"):
        rej("topk_ids, topk_w and plan must be 4-B aligned", **{name: ROUTE_GOOD[name] + 2})
    lg_bytes, pair_bytes, plan_bytes = (15 * 136 + 128) * 2, 128 * 4, 516 * 4
    overlap = "topk_ids, topk_w and plan must not overlap logits or each other"
    for name, size in (("ids", pair_bytes), ("tw", pair_bytes), ("plan", plan_bytes)):
        for at in (LG, LG + lg_bytes - 4, LG - size + 4):
            rej(overlap, **{name: at})
    rej(overlap, ids=TW + pair_bytes - 4)
    rej(overlap, ids=PLAN - pair_bytes + 4)
    rej(overlap, tw=PLAN + plan_bytes - 4)


def test_moe_route_accepts_what_lies_next_to_a_refusal(hip):
    """The limits themselves, checked through a refusal that comes later: M = 1 and 16, E = 8 and 1024, topk = E = 8,
    a stride of exactly E; the alignment rule is the last one before the overlaps."""
    for kw in ({"m": 1}, {"m": 16}, {"e": 8, "ls": 8}, {"e": 1024, "ls": 1024}, {"topk": 1}, {"e": 8, "ls": 8, "topk": 8},
               {"ls": 128}):
        with pytest.raises(hip.HipError, match="gsx_moe_route: logits must be 16-B aligned"):
            _route_call(hip, {**ROUTE_GOOD, **kw, "lg": LG + 8})


def _gemm_good(kind):
    k = 4 * dc.BK[kind]
    v = {"a": A, "a_div": 8, "b": B, "c": C, "plan": PLAN, "m": 16, "topk": 8, "e": 64, "n": 96, "k": k, "sa": 0,
         "sb": 0, "mode": gf.SCALE_NONE}
    if kind == "mxfp4":
        v.update(sa=SA, sb=SB)
    return v


def _gemm_call(hip, kind, v, timed=False, cfg=None):
    args = (_NoStream, kind, v["a"], v["a_div"], v["b"], v["c"], v["plan"], v["m"], v["topk"], v["e"], v["n"], v["k"])
    if timed:
        return hip.time_moe_gemm(*args, 1, v["sa"], v["sb"], v["mode"])
    if cfg is not None:
        return hip.moe_gemm_nt_cfg(*args, cfg, v["sa"], v["sb"], v["mode"])
    return hip.moe_gemm_nt(*args, v["sa"], v["sb"], v["mode"])


@pytest.mark.parametrize("timed", [False, True], ids=["launch", "timed"])
@pytest.mark.parametrize("kind", dc.KINDS)
def test_moe_gemm_rejects_bad_arguments_by_name(hip, kind, timed):
    good = _gemm_good(kind)
    bk = dc.BK[kind]

    def rej(text, **kw):
        with pytest.raises(hip.HipError, match=f"gsx_moe_gemm_nt: {text}"):
            _gemm_call(hip, kind, {**good, **kw}, timed)

    for m in (0, 17):
        rej("need 1 <= M <= 16", m=m)
    rej("need E >= 1", e=0)
    for kw in ({"topk": 0}, {"topk": 9}, {"topk": 8, "e": 7}):
        rej(r"need 1 <= topk <= min\(8, E\)", **kw)
    for a_div in (0, -1):
        rej("need a_div >= 1", a_div=a_div)
    for kw in ({"n": 0}, {"n": 8}, {"n": 104}, {"k": 0}, {"k": bk // 2}, {"k": 3 * bk // 2}):
        rej(f"need N%16==0, K%{bk}==0", **kw)
    for name in ("a", "b", "c", "plan"):
        rej("A, B, C and plan must not be NULL", **{name: 0})
    for name in ("a", "b", "c"):
        rej("operands must be 16-B aligned", **{name: good[name] + 8})
    rej("plan must be 4-B aligned", plan=PLAN + 2)
    if kind == "bf16":
        for kw in ({"sa": SA}, {"sb": SB}, {"mode": gf.SCALE_ROW}):
            rej("bf16 takes no scales: scale_a and scale_b must be NULL and scale_mode NONE", **kw)
    elif kind == "fp8":
        for mode in (gf.SCALE_TENSOR, 3, -1):
            rej("fp8 takes scale_mode NONE or ROW", mode=mode, sa=SA, sb=SB)
        for kw in ({"sa": 0, "sb": SB}, {"sa": SA, "sb": 0}):
            rej("scale_a and scale_b must not be NULL in this scale_mode", mode=gf.SCALE_ROW, **kw)
        rej("scale_a and scale_b must be 4-B aligned", mode=gf.SCALE_ROW, sa=SA + 2, sb=SB)
    else:
        rej("mxfp4 takes scale_mode NONE: its scales are the e8m0 blocks", mode=gf.SCALE_ROW)
        for kw in ({"sa": 0}, {"sb": 0}):
            rej("scale_a and scale_b must not be NULL", **kw)
        rej("scale_a and scale_b must be 16-B aligned", sa=SA + 8)
    # 17 rows (16 of A and one more) of K elements must fit 2^32 - 1 bytes
    unit = {"bf16": 2.0, "fp8": 1.0, "mxfp4": 0.5}[kind]
    big = int((1 << 32) / 17 / unit) // bk * bk + bk
    if big < 1 << 31:
        rej("A \\(and one row more\\) must fit a 32-bit buffer range", k=big)
    row = int(good["k"] * unit)
    c_bytes, a_bytes, b_bytes = 128 * 96 * 2, 16 * row, 64 * 96 * row
    overlap = "C must not overlap A, B, plan, scale_a or scale_b"
    for c in (A, A + a_bytes - 16, A - c_bytes + 16, B + b_bytes - 16, B - c_bytes + 16, PLAN - c_bytes + 16,
              PLAN + 516 * 4 - 16):
        rej(overlap, c=c)
    if kind == "mxfp4":
        rej(overlap, c=SA + 16 * good["k"] // 32 - 16)
        rej(overlap, c=SB + 64 * 96 * good["k"] // 32 - 16)
    if kind == "fp8":
        rej(overlap, c=SA + 16 * 4 - 16, mode=gf.SCALE_ROW, sa=SA, sb=SB)
        rej(overlap, c=SB + 64 * 96 * 4 - 16, mode=gf.SCALE_ROW, sa=SA, sb=SB)


@pytest.mark.parametrize("kind", dc.KINDS)
def test_moe_gemm_launch_cfg_rejects_by_its_own_name(hip, kind):
    good = _gemm_good(kind)
    for cfg in (-1, 4, 99):
        with pytest.raises(hip.HipError, match="gsx_moe_gemm_nt_launch_cfg: unknown config"):
            _gemm_call(hip, kind, good, cfg=cfg)
    with pytest.raises(hip.HipError, match=f"gsx_moe_gemm_nt_launch_cfg: need N%32==0, K%{dc.BK[kind]}==0"):
        _gemm_call(hip, kind, {**good, "n": 48}, cfg=3)
    with pytest.raises(hip.HipError, match="gsx_moe_gemm_nt_launch_cfg: need 1 <= M <= 16"):
        _gemm_call(hip, kind, {**good, "m": 0}, cfg=0)


def test_moe_gemm_accepts_what_lies_next_to_a_refusal(hip):
    """M = 1 and 16, topk = E, a_div beyond P, and with fp8 scale_mode NONE scales that are not looked at: checked
    through the alignment of the plan, which is looked at later."""
    good = _gemm_good("fp8")
    for kw in ({"m": 1}, {"m": 16}, {"topk": 8, "e": 8}, {"e": 1}, {"a_div": 1}, {"a_div": 1000},
               {"sa": 3, "sb": 5}, {"n": 16}):
        kw = {"topk": 1, **kw} if kw.get("e") == 1 else kw
        with pytest.raises(hip.HipError, match="gsx_moe_gemm_nt: plan must be 4-B aligned"):
            _gemm_call(hip, "fp8", {**good, **kw, "plan": PLAN + 1})
    # the largest K whose 17 rows fit is taken as far as the overlap rule
    k = int(((1 << 32) - 1) / 17) // 128 * 128
    with pytest.raises(hip.HipError, match="gsx_moe_gemm_nt: C must not overlap"):
        _gemm_call(hip, "fp8", {**good, "k": k, "c": A})


COMBINE_GOOD = {"y": Y, "ys": 4104, "tw": TW, "out": OUT, "os": 4112, "m": 16, "topk": 8, "h": 4096}


def _combine_call(hip, v, timed=False):
    args = (_NoStream, v["y"], v["ys"], v["tw"], v["out"], v["os"], v["m"], v["topk"], v["h"])
    return hip.time_moe_combine(*args, 1) if timed else hip.moe_combine(*args)


@pytest.mark.parametrize("timed", [False, True], ids=["launch", "timed"])
def test_moe_combine_rejects_bad_arguments_by_name(hip, timed):
    def rej(text, **kw):
        with pytest.raises(hip.HipError, match=f"gsx_moe_combine: {text}"):
            _combine_call(hip, {**COMBINE_GOOD, **kw}, timed)

    for m in (0, 17):
        rej("need 1 <= M <= 16", m=m)
    for topk in (0, 9):
        rej("need 1 <= topk <= 8", topk=topk)
    for h in (0, 4, 12, 4092, -8):
        rej("need H >= 8 and H % 8 == 0", h=h)
    for ys in (4088, 4100):
        rej("need y_stride >= H and y_stride % 8 == 0", ys=ys)
    for os_ in (4088, 4100):
        rej("need out_stride >= H and out_stride % 8 == 0", os=os_)
    for name in ("y", "tw", "out"):
        rej("Y, topk_w and out must not be NULL", **{name: 0})
    for name in ("y", "out"):
        rej("Y and out must be 16-B aligned", **{name: COMBINE_GOOD[name] + 8})
    rej("topk_w must be 4-B aligned", tw=TW + 2)
    y_bytes, out_bytes = (127 * 4104 + 4096) * 2, (15 * 4112 + 4096) * 2
    for out in (Y, Y + y_bytes - 16, Y - out_bytes + 16, TW - out_bytes + 16, TW + 128 * 4 - 16):
        rej("out must not overlap Y or topk_w", out=out)


def test_moe_combine_accepts_what_lies_next_to_a_refusal(hip):
    for kw in ({"m": 1}, {"m": 16}, {"topk": 1}, {"h": 8, "ys": 8, "os": 8}, {"ys": 4096, "os": 4096}):
        with pytest.raises(hip.HipError, match="gsx_moe_combine: topk_w must be 4-B aligned"):
            _combine_call(hip, {**COMBINE_GOOD, **kw, "tw": TW + 1})


def test_unknown_kind_is_rejected_by_name(hip):
    L = hip.lib()
    for kind in (-1, 3):
        assert L.gsx_moe_gemm_nt(None, kind, A, 1, B, C, PLAN, 1, 1, 8, 16, 256, None, None, 0) != 0
        assert f"gsx_moe_gemm_nt: unknown kind {kind}" in L.gsx_last_error().decode()
    with pytest.raises(ValueError, match="decode kind 'fp4'"):
        _gemm_call(hip, "fp4", _gemm_good("bf16"))


# ---- the tools -------------------------------------------------------------------------------------------------------

def test_workload_and_isolation_parsers_take_the_moe_options():
    from gsxtools import isolation, workload

    for mod in (workload, isolation):
        ap = mod.build_parser()
        d = ap.parse_args(["--workload", "layer"])
        assert (d.experts, d.experts_active) == (0, 8)
        d = ap.parse_args(["--workload", "generate", "--experts", "128", "--experts-active", "4"])
        assert (d.experts, d.experts_active) == (128, 4)
        for bad in (["--workload", "layer", "--experts", "8"], ["--workload", "layer", "--experts", "24"],
                    ["--workload", "layer", "--experts", "2048"], ["--workload", "layer", "--experts", "-16"],
                    ["--workload", "layer", "--experts", "16", "--experts-active", "0"],
                    ["--workload", "layer", "--experts", "16", "--experts-active", "9"],
                    ["--workload", "server", "--experts", "16"], ["--workload", "decode", "--experts", "16"],
                    ["--workload", "prefill", "--context", "4096", "--experts", "16"]):
            with pytest.raises(SystemExit):
                ap.parse_args(bad)
    # the dense command line is what it was, byte for byte; the options are passed only when set
    iso = isolation.build_parser()
    dense = iso.parse_args(["--workload", "layer", "--kv-dtype", "fp8", "--kv-gib", "2", "--weights-gib", "1",
                            "--ffn", "1024"])
    assert isolation.layer_cmdline(dense) == ["--context", "8192", "--heads", "64", "--kv-heads", "8", "--kv-dtype",
                                              "fp8", "--page", "16", "--kv-gib", "2.0", "--weights-gib", "1.0", "--ffn",
                                              "1024"]
    assert "--experts" not in isolation.generate_cmdline(iso.parse_args(["--workload", "generate"]))
    moe = iso.parse_args(["--workload", "layer", "--experts", "128", "--experts-active", "8", "--heads", "16",
                          "--kv-heads", "4", "--ffn", "768"])
    line = isolation.layer_cmdline(moe)
    assert line[-4:] == ["--experts", "128", "--experts-active", "8"] and line[:-4] == isolation.dense_layer_cmdline(moe)
    got = workload.build_parser().parse_args(["--workload", "layer", *line])
    assert (got.experts, got.experts_active, got.heads, got.kv_heads, got.ffn) == (128, 8, 16, 4, 768)
    assert "--experts" in isolation.generate_cmdline(moe) and "--experts" not in isolation.prefill_cmdline(moe)


def test_moe_refusals_by_name_and_before_torch(monkeypatch):
    import builtins

    from gsxtools import workload as wl

    assert wl.moe_refusal("layer", 0, 8) is None and wl.moe_refusal("prefill", 0, 8) is None
    assert wl.moe_refusal("layer", 16, 8) is None and wl.moe_refusal("generate", 1024, 1) is None
    assert "--workload prefill --experts" in wl.moe_refusal("prefill", 16, 2)
    assert "--workload layer and generate only" in wl.moe_refusal("server", 16, 2)
    assert "a multiple of 16 in 16..1024" in wl.moe_refusal("layer", 8, 2)
    assert "--experts-active 9: 1..8" in wl.moe_refusal("layer", 16, 9)
    assert (wl.moe_active(16, 8), wl.moe_active(16, 2), wl.moe_active(1024, 8)) == (8, 2, 8)
    real = builtins.__import__

    def no_torch(name, *args, **kw):
        assert name != "torch", "torch was imported before the options were refused"
        return real(name, *args, **kw)

    monkeypatch.setattr(builtins, "__import__", no_torch)
    with pytest.raises(SystemExit, match="--workload prefill --experts"):
        wl.run(0, 0, workload="prefill", batch=1, chunk=128, context=256, experts=16)
    with pytest.raises(SystemExit, match="a multiple of 16"):
        wl.run(0, 0, workload="layer", experts=40)


def test_moe_layer_bytes_by_hand():
    from gsxtools import workload as wl

    # heads 2, kv_heads 1 (hidden 256), ffn 64, 16 experts: QKV [512][256], O [256][256], router [16][256],
    # 16 x (gate and up [128][256], down [256][64])
    assert wl.moe_layer_weight_bytes(2, 1, 64, 16) == (512 * 256 + 256 * 256 + 16 * 256 + 16 * 3 * 64 * 256) * 2
    # heads 16, kv_heads 4 (hidden 2048), ffn 768, 128 experts
    assert wl.moe_layer_weight_bytes(16, 4, 768, 128) == \
        ((16 + 8) * 128 * 2048 + 2048 * 2048 + 128 * 2048 + 128 * 3 * 768 * 2048) * 2
    assert wl.moe_expert_bytes(16, 768) == 3 * 768 * 2048 * 2
    assert wl.moe_layer_read_bytes(16, 4, 768, 128, 128) == wl.moe_layer_weight_bytes(16, 4, 768, 128)
    assert wl.moe_layer_read_bytes(2, 1, 64, 16, 5) == (512 * 256 + 256 * 256 + 16 * 256 + 5 * 3 * 64 * 256) * 2
    # the dense layer's function and its values are as they were
    assert wl.layer_weight_bytes(8, 2, 3584) == ((8 + 4) * 128 * 1024 + 1024 * 1024 + 3 * 3584 * 1024) * 2
