"""What the MoE prefill entry points (native/kernels/moe_prefill.hip) refuse, by rule text and before the first device
call, the size of the tile plan, and the tools' handling of ``--workload prefill-moe``.  No GPU."""
import pytest

torch = pytest.importorskip("torch")

# Addresses that are never dereferenced: every call below is refused before the first device call.
LG, IDS, TW, PLAN, WS, A, B, C, Y, OUT = (0x10000000 * i for i in range(1, 11))
GOOD = {"route": dict(lg=LG, ls=136, ids=IDS, tw=TW, m=300, e=128, topk=8),
        "plan": dict(ids=IDS, plan=PLAN, m=300, topk=8, e=128, ws=WS, wsb=1 << 20),
        "gemm_nt": dict(a=A, a_div=8, b=B, c=C, plan=PLAN, m=300, topk=8, e=128, n=256, k=192),
        "combine": dict(y=Y, ys=264, tw=TW, out=OUT, os=264, m=300, topk=8, h=264)}
# the last rule before the overlaps: a call that gets this far was accepted by every rule in front of it
LATE = {"route": (dict(lg=LG + 8), "logits must be 16-B aligned"),
        "plan": (dict(ws=WS + 2), "topk_ids, plan and workspace must be 4-B aligned"),
        "gemm_nt": (dict(plan=PLAN + 2), "plan must be 4-B aligned"),
        "combine": (dict(tw=TW + 2), "topk_w must be 4-B aligned")}
M_RULE, E_RULE, K_RULE = "need 1 <= M <= 32768", "need 8 <= E <= 1024 and E % 8 == 0", r"need 1 <= topk <= min\(8, E\)"
SIZES = [(dict(m=0), M_RULE, dict(m=1)), (dict(m=32769), M_RULE, dict(m=32768)), (dict(e=4), E_RULE, dict(e=8)),
         (dict(e=1032), E_RULE, dict(e=1024)), (dict(e=132), E_RULE, None), (dict(topk=0), K_RULE, dict(topk=1)),
         (dict(topk=9), K_RULE, None)]
WIDE = {"route": dict(ls=2048)}  # a stride that every E fits
# (entry point, what is wrong, the rule's text, the accepted neighbour)
REFUSALS = [(ep, {**WIDE.get(ep, {}), **bad}, text, near and {**WIDE.get(ep, {}), **near})
            for ep in ("route", "plan", "gemm_nt") for bad, text, near in SIZES] + [
    ("route", dict(ls=120), "need logits_stride >= E and logits_stride % 8 == 0", dict(ls=128)),
    ("route", dict(ls=132), "need logits_stride >= E and logits_stride % 8 == 0", None),
    ("route", dict(ids=0), "logits, topk_ids and topk_w must not be NULL", None),
    ("route", dict(tw=TW + 2), "topk_ids and topk_w must be 4-B aligned", None),
    ("route", dict(ids=LG + (299 * 136 + 128) * 2 - 4), "topk_ids and topk_w must not overlap logits or each other",
     None),
    ("route", dict(tw=IDS + 2400 * 4 - 4), "topk_ids and topk_w must not overlap logits or each other", None),
    ("plan", dict(ws=0), "topk_ids, plan and workspace must not be NULL", None),
    ("plan", dict(wsb=3 * 128 * 4 - 1), "workspace too small: need 1536 bytes", dict(wsb=1536)),
    ("plan", dict(ws=PLAN + (4 + 129 * 145) * 4 - 4), "plan and workspace must not overlap topk_ids or each other", None),
    ("gemm_nt", dict(a_div=0), "need a_div >= 1", dict(a_div=1)),
    ("gemm_nt", dict(n=192), "need N%128==0, K%64==0", dict(n=128)),
    ("gemm_nt", dict(k=96), "need N%128==0, K%64==0", dict(k=64)),
    ("gemm_nt", dict(b=0), "A, B, C and plan must not be NULL", None),
    ("gemm_nt", dict(c=C + 8), "operands must be 16-B aligned", None),
    ("gemm_nt", dict(k=1 << 25), "K too large: 128 rows of K elements must stay below 2\\^31", None),
    ("gemm_nt", dict(c=PLAN + 16), "C must not overlap A, B or plan", None),
    ("combine", dict(m=0), M_RULE, dict(m=1)), ("combine", dict(m=32769), M_RULE, dict(m=32768)),
    ("combine", dict(topk=9), "need 1 <= topk <= 8", dict(topk=8)),
    ("combine", dict(h=12), "need H >= 8 and H % 8 == 0", dict(h=8)),
    ("combine", dict(ys=256), "need y_stride >= H and y_stride % 8 == 0", None),
    ("combine", dict(os=268), "need out_stride >= H and out_stride % 8 == 0", None),
    ("combine", dict(out=0), "Y, topk_w and out must not be NULL", None),
    ("combine", dict(y=Y + 8), "Y and out must be 16-B aligned", None),
    ("combine", dict(out=TW + 16), "out must not overlap Y or topk_w", None)]


class _NoStream:
    """Stands in for ``hip.Stream``: the calls under test never get as far as using one."""
    handle = None


@pytest.fixture(scope="module")
def hip():
    from gpushare_scheduler_extender_amd.ops import hip as h

    h.lib()
    return h


def _call(hip, ep, v, timed):
    order = {"route": "lg ls ids tw m e topk", "plan": "ids plan m topk e ws wsb",
             "gemm_nt": "a a_div b c plan m topk e n k", "combine": "y ys tw out os m topk h"}[ep]
    args = (_NoStream, *(v[name] for name in order.split()))
    name = "moe_prefill_gemm" if timed and ep == "gemm_nt" else f"moe_prefill_{ep}"
    return getattr(hip, "time_" + name)(*args, 1) if timed else getattr(hip, name)(*args)


@pytest.mark.parametrize("ep,bad,text,near", REFUSALS, ids=[f"{r[0]}-{i}" for i, r in enumerate(REFUSALS)])
def test_entry_points_refuse_by_rule_text_and_take_the_neighbour(hip, ep, bad, text, near):
    for timed in (False, True):
        with pytest.raises(hip.HipError, match=f"gsx_moe_prefill_{ep}: {text}"):
            _call(hip, ep, {**GOOD[ep], **bad}, timed)
    if near is not None:
        late, late_text = LATE[ep]
        with pytest.raises(hip.HipError, match=f"gsx_moe_prefill_{ep}: {late_text}"):
            _call(hip, ep, {**GOOD[ep], **near, **late}, False)


def test_launch_cfg_refuses_under_its_own_name(hip):
    v = GOOD["gemm_nt"]
    args = (_NoStream, v["a"], v["a_div"], v["b"], v["c"], v["plan"], v["m"], v["topk"], v["e"], v["n"])
    with pytest.raises(hip.HipError, match="gsx_moe_prefill_gemm_nt_launch_cfg: unknown config"):
        hip.moe_prefill_gemm_nt_cfg(*args, v["k"], 1)
    with pytest.raises(hip.HipError, match="gsx_moe_prefill_gemm_nt_launch_cfg: need N%128==0, K%64==0"):
        hip.moe_prefill_gemm_nt_cfg(*args, 100, 0)


@pytest.mark.parametrize("m,topk,e", [(2, 2, 8), (4, 2, 8), (32768, 8, 1024)], ids=["P<E", "P=E", "P=32768*8"])
def test_plan_ints_is_the_formula(hip, m, topk, e):
    p = m * topk
    t_max = (p + min(e, p) * 127) // 128
    assert hip.moe_prefill_plan_ints(m, topk, e) == 4 + t_max + 128 * t_max
    assert hip.moe_prefill_workspace_bytes(m, topk, e) == -(-p // 1024) * e * 4
    with pytest.raises(hip.HipError, match=f"gsx_moe_prefill_plan_ints: {M_RULE}"):
        hip.moe_prefill_plan_ints(0, topk, e)


def test_parsers_and_refusals_of_prefill_moe():
    from gsxtools import isolation, workload as wl

    ap = wl.build_parser()
    ok = ["--workload", "prefill-moe", "--context", "256", "--chunk", "128", "--batch", "1"]
    d = ap.parse_args([*ok, "--experts", "256", "--experts-active", "4"])
    assert (d.workload, d.experts, d.experts_active) == ("prefill-moe", 256, 4)
    for bad in (ok, [*ok, "--experts", "64"], [*ok, "--experts", "192"], [*ok, "--experts", "2048"],
                [*ok, "--experts", "128", "--experts-active", "9"], [*ok[:2], *ok[4:], "--experts", "128"],
                [*ok[:4], "--chunk", "100", "--experts", "128"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    with pytest.raises(SystemExit):  # the isolation harness has no such pod
        isolation.build_parser().parse_args(["--workload", "prefill-moe", "--experts", "128"])
    assert wl.moe_refusal("prefill-moe", 128, 8) is None and wl.moe_refusal("prefill-moe", 1024, 1) is None
    assert "a multiple of 128 in 128..1024" in wl.moe_refusal("prefill-moe", 0, 8)
    assert "a multiple of 128 in 128..1024" in wl.moe_refusal("prefill-moe", 16, 8)
    assert "--experts-active 0: 1..8" in wl.moe_refusal("prefill-moe", 128, 0)
    # the dense prefill workload still has no experts, under the text it had
    assert wl.moe_refusal("prefill", 128, 2) == ("--workload prefill --experts: more than 16 rows needs a grouped large "
                                                 "GEMM, which there is none of")
    for mod in (wl, isolation):
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(["--workload", "prefill", "--context", "4096", "--experts", "128"])
    with pytest.raises(SystemExit, match="--workload prefill --experts"):
        wl.run(0, 0, workload="prefill", batch=1, chunk=128, context=256, experts=128)
