"""``tests/attn_prefill_cases.py`` on the CPU: the twin of the contract lies inside the bound for every case the GPU runs,
the fp32 term of the bound stays below a quarter of the bf16 term, the exact cases are exact in the twin (and a twin
that masks or counts wrongly is not), the validation rules' edges, and the tools' options."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import attn_decode_cases as ac  # noqa: E402
from tests import attn_prefill_cases as pc  # noqa: E402


def _inside(p: pc.Problem, got: torch.Tensor, what: str):
    bound, ref, worst = pc.error_bound(p)
    err = np.abs(got.double().numpy() - ref)
    assert not np.isnan(err).any(), what
    over = err > bound
    assert not over.any(), f"{what}: {int(over.sum())} elements outside the bound, worst {float((err - bound).max())}"
    return worst


def test_the_shapes_come_from_the_table_and_cover_what_the_issue_lists():
    assert pc.T_VALUES == (1, 17, pc.Q_ROWS - 1, pc.Q_ROWS, pc.Q_ROWS + 1, 2 * pc.Q_ROWS + 1)
    assert pc.BASES == (0, 1, 15, 16, pc.KV_TILE - 1, pc.KV_TILE, 200)
    cases = pc.staircase_cases("bf16")
    assert {p.t for _, p in cases} == set(pc.T_VALUES)
    assert {p.page for _, p in cases} == set(pc.PAGES)
    for t in pc.T_VALUES:
        assert {b for _, p in cases if p.t == t for b in p.bases()} == set(pc.BASES), t
    assert {p.g for _, p in pc.random_cases("bf16")} == {1, 4, 16}
    assert {p.hkv for _, p in pc.random_cases("bf16")} == {1, 2}
    assert {p.b for _, p in pc.random_cases("bf16")} == {1, 3}
    for kind in pc.KINDS:
        for _, p in pc.all_cases(kind):
            ends = [x + n for x, n in zip(p.bases(), p.live())]
            assert max(ends) <= 720  # small: the whole GPU file runs in seconds
            assert kind == "bf16" or p.want is None or max(ends) <= 255  # e4m3 staircases are exact below 256 only
            # no table entry but the clamped one is out of range, and that one stays inside the allocation
            assert int(p.block_table.min()) >= 0 and int(p.block_table.max()) < p.k_cache.shape[0]


@pytest.mark.parametrize("kind", pc.KINDS)
def test_exact_cases_are_exact_in_the_twin(kind):
    for name, p in [*pc.staircase_cases(kind), *pc.dead_row_cases(kind)]:
        assert p.want is not None
        for tile in (pc.KV_TILE, 32) if p.t <= 17 else (pc.KV_TILE,):
            ac.assert_bits_equal(pc.twin(p, tile), p.want, f"{kind}, {name}, tile {tile}")
        # and the fp64 reference agrees
        assert np.array_equal(pc.reference(p), p.want.double().numpy()), name
        dead = [b * p.t + t for b, n in enumerate(p.live()) for t in range(n, p.t)]
        assert not p.want[dead].any()


@pytest.mark.parametrize("kind", pc.KINDS)
def test_a_wrong_mask_or_tile_fails_a_staircase(kind):
    name, p = next((n, q) for n, q in pc.staircase_cases(kind) if q.t == 17 and max(q.bases()) >= 64)
    for wrong in ("above", "no diagonal", "skip"):
        got = pc.twin(p, pc.KV_TILE, wrong)
        assert (ac.bits(got) != ac.bits(p.want)).any(), f"{kind}, {name}: {wrong} went unnoticed"


@pytest.mark.parametrize("kind", pc.KINDS)
def test_count_cases_lie_inside_the_bound_and_catch_a_miscount(kind):
    for name, p in pc.count_cases(kind):
        ref = pc.reference(p)
        # what the docstring says a count case computes
        for b, (base, n) in enumerate(zip(p.bases(), p.live())):
            for t in (0, n - 1):
                want = np.bincount(np.arange(base + t + 1) % pc.D, minlength=pc.D) / (base + t + 1) * p.v_scale
                assert np.allclose(ref[b * p.t + t], want[None, :], rtol=0, atol=1e-12)
        worst = _inside(p, pc.twin(p), f"{kind}, {name}")
        assert worst <= 1.0, (name, worst)
        bound = pc.error_bound(p)[0]
        for wrong in ("above", "no diagonal", "skip", "twice"):
            err = np.abs(pc.twin(p, pc.KV_TILE, wrong).double().numpy() - ref)
            assert (np.nan_to_num(err, nan=np.inf) > bound).any(), f"{kind}, {name}: {wrong} went unnoticed"


@pytest.mark.parametrize("kind", pc.KINDS)
def test_random_cases_lie_inside_the_bound(kind):
    for name, p in [*pc.random_cases(kind), *pc.t1_cases(kind)]:
        for tile in (pc.KV_TILE, 32):
            worst = _inside(p, pc.twin(p, tile), f"{kind}, {name}, tile {tile}")
        assert worst <= 1.0, f"{kind}, {name}: the fp32 term is {worst} of a quarter of the bf16 term"


@pytest.mark.parametrize("kind", pc.KINDS)
def test_t1_is_the_decode_problem(kind):
    for name, p in pc.t1_cases(kind):
        d = p.as_decode()
        assert d.lens() == [x + 1 for x in p.bases()]
        assert np.array_equal(ac.reference(d), pc.reference(p)), name
        # the decode bound counts the longest sequence's tokens for every sequence; this one each row's own
        theirs, mine = ac.error_bound(d)[0], pc.error_bound(p)[0]
        longest = int(np.argmax(p.bases()))
        assert (mine <= theirs * (1 + 1e-12)).all(), name
        assert np.allclose(theirs[longest], mine[longest], rtol=1e-12, atol=0), name


@pytest.mark.parametrize("kind", pc.KINDS)
def test_split_and_alone_views_are_the_same_rows(kind):
    _, p = next((n, q) for n, q in pc.random_cases(kind) if q.b == 3 and q.t > 1)
    whole = pc.reference(p).reshape(p.b, p.t, p.hq, pc.D)
    first, second = pc.split_chunk(p, 100)
    same = dict(rtol=1e-12, atol=1e-15)  # fp64 sums of other lengths: the last bits may differ
    assert np.allclose(pc.reference(first).reshape(p.b, 100, p.hq, pc.D), whole[:, :100], **same)
    assert np.allclose(pc.reference(second).reshape(p.b, p.t - 100, p.hq, pc.D), whole[:, 100:], **same)
    assert np.allclose(pc.reference(pc.alone(p, 1)), whole[1], **same)


@pytest.mark.parametrize("kind", pc.KINDS)
def test_chained_problem_from_the_appends_twin(kind):
    from tests import kv_append_cases as kc

    a = pc.chain_append_problem(kind)
    assert len(a.live()) == a.b * a.t
    r = kc.twin(a)
    p = pc.chained_problem(a, r.q_out, r.k[kc.GUARD:kc.GUARD + a.num_pages], r.v[kc.GUARD:kc.GUARD + a.num_pages])
    assert p.bases() == a.base() and p.live() == [a.t] * a.b
    worst = _inside(p, pc.twin(p), f"{kind}, chained")
    assert worst <= 1.0


def test_validation_edges():
    seen = set()
    for args, refusal in pc.edges():
        assert pc.validate(args) == refusal, (args, refusal)
        seen.add(refusal)
    # every rule has a refused edge, and an accepted one next to it
    rules = {"unknown kind 2", "need D == 128", "need 1 <= Hq <= 4096", "need Hq % Hkv == 0 and Hq / Hkv <= 16",
             "need page % 16 == 0 and 16 <= page <= 256", "need B >= 1 and T >= 1", "B * T must stay below 2^31",
             "ceil(T / 256) * B * Hq must stay below 2^31", "need num_pages >= 1", "need table_stride >= 1",
             "need max_seq_len >= 1", "need max_seq_len <= table_stride * page",
             "Q, K_cache, V_cache, O, block_table and seq_lens must not be NULL",
             "Q, K_cache, V_cache and O must be 16-B aligned", "block_table and seq_lens must be 4-B aligned",
             "O must not overlap Q", "scale, k_scale and v_scale must be finite and > 0",
             "a bf16 cache takes no scales: k_scale and v_scale must be 1.0", None}
    assert rules <= seen


# ---- the tools -------------------------------------------------------------------------------------------------------

def test_workload_and_isolation_parsers_take_the_prefill_workload():
    from gsxtools import isolation, workload

    for mod in (workload, isolation):
        ap = mod.build_parser()
        # --context is the length after the chunk here and has to be given; --chunk defaults to 2048
        d = ap.parse_args(["--workload", "prefill", "--context", "8192"])
        assert (d.workload, d.batch, d.chunk, d.context, d.heads, d.kv_heads, d.kv_dtype, d.page, d.ffn) == \
            ("prefill", 8, 2048, 8192, 64, 8, "bf16", 16, None)
        assert ap.parse_args(["--workload", "prefill", "--context=4096"]).context == 4096
        got = ap.parse_args(["--workload", "prefill", "--batch", "256", "--chunk", "128", "--context", "128"])
        assert (got.batch, got.chunk, got.context) == (256, 128, 128)
        for bad in (["--batch", "3", "--chunk", "100", "--context", "256"],  # 300 rows: no multiple of 128
                    ["--batch", "2", "--chunk", "512", "--context", "256"],  # the chunk is longer than the context
                    ["--batch", "0", "--context", "8192"], ["--batch", "257", "--chunk", "128", "--context", "8192"],
                    ["--chunk", "0", "--context", "8192"], ["--chunk", "128"]):  # the last: no --context
            with pytest.raises(SystemExit):
                ap.parse_args(["--workload", "prefill", *bad])
        # the other workloads' ranges are what they were
        with pytest.raises(SystemExit):
            ap.parse_args(["--workload", "layer", "--batch", "17"])
    a = isolation.build_parser().parse_args(["--workload", "prefill", "--chunk", "256", "--batch", "2", "--ffn", "1024",
                                             "--context", "8192"])
    got = workload.build_parser().parse_args(["--workload", "prefill", "--batch", "2", *isolation.prefill_cmdline(a)])
    assert (got.chunk, got.ffn, got.context) == (256, 1024, 8192)
    assert {"prefill-noisy", "prefill-noisy-partitioned"} <= set(isolation.SCENARIOS)
    with pytest.raises(SystemExit, match="--workload prefill: scenario noisy is not one of"):
        isolation.main(["--workload", "prefill", "--context", "8192", "--scenarios", "noisy"])
    with pytest.raises(SystemExit, match="prefill-noisy: --batch 1 x --chunk 100 = 100 rows"):
        isolation.main(["--scenarios", "prefill-noisy", "--chunk", "100", "--prefill-batch", "1"])


def test_prefill_workload_refuses_before_it_loads_torch(monkeypatch):
    """``run`` itself, called without the parser, refuses the same sizes before ``import torch``."""
    import builtins

    from gsxtools import workload

    real = builtins.__import__

    def no_torch(name, *args, **kw):
        assert name != "torch", "torch was imported before the sizes were refused"
        return real(name, *args, **kw)

    monkeypatch.setattr(builtins, "__import__", no_torch)
    with pytest.raises(SystemExit, match="multiple of 128"):
        workload.run(0, 0, workload="prefill", batch=3, chunk=100, context=256)
    with pytest.raises(SystemExit, match="more than --context"):
        workload.run(0, 0, workload="prefill", batch=2, chunk=512, context=256)


def test_prefill_workload_sizes():
    from gsxtools import workload as wl

    assert wl.prefill_refusal(2, 128, 256) is None and wl.prefill_refusal(1, 128, 128) is None
    # rows at positions context - chunk .. context - 1 see pos + 1 tokens each
    assert wl.prefill_visible_pairs(1, 4, 4) == 1 + 2 + 3 + 4
    assert wl.prefill_visible_pairs(3, 2, 10) == 3 * (9 + 10)
    assert wl.prefill_visible_pairs(16, 2048, 2048) == 16 * 2048 * 2049 // 2


def test_isolation_summary_with_solo_figures():
    from gsxtools import isolation

    s = isolation.with_solo(isolation.summarize("prefill-noisy", [{"tflops": 10.0, "tbps": 2.0}, {"tflops": 300.0}]),
                            [{"tflops": 20.0}, {"tflops": 400.0}])
    assert s["solo_tflops"] == [20.0, 400.0] and s["ratio_to_solo"] == [0.5, 0.75]
