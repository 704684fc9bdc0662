"""The sampler's twin (``tests/sample_cases.py``) checked on the CPU: the polynomial, the weights' edges, the draw
frequencies against an fp64 softmax, and that each twin that is wrong on purpose is told from the right one by the cases
named for it, which ``tests/test_gpu_sample.py`` then runs on the kernel."""
import numpy as np
import pytest

from tests import sample_cases as sc

F32 = np.float32


def test_g_is_within_2_to_minus_20_of_two_to_the_f():
    """On a grid of 2^20 + 1 points of [0, 1) (every multiple of 2^-20, and the largest fp32 below 1) and at 10^6
    random points.  The bound is the issue's; the fit is within 2^-22.6."""
    rng = np.random.default_rng(0)
    grid = np.append(np.arange(2 ** 20, dtype=np.float64) / 2 ** 20, np.nextafter(F32(1), F32(0))).astype(F32)
    for f in (grid, rng.random(10 ** 6, dtype=F32)):
        assert float(f.min()) >= 0 and float(f.max()) < 1
        err = np.abs(sc.poly(f).astype(np.float64) - np.exp2(f.astype(np.float64)))
        print(f"max |g - 2^f| = 2^{np.log2(err.max()):.2f}")
        assert float(err.max()) <= 2.0 ** -20
    assert sc.poly(np.zeros(1, F32))[0] == 1


def test_weight_edges():
    c1 = sc.scale_c(sc.LOG2E)
    assert c1 == 1  # so x = d
    codes = sc.bf16_bits(np.array([0.0, -0.0, -1.0, -31.0, -32.0, -32.25, -33.0, -np.inf, np.nan], F32))
    w = sc.weights(codes, 0, c1)
    assert [int(x) for x in w] == [1 << 32, 1 << 32, 1 << 31, 2, 1, 0, 0, 0, 0]
    assert int(sc.weights(np.array([0xFFC1, 0x7F81], np.uint16), 0, c1).sum()) == 0  # NaNs with a payload
    # d = 0 against any finite maximum and any temperature
    for first in (0x4200, 0xC200, 0x0001, 0x7F7F, 0xFF7F, 0x8000):
        for t in (2.0 ** -20, 0.8, 1.0, 2.0 ** 20):
            assert int(sc.weights(np.array([first], np.uint16), first, sc.scale_c(t))[0]) == 1 << 32
    # the edge x = -32 with another c: the last live logit and the first dead one
    c = sc.scale_c(0.8)
    vals = sc.bf16_value(np.arange(0xC000, 0xC300, dtype=np.uint16))  # -2 .. -128
    x = (vals * c).astype(F32)
    w = sc.weights(np.arange(0xC000, 0xC300, dtype=np.uint16), 0, c)
    assert bool((w[x >= -32] >= 1).all()) and bool((w[x < -32] == 0).all()) and bool((x < -32).any())
    assert bool((np.diff(w.astype(np.int64)) <= 0).all())  # weights do not increase as the logit falls
    # the clamp of T
    assert sc.scale_c(2.0 ** -30) == sc.scale_c(2.0 ** -16) and sc.scale_c(2.0 ** 30) == sc.scale_c(2.0 ** 16)


def test_keys_order_the_codes():
    codes = np.arange(65536, dtype=np.uint16)
    key = sc.keys(codes)
    with np.errstate(invalid="ignore"):
        val = sc.bf16_value(codes).astype(np.float64)
    nan = np.isnan(val)
    assert bool((key[nan] == 0).all()) and int(key[~nan].min()) == 0x7F == int(key[sc.NEG_INF])
    assert int(key[sc.NEG_ZERO]) == int(key[0]) == 0x8000
    order = np.argsort(key[~nan], kind="stable")
    assert bool((np.diff(val[~nan][order]) >= 0).all())
    a, b = val[~nan][order][:-1], val[~nan][order][1:]
    assert bool(((np.diff(key[~nan][order]) > 0) == (a < b)).all())


PARAMETER_SETS = [(1.0, 0, 1.0), (0.7, 10, 1.0), (1.5, 0, 0.8), (0.8, 20, 0.9), (2.0, 8, 0.7)]


@pytest.mark.parametrize("t,k,p", PARAMETER_SETS)
def test_draw_frequencies_fit_the_softmax(t, k, p):
    """20,000 draws at V = 64 against softmax(l / T) cut by top-k and top-p in fp64.  Cells are pooled until each
    expects >= 5 draws.  Chi-square has mean dof and variance 2 dof; the bound is dof + 6 sqrt(2 dof) + 6, which a
    right sampler exceeds with a probability below 10^-5 at these dof (1 .. 63), and the seeds are fixed."""
    rng = np.random.default_rng(42)
    bits = sc.random_bits(rng, 64, 2.0)
    draws = 20000
    prep = sc.prepare(bits, t, k, p)
    seeds = sc.seeds_for(draws, 7)
    got = np.bincount([prep.draw(int(s), 3) for s in seeds], minlength=64)
    probs = sc.reference_probs(sc.bf16_value(bits), t, k, p)
    assert bool((got[probs == 0] == 0).all()), "a token outside the reference's support was drawn"
    order = np.argsort(-probs, kind="stable")
    cells_e, cells_o, e, o = [], [], 0.0, 0
    for i in order:
        e, o = e + probs[i] * draws, o + int(got[i])
        if e >= 5:
            cells_e.append(e)
            cells_o.append(o)
            e, o = 0.0, 0
    if e > 0:
        cells_e[-1] += e
        cells_o[-1] += o
    ce, co = np.array(cells_e), np.array(cells_o)
    dof = len(ce) - 1
    assert dof >= 1
    chi2 = float(((co - ce) ** 2 / ce).sum())
    print(f"T={t} k={k} p={p}: chi2 {chi2:.1f} at {dof} degrees of freedom")
    assert chi2 <= dof + 6 * np.sqrt(2 * dof) + 6


@pytest.mark.parametrize("flaw", sc.FLAWS)
def test_a_flawed_twin_is_told_apart(flaw):
    cases = sc.flaw_cases()[flaw]
    assert cases
    for case in cases:
        right, wrong = case.expected(), case.expected(flaw)
        assert not np.array_equal(right, wrong), f"{flaw}: {case.name} does not tell it from the right twin"


def test_every_case_gives_tokens_in_range():
    for case in sc.sample_cases() + [sc.grid_case(v, 3) for v in sc.GRID_V[:5]]:
        tok = case.expected()
        assert tok.shape == (case.m,) and bool(((tok >= 0) & (tok < case.v)).all()), case.name


def test_tie_and_edge_cases_are_what_they_say():
    # a top-k cut inside the tie group: S holds exactly its lowest members
    for case in sc.tie_cut_cases():
        prep = sc.prepare(case.bits, 2.0, int(case.top_k[0]), 1.0)
        group = np.flatnonzero(case.bits == 0x4000)
        want = np.sort(np.concatenate(([5, 40000], group[:max(0, int(case.top_k[0]) - 2)])))
        if int(case.top_k[0]) <= 2 + group.size:
            assert np.array_equal(prep.s_idx, want), case.name
    less, exact, more, ulps = sc.top_p_edge_cases()
    for case, groups in ((less, 1), (exact, 1), (more, 2)):
        prep = sc.prepare(case.bits, sc.LOG2E, 0, 0.5)
        assert prep.n_idx.size == groups and prep.zn == (1 << 32) + (groups - 1) * (1 << 31), case.name
    tok = ulps.expected()
    first = sc.prepare(ulps.bits, None, 0, 1.0).greedy
    assert bool((tok[0::3] == first).all()) and bool((tok[2::3] == first).all()) and bool((tok[1::3] != first).any())


def test_embed_reference_drops_tokens_out_of_range():
    table = np.arange(40, dtype=np.uint16).reshape(5, 8) + 1
    out = sc.embed_reference(table, np.array([4, -1, 5, sc.INT_MAX, 0], np.int32), 8)
    assert np.array_equal(out[0], table[4]) and np.array_equal(out[4], table[0]) and not out[1:4].any()
