"""CPU checks for the decode attention (native/kernels/attn_decode.hip): the selection cases of
``tests/attn_decode_cases.py`` against the fp64 reference and the NumPy twin of the numeric contract, the window cases
likewise and against twins that count a token twice or not at all, the random cases' bound, the dispatcher's rule
against the library's workspace query, the configuration table, every argument the entry points refuse, the tools'
parsers and the size of the workload's KV ring.  No GPU: the refused calls never reach the device."""
import dataclasses
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import attn_decode_cases as ac  # noqa: E402


@pytest.fixture(scope="module")
def hip():
    from gpushare_scheduler_extender_amd.ops import hip as h

    h.lib()
    assert hasattr(h, "decode_attn_cfgs"), "the bindings have no decode attention"
    return h


# ---- the cases -------------------------------------------------------------------------------------------------------

def _exact(name, p, tiles=(16, 32)):
    """The fp64 reference rounded to bf16, and the fp32 twin at each tile size, return the target rows exactly."""
    assert p.want is not None and not bool(torch.isnan(p.want).any())
    ac.assert_bits_equal(ac.to_bf16(ac.reference(p)), p.want, f"{name}: the fp64 reference")
    for tile in tiles:
        ac.assert_bits_equal(ac.twin(p, tile), p.want, f"{name}: the twin at tile {tile}")


def test_walsh_rows_are_orthogonal_and_v_rows_tell_slots_apart():
    w = ac.walsh()
    assert w.shape == (128, 128) and set(np.unique(w)) == {-1.0, 1.0}
    assert np.array_equal(w @ w.T, 128 * np.eye(128, dtype=np.float32))
    pp, h, slot = np.meshgrid(np.arange(40), np.arange(2), np.arange(16), indexing="ij")
    rows = ac.v_rows(pp.ravel(), h.ravel(), slot.ravel(), 16, 2)
    assert rows.min() >= 1 and rows.max() <= 15 and len(np.unique(rows, axis=0)) == 40 * 2 * 16
    # every value is exact in e4m3 as it is in bf16
    assert torch.equal(torch.from_numpy(rows).to(ac.FP8).float(), torch.from_numpy(rows))


@pytest.mark.parametrize("kind", ac.KINDS)
def test_selection_cases_short_and_tables_are_exact(kind):
    cases = ac.short_cases(kind) + ac.table_cases(kind)
    assert {p.g for _, p in cases} == {1, 2, 4, 8, 16} and {p.page for _, p in cases} == {16, 64}
    assert {n for _, p in ac.short_cases(kind) for n in p.lens()} == set(ac.SHORT_LENS)
    for name, p in cases:
        _exact(f"{kind}, {name}", p)
        # poison: every slot no sequence owns holds NaN in V, and every unused table entry names such a page
        owned = torch.zeros(p.num_pages, p.page, dtype=torch.bool)
        for b, n in enumerate(p.lens()):
            t = torch.arange(n)
            owned[p.block_table[b][t // p.page].long(), t % p.page] = True
            spare = p.block_table[b][-(-n // p.page):].long()
            assert bool((spare >= 0).all()) and bool((spare < p.num_pages).all())
            assert not bool(owned[spare].any()) or name == "shared"
        v = p.v_cache.float().permute(0, 2, 1, 3)  # [page][slot][head][d]
        assert bool(torch.isnan(v[~owned]).all()) and not bool(torch.isnan(v[owned]).any())


def test_clamped_case_has_lengths_above_max_seq_len():
    p = dict(ac.table_cases("bf16"))["clamped"]
    assert [int(x) > p.max_seq_len for x in p.seq_lens] == [True, False, True] and p.lens() == [75, 20, 75]
    q = dict(ac.table_cases("bf16"))["stride + 5"]
    assert q.table_stride == -(-q.max_seq_len // q.page) + 5


@pytest.mark.parametrize("cfg", ac.ALL, ids=lambda c: "dispatch" if c is None else str(c))
@pytest.mark.parametrize("kind", ac.KINDS)
def test_selection_cases_of_the_splits_are_exact(kind, cfg):
    """Every length of ``split_lengths`` for every split count.  Read back from ``want``, the targets of every
    sequence hold its first token, its last token and both sides of every cut of every split count of ``SPLITS``
    (the case's own among them), and otherwise half, tile and page boundaries that reach into the last quarter of
    the sequence.  The twin at the kernel's tile (and, at one split, at tile 16 as well)."""
    _, w, f = ac.CFGS[ac.DISPATCHED if cfg is None else cfg]
    for splits in ac.SPLITS:
        lens = ac.split_lengths(cfg, splits)
        per_split = {-(-(-(-n // ac.TILE)) // splits) for n in lens}
        assert {1, w - 1, w + 1, f * w + 1, 2 * f * w, 2 * f * w + 1} <= per_split  # a tile short, ragged, steady
        if splits > 1:
            assert any(-(-n // ac.TILE) < splits for n in lens)  # a split without a token
            assert any(n - c == 1 for n in lens for c in ac.split_cuts(n, splits)[-1:])  # a last split of one token
        for name, p in ac.split_cases(kind, cfg, splits):
            hit = ac.targets(p)
            for b, n in enumerate(p.lens()):
                got, cuts = set(hit[b]), ac.all_cuts(n)
                assert set(ac.split_cuts(n, splits)) <= set(cuts)
                assert {0, n - 1} <= got and all({c - 1, c} <= got for c in cuts), (name, b, splits, sorted(got))
                assert got <= set(ac.boundary_tokens(n, 16, cuts))
                if n >= 256:  # the heads left over are spread over the whole length
                    other = got - {0, n - 1} - {t for c in cuts for t in (c - 1, c)}
                    assert min(other) < n // 4 and max(other) >= n - n // 4, (name, b, sorted(other))
            _exact(f"{kind} cfg {cfg} splits {splits}, {name}", p, (16, 32) if splits == 1 else (32,))


@pytest.mark.parametrize("kind", ac.KINDS)
def test_targets_visit_every_boundary(kind):
    """G = 16 and Hkv = 2 are 32 targets per sequence: more than a sequence of 70 tokens has boundaries, so every
    sequence visits them all, and each of its two KV heads has targets in the first and the last tile, left and right
    of a boundary.  With one head per KV head, sequences of one length visit everything between them."""
    n = 70
    p = ac.selection_problem(kind, 16, 16, [n] * 2, **ac.fp8_scales(kind))
    marks = ac.boundary_tokens(n, 16)
    assert marks == [0, 15, 16, 31, 32, 47, 48, 63, 64, 69]
    hit = ac.targets(p)  # read back from the result: the row of V a head got names its slot
    assert set(hit[0]) == set(marks) and set(hit[1]) == set(marks) and hit[0] != hit[1]
    for kv in range(2):
        mine = set(hit[0][kv * 16:(kv + 1) * 16])
        assert min(mine) < 32 and max(mine) >= n - 32 and {t % 16 for t in mine} >= {0, 15}, sorted(mine)
    few = ac.selection_problem(kind, 1, 16, [n] * 5, **ac.fp8_scales(kind))
    assert {t for row in ac.targets(few) for t in row} == set(marks)


def _windows(p, b):
    """``inside[Hkv][G][n]``: the tokens of sequence b that score a head's maximum, read back from Q and the K cache."""
    k, _ = p.gather(b, scaled=False)
    q = p.q.to(torch.float64).numpy().reshape(p.b, p.hkv, p.g, ac.D)[b]
    x = np.einsum("hgd,htd->hgt", q, k)
    return x == x.max(axis=2, keepdims=True), x


def _windows_cover(name, p, split_counts, negative=False):
    """Read back from the caches: every head's window is one run of s tokens (s a power of two, the same for the
    heads of a sequence), all other tokens score 2048 less, the windows of every KV head cover the sequence, and
    both sides of every cut of every split count in ``split_counts`` lie in one window."""
    for b, n in enumerate(p.lens()):
        if n == 0:
            continue
        inside, x = _windows(p, b)
        s = int(inside[0, 0].sum())
        assert s & (s - 1) == 0 and s == ac.window_spans(n, p.g)[0] and bool((inside.sum(axis=2) == s).all()), (name, b)
        top = -2048 if negative else 2048
        assert set(np.unique(x)) <= {top, top - 2048}, (name, b, np.unique(x))
        for h in range(p.hkv):
            for g in range(p.g):
                (where,) = np.nonzero(inside[h, g])
                assert where[-1] - where[0] == s - 1, (name, b, h, g)
            assert bool(inside[h].any(axis=0).all()), f"{name}: sequence {b}, KV head {h}: a token that no head counts"
            for splits in split_counts:
                for cut in ac.split_cuts(n, splits):
                    assert bool((inside[h, :, cut - 1] & inside[h, :, cut]).any()), (name, b, h, splits, cut)


@pytest.mark.parametrize("cfg", ac.ALL, ids=lambda c: "dispatch" if c is None else str(c))
@pytest.mark.parametrize("kind", ac.KINDS)
def test_window_cases_of_the_splits_are_exact(kind, cfg):
    """The lengths of ``split_lengths`` as window cases: exact, the windows cover, every cut lies inside a window."""
    for splits in ac.SPLITS:
        for name, p in ac.window_split_cases(kind, cfg, splits):
            assert p.g == 16 and p.hkv == 2
            _windows_cover(f"{kind} cfg {cfg} splits {splits}, {name}", p, (splits,))
            _exact(f"{kind} cfg {cfg} splits {splits}, {name}", p, (16, 32) if splits == 1 else (32,))
        assert sorted(n for _, p in ac.window_split_cases(kind, cfg, splits) for n in p.lens()) == \
            ac.split_lengths(cfg, splits)


@pytest.mark.parametrize("kind", ac.KINDS)
def test_window_cases_with_negative_scores_and_of_other_shapes_are_exact(kind):
    """The variant whose scores are all far below zero, and ``OTHER_SHAPES`` as window and as selection cases."""
    for name, p in ac.negative_cases(kind):
        assert p.g == 8
        for b in range(p.b):
            assert _windows(p, b)[1].max() == -2048  # -261.2 in the exp2 argument; the others -522.4
        _windows_cover(f"{kind}, {name}", p, ac.SPLITS, negative=True)
        _exact(f"{kind}, {name}", p)
    cases = ac.other_shape_cases(kind)
    assert {p.hkv for _, p in cases} == {1, 3, 8} and {p.page for _, p in cases} == {32, 48, 128, 256}
    assert {p.g for _, p in cases} == {3, 7, 12}
    for name, p in cases:
        if name.startswith("windows"):
            _windows_cover(f"{kind}, {name}", p, ac.SPLITS)
        _exact(f"{kind}, {name}", p)


MISCOUNT_LENGTHS = ((1, 2, 17, 33, 100), (129, 600, 2033), (4785,), (8433,))


@pytest.mark.parametrize("kind", ac.KINDS)
def test_a_miscounted_token_changes_a_window_case(kind):
    """Why the window cases exist.  A twin that takes a tile twice or leaves one out (first, middle, last), leaves out
    a 16-token half or a single token, or takes a token twice, changes the result of every sequence of more than one
    tile, at the lengths where the ring's steady loop and drain run among them."""
    seen = set()
    for lens in MISCOUNT_LENGTHS:
        p = ac.window_problem(kind, 16, 16, lens, **ac.fp8_scales(kind))
        _exact(f"{kind}, lengths {lens}", p)
        many = [b for b, n in enumerate(lens) if n > ac.TILE]
        for what in ac.miscounts(max(lens)):
            got = ac.twin(p, ranges=lambda b, n: ac.miscounts(n).get(what, ac.tile_ranges(n)))  # noqa: B023
            for b in range(p.b):
                same = torch.equal(ac.bits(got[b]), ac.bits(p.want[b]))
                assert same == (b not in many), f"{kind}, {lens[b]} tokens, {what}: " + ("unseen" if same else "seen")
            seen.add(what)
    assert len(seen) == 9, seen


def test_a_miscounted_tile_leaves_a_selection_case_as_it_is():
    """The same twins on ``split_cases``: a tile taken twice changes nothing (l = 2, acc = 2 v), and neither does a
    tile left out that holds no target.  The selection cases test addressing, not counting."""
    doubled = dropped = 0
    for splits in (1, 3):
        for name, p in ac.split_cases("bf16", 2, splits):
            hit = ac.targets(p)

            def free(n, b):  # the ranges without the first tile that holds no target, if there is one
                base = ac.tile_ranges(n)
                for i, (t0, t1) in enumerate(base):
                    if not any(t0 <= t < t1 for t in hit[b]):
                        return base[:i] + base[i + 1:]
                return base

            for what in ("the first tile twice", "the middle tile twice", "the last tile twice"):
                got = ac.twin(p, ranges=lambda b, n: ac.miscounts(n).get(what, ac.tile_ranges(n)))  # noqa: B023
                ac.assert_bits_equal(got, p.want, f"splits {splits}, {name}, {what}")
                doubled += sum(n > ac.TILE for n in p.lens())
            got = ac.twin(p, ranges=lambda b, n: free(n, b))
            ac.assert_bits_equal(got, p.want, f"splits {splits}, {name}, a tile without a target left out")
            dropped += sum(len(free(n, b)) < len(ac.tile_ranges(n)) for b, n in enumerate(p.lens()))
    assert doubled >= 25 and dropped >= 4, (doubled, dropped)


@pytest.mark.parametrize("cfg", list(ac.CFGS))
@pytest.mark.parametrize("kind", ac.KINDS)
def test_window_cases_of_more_splits_are_exact(kind, cfg):
    """16, 32, 37 and 64 splits: per split 1, W + 1 and 2 F W + 1 tiles, a split without a token, a last split of one
    token and one of a full tile.  The twin at tile 16 as well where the sequences are short."""
    _, w, f = ac.CFGS[cfg]
    for splits in ac.MORE_SPLITS:
        lens = ac.more_split_lengths(cfg, splits)
        assert {-(-(-(-n // ac.TILE)) // splits) for n in lens} >= {1, 3, w + 1, 2 * f * w + 1}
        assert any(-(-n // ac.TILE) < splits for n in lens)  # a split without a token
        assert any(n - ac.split_cuts(n, splits)[-1] == 1 for n in lens)  # a last split of one token
        assert any(n - ac.split_cuts(n, splits)[-1] == ac.TILE and len(ac.split_cuts(n, splits)) == splits - 1
                   for n in lens)  # and of one full tile
        cases = ac.more_split_cases(kind, cfg, splits)
        assert sorted(n for _, p in cases for n in p.lens()) == lens
        for name, p in cases:
            assert max(p.k_cache.numel(), p.v_cache.numel()) * 4 <= 70 << 20 and (p.b == 1 or max(p.lens()) <= ac.LONG)
            _windows_cover(f"{kind} cfg {cfg} splits {splits}, {name}", p, (splits,))
            _exact(f"{kind} cfg {cfg} splits {splits}, {name}", p, (16, 32) if max(p.lens()) <= ac.LONG else (32,))


@pytest.mark.parametrize("shape", ac.DISPATCH_SHAPES, ids=[s[0] for s in ac.DISPATCH_SHAPES])
def test_dispatch_cases_are_exact(shape):
    """The rows of ``DISPATCH_SHAPES``: ``pick()`` gives the split count the row names, the window case covers and has
    every cut of that count inside a window, the selection case has targets on both sides of every such cut, and
    both are exact for both cache types (the e4m3 ones are the bf16 ones stored as e4m3)."""
    name, hkv, g, page, lens, max_seq_len, splits = shape
    assert ac.pick(len(lens) * hkv, max_seq_len) == splits and max(lens) == max_seq_len - 15
    cases = ac.dispatch_cases(shape)
    for kind in ac.KINDS:
        (_, win), (_, sel) = cases[kind]
        assert win.kind == sel.kind == kind and win.max_seq_len == sel.max_seq_len == max_seq_len
        for p in (win, sel):
            assert (p.hkv, p.g, p.page, p.lens()) == (hkv, g, page, list(lens))
        _exact(f"{kind}, windows, {name}", win, (32,))
        _exact(f"{kind}, selection, {name}", sel, (32,))
    _windows_cover(name, cases["bf16"][0][1], (splits,))
    sel = cases["bf16"][1][1]
    hit = ac.targets(sel)
    for b, n in enumerate(lens):
        cuts = ac.split_cuts(n, splits)
        sides = {t for c in cuts for t in (c - 1, c)}
        if g * hkv >= 2 * splits:  # enough heads for both sides of every cut
            assert sides <= set(hit[b]), (name, b)
        elif n == max(lens):  # otherwise every head of the long sequence, but two at most, sits at a cut
            assert len(sides & set(hit[b])) >= g * hkv - 2, (name, b, sorted(hit[b]))


def test_an_exact_case_stored_as_e4m3_is_the_builders():
    for build in (lambda kind, fs: ac.window_problem(kind, 8, 32, [100, 0, 33], hkv=3, **fs),
                  lambda kind, fs: ac.selection_problem(kind, 8, 32, [100, 0, 33], hkv=3, **fs)):
        a, b = ac.to_fp8(build("bf16", {})), build("fp8", ac.fp8_scales("fp8"))
        assert (a.kind, a.scale, a.k_scale, a.v_scale, a.max_seq_len) == (b.kind, b.scale, b.k_scale, b.v_scale,
                                                                          b.max_seq_len)
        for x, y in ((a.k_cache, b.k_cache), (a.v_cache, b.v_cache)):  # NaN where NaN is (its sign is free), else the byte
            nan = torch.isnan(x.float())
            assert x.dtype == y.dtype == ac.FP8 and torch.equal(nan, torch.isnan(y.float()))
            assert torch.equal(x.view(torch.uint8)[~nan], y.view(torch.uint8)[~nan])
        assert torch.equal(a.block_table, b.block_table) and torch.equal(ac.bits(a.want), ac.bits(b.want))


@pytest.mark.parametrize("kind", ac.KINDS)
def test_clamp_cases_are_exact(kind):
    """``seq_lens`` below zero, and a page index at or above ``num_pages``."""
    p = dict(ac.table_cases(kind))["negative"]
    assert [int(x) for x in p.seq_lens] == [-1, 90, -2 ** 31] and p.lens() == [0, 90, 0]
    assert not p.want[0].any() and not p.want[2].any() and bool(p.want[1].any())
    c = ac.page_clamp_problem(kind)
    assert c.k_cache.shape[0] == c.v_cache.shape[0] == c.num_pages + 3
    over = (c.block_table >= c.num_pages).nonzero()
    assert over.tolist() == [[0, 3]] and int(c.block_table[0, 3]) == c.num_pages + 1 and c.lens()[0] > 4 * c.page
    assert bool(torch.isnan(c.v_cache[c.num_pages:].float()).all())  # poison beyond num_pages
    assert not bool(torch.isnan(c.v_cache[c.num_pages - 1].float()).any())  # the page the clamp lands on is in use
    _exact(f"{kind}, page index above num_pages", c)
    # without the clamp the entry names a poison page inside the allocation, and the result is another
    unclamped = ac.twin(dataclasses.replace(c, beyond=0))
    assert not torch.equal(ac.bits(unclamped[0]), ac.bits(c.want[0])) and bool(torch.isnan(unclamped[0]).any())
    assert torch.equal(ac.bits(unclamped[1:]), ac.bits(c.want[1:]))


def test_fp8_codes_case_holds_every_code_at_every_byte_position():
    p, codes = ac.fp8_codes_problem()
    assert codes.shape == (32, 128) and p.kind == "fp8" and (p.g, p.hkv) == (16, 2)
    finite = sorted(set(range(256)) - {0x7F, 0xFF})
    for pos in range(16):
        assert sorted(set(codes[:, pos::16].ravel().tolist())) == finite, pos
    # the value of a code, from the format: sign, 4 bits of exponent with bias 7, 3 of mantissa; exponent 0 is subnormal
    c = codes.astype(np.int64)
    e, m = (c >> 3) & 15, c & 7
    value = np.where(e == 0, m / 8 * 2.0 ** -6, (1 + m / 8) * 2.0 ** (e - 7)) * np.where(c & 128, -1.0, 1.0)
    assert np.array_equal(p.want[0].double().numpy(), value * p.v_scale)
    assert value.max() == 448 and np.abs(value[value != 0]).min() == 2.0 ** -9
    v = p.v_cache.view(torch.uint8)
    owned = ~torch.isnan(p.v_cache.float())
    assert bool(owned.any()) and not bool(((v & 0x7F) == 0x7F)[owned].any())  # every owned slot is finite
    ac.assert_bits_equal(ac.to_bf16(ac.reference(p)), p.want, "the fp64 reference", zeros_by_value=True)
    for tile in (16, 32):
        ac.assert_bits_equal(ac.twin(p, tile), p.want, f"the twin at tile {tile}", zeros_by_value=True)


@pytest.mark.parametrize("kind", ac.KINDS)
def test_random_cases_fit_the_bound(kind):
    """``f <= u / 4 max |v|`` (the bf16 terms dominate), and the twin is inside the bound at tiles of 16, 32 and 64."""
    assert max(ac.RANDOM_MORE[3]) == 4096  # the longest the case may be; the assertions below hold at it
    for case in (*ac.RANDOM_CASES, ac.RANDOM_MORE):
        p = ac.random_problem(kind, *case)
        bound, rel, share = ac.error_bound(p)
        assert rel <= ac.U / 4 and share <= 1.0, (case, rel)
        ref = ac.reference(p)
        for b, n in enumerate(p.lens()):
            assert n > 0 or (not ref[b].any() and not bound[b].any())
        for tile in (16, 32, 64):
            err = np.abs(ac.twin(p, tile).double().numpy() - ref)
            worst = float((err / np.maximum(bound, 1e-300)).max())
            print(f"{kind} case {case[0]} tile {tile}: f is {share:.3f} of u/4 max|v|, twin error {worst:.3f} of bound")
            assert bool((err <= bound).all()), (case, tile, worst)


# ---- the table ---------------------------------------------------------------------------------------------------------

def test_attn_table_is_the_librarys_and_ends(hip):
    assert hip.decode_attn_cfgs() == ac.CFGS
    L = hip.lib()
    import ctypes

    for cfg in (-1, len(ac.CFGS), 99):
        assert L.gsx_decode_attn_cfg_name(cfg) is None
        w, f = ctypes.c_int(7), ctypes.c_int(7)
        assert L.gsx_decode_attn_cfg_shape(cfg, ctypes.byref(w), ctypes.byref(f)) != 0 and (w.value, f.value) == (7, 7)


def test_attn_workspace_bytes(hip):
    """A multiple of the partial's 520 bytes per (sequence, head), never more than 64 splits' worth, none where one
    split does (many pairs, or a short context); refused by name for a bad shape."""
    for b, hq, n in ((1, 64, 32768), (8, 64, 8192), (64, 64, 2048), (256, 64, 1024), (1, 8, 100), (5, 32, 1100)):
        got = hip.decode_attn_workspace_bytes(b, hq, 128, 16, n)
        assert got % (b * hq * ac.PARTIAL_BYTES) == 0 and got // (b * hq * ac.PARTIAL_BYTES) <= ac.MAX_SPLITS
    assert hip.decode_attn_workspace_bytes(1, 64, 128, 16, 32768) > 0
    assert hip.decode_attn_workspace_bytes(256, 64, 128, 16, 64) == 0
    for kw, text in (({"d": 64}, "need D == 128"), ({"page": 24}, "need page % 16 == 0 and 16 <= page <= 256"),
                     ({"b": 0}, "need 1 <= B"), ({"n": 0}, "need max_seq_len >= 1")):
        v = {"b": 2, "hq": 8, "d": 128, "page": 16, "n": 100, **kw}
        with pytest.raises(hip.HipError, match=f"gsx_decode_attn_workspace_bytes: {text}"):
            hip.decode_attn_workspace_bytes(v["b"], v["hq"], v["d"], v["page"], v["n"])


def test_pick_is_the_librarys_dispatch_rule(hip):
    """``attn_decode_cases.pick`` against the library, through the workspace query alone (a launch is never used to
    probe the rule: where one split is picked nothing would be refused).  With Hq <= 16 the query counts B pairs, so
    its bytes over B * Hq * 520 are the split count, and 0 bytes mean one split.  Then "any legal Hkv": whatever Hkv
    a caller passes with the B and Hq of the query, the dispatcher picks no more splits than the query allowed for."""
    def query(b, hq, n):
        got = hip.decode_attn_workspace_bytes(b, hq, 128, 16, n)
        assert got % (b * hq * ac.PARTIAL_BYTES) == 0
        return max(got // (b * hq * ac.PARTIAL_BYTES), 1)

    lengths = sorted({1, 31, 33, 1000, 100000, 1 << 30}
                     | {1024 * k + dn for k in range(1, 67) for dn in (-32, -31, -1, 0, 1)})  # around every 32 * 32 * k
    seen = set()
    for pairs in (*range(1, 9), 9, 31, 32, 33, 64, 255, 256, 257, 512):
        for n in lengths:
            want = ac.pick(pairs, n)
            assert query(pairs, 16, n) == want, (pairs, n, want)
            seen.add(want)
        assert query(pairs, 5, 8192) == ac.pick(pairs, 8192)
    assert seen >= {1, 2, 3, 4, 8, 32, 37, 43, 64} and max(seen) == ac.MAX_SPLITS
    assert [ac.pick(*row) for row in ((64, 8192), (2, 8192), (8, 32768), (7, 37888), (4, 65536), (3, 65536))] == \
        [4, 8, 32, 37, 64, 64]
    for b in (1, 2, 3, 8, 64):
        for hq in (1, 8, 16, 17, 32, 48, 64, 96, 128):
            legal = [hkv for hkv in range(1, hq + 1) if hq % hkv == 0 and hq // hkv <= 16]
            for n in (100, 1100, 4096, 8192, 32768, 37888, 65536, 1 << 20):
                allowed = query(b, hq, n)
                assert all(ac.pick(b * hkv, n) <= allowed for hkv in legal), (b, hq, n, allowed)


# ---- what the entry points refuse --------------------------------------------------------------------------------------

# Addresses that are never dereferenced: every call below is refused before the first device call.
Q, K, V, BT, SL, O, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000


class _NoStream:
    """Stands in for ``hip.Stream``: the calls under test never get as far as using one."""
    handle = None


def _good(kind):
    scales = (1.0, 1.0) if kind == "bf16" else (0.5, 2.0)
    return {"q": Q, "k": K, "v": V, "bt": BT + 4, "sl": SL + 4, "o": O, "b": 3, "hq": 16, "hkv": 2, "d": 128, "page": 32,
            "num_pages": 40, "stride": 10, "n": 320, "scale": 0.088, "ks": scales[0], "vs": scales[1], "ws": WS,
            "ws_bytes": 1 << 30, "splits": 2}


def _call(hip, kind, cfg, v):
    args = (_NoStream, kind, v["q"], v["k"], v["v"], v["bt"], v["sl"], v["o"], v["b"], v["hq"], v["hkv"], v["d"],
            v["page"], v["num_pages"], v["stride"], v["n"], v["scale"])
    tail = (v["ks"], v["vs"], v["ws"], v["ws_bytes"])
    if cfg is None:
        hip.decode_attn(*args, *tail)
    else:
        hip.decode_attn_cfg(*args, cfg, v["splits"], *tail)


def _entry(cfg):
    return "gsx_decode_attn" if cfg is None else "gsx_decode_attn_launch_cfg"


@pytest.mark.parametrize("cfg", ac.ALL, ids=lambda c: "dispatch" if c is None else str(c))
@pytest.mark.parametrize("kind", ac.KINDS)
def test_attn_entry_points_reject_bad_arguments_by_name(hip, kind, cfg):
    def rej(text, **kw):
        with pytest.raises(hip.HipError, match=f"{_entry(cfg)}: {text}"):
            _call(hip, kind, cfg, {**_good(kind), **kw})

    for d in (0, 64, 127, 256):
        rej("need D == 128", d=d)
    rej("need 1 <= B", b=0)
    rej("need 1 <= Hq", hq=0)
    rej("B \\* Hq must stay below 2\\^31", b=1 << 20, hq=4096, hkv=256)  # the merge launches B * Hq workgroups
    for hq, hkv in ((16, 3), (16, 0), (34, 2), (17, 1), (8, 16)):
        rej("need Hq % Hkv == 0 and Hq / Hkv <= 16", hq=hq, hkv=hkv)
    for page in (0, 8, 24, 272, 512, -16):
        rej("need page % 16 == 0 and 16 <= page <= 256", page=page)
    rej("need num_pages >= 1", num_pages=0)
    rej("need table_stride >= 1", stride=0)
    rej("need max_seq_len >= 1", n=0)
    rej("need max_seq_len <= table_stride \\* page", n=321)
    for name in ("q", "k", "v", "o", "bt", "sl"):
        rej("Q, K_cache, V_cache, O, block_table and seq_lens must not be NULL", **{name: 0})
    for name in ("q", "k", "v", "o"):
        rej("Q, K_cache, V_cache and O must be 16-B aligned", **{name: Q + 8})
    for name in ("bt", "sl"):
        rej("block_table and seq_lens must be 4-B aligned", **{name: BT + 2})
    for name in ("scale", "ks", "vs"):
        rej("scale, k_scale and v_scale must be finite", **{name: float("nan")})
    if kind == "bf16":
        rej("a bf16 cache takes no scales: k_scale and v_scale must be 1.0", ks=0.5)
        rej("a bf16 cache takes no scales: k_scale and v_scale must be 1.0", vs=2.0)
    if cfg is not None:
        for splits in (0, -1, 65):
            rej("need 1 <= splits <= 64", splits=splits)
        need = 3 * 16 * 2 * ac.PARTIAL_BYTES
        rej(f"workspace too small: 2 splits need {need} bytes", ws_bytes=need - 1)
        rej(f"workspace too small: 2 splits need {need} bytes", ws=0)
        rej("workspace must be 16-B aligned", ws=WS + 8)
    else:
        # the dispatcher splits one long sequence: it needs the workspace the query names
        v = {"b": 1, "hq": 16, "hkv": 2, "stride": 1024, "n": 32768}
        need = hip.decode_attn_workspace_bytes(1, 16, 128, 32, 32768)
        assert need > 0
        rej("workspace too small", **v, ws_bytes=16)
        rej("workspace too small", **v, ws=0)


@pytest.mark.parametrize("cfg", ac.ALL, ids=lambda c: "dispatch" if c is None else str(c))
def test_attn_unknown_kind_is_rejected_by_name(hip, cfg):
    L = hip.lib()
    g = _good("bf16")
    for kind in (-1, 2, 7):
        args = [None, kind, Q, K, V, BT, SL, O, 3, 16, 2, 128, 32, 40, 10, 320, 0.088, 1.0, 1.0, WS, 1 << 30]
        args += [] if cfg is None else [cfg, g["splits"]]
        rc = (L.gsx_decode_attn if cfg is None else L.gsx_decode_attn_launch_cfg)(*args)
        assert rc != 0 and L.gsx_last_error().decode() == f"{_entry(cfg)}: unknown kind {kind}"
    with pytest.raises(ValueError, match="attention cache kind 'fp4'"):
        _call(hip, "fp4", cfg, g)


@pytest.mark.parametrize("kind", ac.KINDS)
def test_attn_unknown_config_is_rejected_by_name(hip, kind):
    for cfg in (-1, len(ac.CFGS), 40):
        with pytest.raises(hip.HipError, match="gsx_decode_attn_launch_cfg: unknown config"):
            _call(hip, kind, cfg, _good(kind))


def test_time_decode_attn_rejects_before_it_touches_the_device(hip):
    g = _good("bf16")
    args = (_NoStream, "bf16", Q, K, V, BT, SL, O, 3, 16, 2, 64, 32, 40, 10, 320, 0.088)
    with pytest.raises(hip.HipError, match="gsx_decode_attn: need D == 128"):
        hip.time_decode_attn(*args, 0, 1.0, 1.0, g["ws"], g["ws_bytes"])


# ---- the tools -------------------------------------------------------------------------------------------------------

def test_workload_and_isolation_parsers_take_the_attn_workload():
    from gsxtools import isolation, workload

    for mod in (workload, isolation):
        ap = mod.build_parser()
        assert "--kv-dtype" in ap.format_help()
        d = ap.parse_args(["--workload", "attn"])
        assert (d.workload, d.batch, d.context, d.heads, d.kv_heads, d.kv_dtype, d.kv_gib, d.page) == \
            ("attn", 8, 8192, 64, 8, "bf16", None, 16)
        for b in (1, 17, 256):
            assert ap.parse_args(["--workload", "attn", "--batch", str(b)]).batch == b
        got = ap.parse_args(["--workload", "attn", "--kv-dtype", "fp8", "--kv-gib", "0.5", "--context", "512"])
        assert (got.kv_dtype, got.kv_gib, got.context) == ("fp8", 0.5, 512)
        for bad in (["--workload", "attn", "--batch", "0"], ["--workload", "attn", "--batch", "257"],
                    ["--workload", "attn", "--kv-dtype", "mxfp4"], ["--workload", "decode", "--batch", "17"]):
            with pytest.raises(SystemExit):
                ap.parse_args(bad)
    assert {"attn-noisy", "attn-noisy-partitioned"} <= set(isolation.SCENARIOS)
    # pod 0 of an attn-* scenario is an attention pod whatever --workload says: its --batch has the attention's range
    iso = isolation.build_parser()
    assert iso.parse_args(["--scenarios", "attn-noisy,attn-noisy-partitioned", "--batch", "64"]).batch == 64
    with pytest.raises(SystemExit):
        iso.parse_args(["--scenarios", "decode-noisy", "--batch", "64"])
    a = isolation.build_parser().parse_args(["--workload", "attn", "--kv-dtype", "fp8", "--kv-gib", "2"])
    assert isolation.attn_cmdline(a) == ["--context", "8192", "--heads", "64", "--kv-heads", "8", "--kv-dtype", "fp8",
                                         "--page", "16", "--kv-gib", "2.0"]
    # what the harness hands an attention pod is what the workload's parser takes
    assert workload.build_parser().parse_args(["--workload", "attn", *isolation.attn_cmdline(a)]).kv_gib == 2.0


def test_workload_kv_ring_size():
    from gsxtools import workload as wl

    gib = 1 << 30
    assert wl.kv_layer_bytes("bf16", 8, 8192, 8) == 256 << 20  # K and V, 8 x 8192 tokens, 8 heads of 128
    assert wl.kv_layer_bytes("fp8", 8, 8192, 8) == 128 << 20
    assert wl.kv_pages(8, 8192, 16) == (512, 4096) and wl.kv_pages(3, 100, 16) == (7, 21)
    assert wl.default_kv_bytes(0) == 4 * gib and wl.default_kv_bytes(8) == 2 * gib
    for dtype in ac.KINDS:
        for batch, context in ((1, 32768), (8, 8192), (256, 1024), (4, 512)):
            one = wl.kv_layer_bytes(dtype, batch, context, 8)
            for want in (0, one, one + 1, gib // 8, 4 * gib):
                layers = wl.kv_ring_layers(want, one)
                assert layers >= 2 and layers * one >= want and (layers == 2 or (layers - 1) * one < want)
    # at the defaults a step streams more than the 256 MiB Infinity Cache
    assert wl.kv_ring_layers(4 * gib, wl.kv_layer_bytes("bf16", 8, 8192, 8)) == 16
    assert math.isclose(wl.kv_ring_layers(4 * gib, 1 << 28) * (1 << 28), 4 * gib)
