"""Problems for the decode attention tests (native/kernels/attn_decode.hip): one new token per sequence, grouped-query
attention over a paged KV cache in bf16 or e4m3, D = 128.

Plain Python on torch and NumPy, no GPU.  These things live here (and :func:`pick`, the dispatcher's rule; the
**window cases**, which are exact like the selection cases but weigh a run of tokens equally, so that a token
counted twice or not at all shows, are described above :func:`window_spans`):

* :func:`reference`, the fp64 attention of a :class:`Problem`, and :func:`twin`, a NumPy transcription of the numeric
  contract in ``gsx_kernels.h``: fp32 scores times ``scale * k_scale * log2 e``, ``exp2`` against a running maximum,
  ``l`` from the unrounded probabilities, P rounded to bf16 for the PV product, fp32 accumulators, one rounding of
  ``(acc / l) * v_scale`` to bf16, for any tile size;
* **selection cases** (:func:`selection_problem`), whose result is exact whatever the order of the arithmetic.  With
  ``w_j`` row j of the 128 x 128 Walsh matrix, query head g of a group has ``q = w_g`` and token t has
  ``k_t = 16 * sum of w_g`` over the heads that target it (a token nobody targets: ``16 w_j``, j >= 16).  The rows
  are orthogonal, so with ``scale = 1 / sqrt(128)`` a head's target scores 16 * 128 / sqrt(128) * log2 e = 261.2 in the
  ``exp2`` argument and every other token 0: the target's probability is exactly 1, the others underflow to exactly 0
  (fp32 ``exp2(-261)`` is 0, denormals included), ``l = 1`` and O is the target's row of V bit for bit.  V holds
  integers 1..15 that encode (physical page, KV head, slot, d), so a row read from anywhere else differs.  All of
  it is exact in e4m3 too (16 n for n <= 16, integers <= 15), and with ``k_scale`` and ``v_scale`` powers of two.
  Slots at or past ``seq_len`` and pages no sequence owns are **poison**: ``k = 32 w_g``, which would win the softmax
  if it were read, and V = NaN.  Unused block-table entries name a poison page, never an index out of range: a wrong
  kernel fails a comparison and does not fault;
* **random cases** (:func:`random_problem`) with the bound of :func:`error_bound` against the fp64 reference.

The bound.  With u = 2^-8 (bf16's unit roundoff) an element of O may be off by

    u * max_t |v[t][d]|  +  u * |o_ref|  +  f

The first term is P rounded to bf16: each probability moves by at most u of itself, the weights sum to 1, so the
weighted sum of column d of V moves by at most u times its largest entry (and the same relative change of l cancels
to first order, which only helps).  The second is the final rounding.  ``f`` is what fp32 does:
``f = 2 ln 2 * dx * max_t |v[t][d]|``, where ``dx`` bounds the error of an ``exp2`` argument: a relative change of
``ln 2 * dx`` in every p, at most twice that in p / l.  With eps = 2^-24, c = scale * k_scale * log2 e and S the largest
``sum_d |q_d k_d|`` of the case,

    dx = (D + 2) eps S c        D additions of the dot product, the rounding of c and the multiplication by it
       + 2 eps S c              the subtraction x - m, |x - m| <= 2 S c
       + (T + 4) eps / ln 2     exp2 itself (2 ulp) and the fp32 sums of l and acc over T tokens, written as an
                                equivalent change of the argument

V means the dequantised value (times ``v_scale``).  ``tests/test_attn_decode_cases.py`` asserts for every random case
that ``f <= u / 4 * max |v|``, so the bf16 terms dominate, and that the twin stays inside the bound.
"""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np
import torch

D = 128
TILE = 32  # tokens of a kernel tile
KINDS = ("bf16", "fp8")
FP8 = torch.float8_e4m3fn
U = 2.0 ** -8
EPS = 2.0 ** -24
LOG2E = 1.4426950408889634
MAX_SPLITS = 64
PARTIAL_BYTES = (D + 2) * 4  # workspace per (sequence, query head, split)

# the library's table (gsx_decode_attn_cfg_name / _cfg_shape): name, waves per workgroup, tiles in flight per wave
CFGS = {0: ("4w-f1", 4, 1), 1: ("4w-f2", 4, 2), 2: ("8w-f1", 8, 1), 3: ("8w-f2", 8, 2)}
ALL = [*CFGS, None]  # None: the dispatching entry point
SPLITS = (1, 2, 3, 8)
MORE_SPLITS = (16, 32, 37, 64)  # what the dispatcher can also choose: run on a shorter list of lengths
DISPATCHED = 2  # the configuration gsx_decode_attn runs (attn_pick() in attn_decode.hip)


def pick(pairs: int, max_seq_len: int) -> int:
    """The split count ``gsx_decode_attn`` runs for ``pairs`` (sequence, KV head) pairs: a transcription of
    ``attn_pick()``.  One workgroup for each of 256 CUs, but every wave of a split keeps 4 tiles, and at most 64."""
    tiles = -(-max_seq_len // TILE)
    return max(min(-(-256 // pairs), tiles // (4 * CFGS[DISPATCHED][1]), MAX_SPLITS), 1)


@functools.lru_cache(maxsize=None)
def walsh() -> np.ndarray:
    """The 128 x 128 Walsh (Sylvester-Hadamard) matrix, entries +-1, as float32; its rows are orthogonal."""
    h = np.ones((1, 1), dtype=np.float32)
    while h.shape[0] < D:
        h = np.block([[h, h], [h, -h]])
    return h


@dataclasses.dataclass(frozen=True)
class Problem:
    """One decode step.  ``q`` is bf16 ``[B][Hq][D]``; the caches are ``[num_pages][Hkv][page][D]`` in bf16 or
    ``torch.float8_e4m3fn``; ``block_table`` is int32 ``[B][table_stride]`` and ``seq_lens`` int32 ``[B]``.  ``want``
    is the exact bf16 result of a selection case, None otherwise.  Tensors are shared: not to be written to."""
    kind: str
    q: torch.Tensor
    k_cache: torch.Tensor
    v_cache: torch.Tensor
    block_table: torch.Tensor
    seq_lens: torch.Tensor
    max_seq_len: int
    scale: float
    k_scale: float = 1.0
    v_scale: float = 1.0
    want: torch.Tensor | None = None
    page_base: int = 0  # the caches here hold physical pages page_base .. only (a cache too large for the host)
    beyond: int = 0  # pages at the end of the caches that ``num_pages`` does not count (:func:`page_clamp_problem`)

    @property
    def b(self) -> int:
        return self.q.shape[0]

    @property
    def hq(self) -> int:
        return self.q.shape[1]

    @property
    def hkv(self) -> int:
        return self.k_cache.shape[1]

    @property
    def g(self) -> int:
        return self.hq // self.hkv

    @property
    def page(self) -> int:
        return self.k_cache.shape[2]

    @property
    def num_pages(self) -> int:
        return self.page_base + self.k_cache.shape[0] - self.beyond

    @property
    def table_stride(self) -> int:
        return self.block_table.shape[1]

    def lens(self) -> list[int]:
        """The lengths the kernel uses: ``seq_lens`` clamped to ``max_seq_len``."""
        return [min(max(int(x), 0), self.max_seq_len) for x in self.seq_lens]

    def gather(self, b: int, dtype=np.float64, scaled: bool = True) -> tuple[np.ndarray, np.ndarray]:
        """``K[Hkv][len][D]`` and ``V[Hkv][len][D]`` of sequence ``b``, through its block table (a page index at or
        above ``num_pages`` names the last page, as the contract has it): dequantised, or (``scaled=False``) the
        stored values."""
        n = self.lens()[b]
        t = np.arange(n)
        pages = np.minimum(self.block_table[b].numpy()[t // self.page], self.num_pages - 1) - self.page_base
        slots = t % self.page
        k = _float64(self.k_cache[pages, :, slots]) * (self.k_scale if scaled else 1.0)
        v = _float64(self.v_cache[pages, :, slots]) * (self.v_scale if scaled else 1.0)  # [len][Hkv][D]
        return k.transpose(1, 0, 2).astype(dtype), v.transpose(1, 0, 2).astype(dtype)


@functools.lru_cache(maxsize=None)
def _fp8_values() -> np.ndarray:
    return torch.arange(256, dtype=torch.uint8).view(FP8).to(torch.float64).numpy()


def _float64(t: torch.Tensor) -> np.ndarray:
    """The values of a piece of a cache; e4m3 through a table of the 256 codes (torch converts them one by one)."""
    return _fp8_values()[t.view(torch.uint8).numpy()] if t.dtype == FP8 else t.to(torch.float64).numpy()


def reference(p: Problem) -> np.ndarray:
    """The attention in fp64, ``[B][Hq][D]``; a sequence of length 0 gives zeros."""
    out = np.zeros((p.b, p.hq, D))
    q = p.q.to(torch.float64).numpy().reshape(p.b, p.hkv, p.g, D)
    for b, n in enumerate(p.lens()):
        if n == 0:
            continue
        k, v = p.gather(b)
        x = np.einsum("hgd,htd->hgt", q[b], k) * p.scale
        w = np.exp(x - x.max(axis=2, keepdims=True))
        w /= w.sum(axis=2, keepdims=True)
        out[b] = np.einsum("hgt,htd->hgd", w, v).reshape(p.hq, D)
    return out


def to_bf16(x: np.ndarray) -> torch.Tensor:
    """Round to nearest even, through fp32 (exact for what the selection cases hold)."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).bfloat16()


def _bf16_round(x: np.ndarray) -> np.ndarray:
    return to_bf16(x).float().numpy()


def tile_ranges(n: int, tile: int = TILE) -> list[tuple[int, int]]:
    """The tiles of a sequence of ``n`` tokens as ``(first token, one past the last)``, in order."""
    return [(t0, min(t0 + tile, n)) for t0 in range(0, n, tile)]


def twin(p: Problem, tile: int = TILE, ranges=None) -> torch.Tensor:
    """The contract in NumPy, fp32 throughout, in tiles of ``tile`` tokens: bf16 ``[B][Hq][D]``.  ``ranges(b, n)``, if
    given, names the runs of tokens that sequence b visits instead of :func:`tile_ranges` (none of them empty): a twin
    that counts tokens wrongly, for the tests of the tests (:func:`miscounts`)."""
    out = np.zeros((p.b, p.hq, D), dtype=np.float32)
    q = p.q.float().numpy().reshape(p.b, p.hkv, p.g, D)
    c = np.float32(np.float32(np.float32(p.scale) * np.float32(p.k_scale)) * np.float32(LOG2E))
    for b, n in enumerate(p.lens()):
        if n == 0:
            continue
        k, v = p.gather(b, np.float32, scaled=False)  # the factors are applied where the kernel applies them
        m = np.full((p.hkv, p.g), -np.inf, dtype=np.float32)
        l = np.zeros((p.hkv, p.g), dtype=np.float32)
        acc = np.zeros((p.hkv, p.g, D), dtype=np.float32)
        for t0, t1 in tile_ranges(n, tile) if ranges is None else ranges(b, n):
            kt, vt = k[:, t0:t1], v[:, t0:t1]
            x = (np.einsum("hgd,htd->hgt", q[b], kt).astype(np.float32) * c).astype(np.float32)
            mn = np.maximum(m, x.max(axis=2))
            with np.errstate(invalid="ignore"):
                alpha = np.exp2(m - mn).astype(np.float32)
            pr = np.exp2(x - mn[:, :, None]).astype(np.float32)
            l = (l * alpha + pr.sum(axis=2, dtype=np.float32)).astype(np.float32)
            acc = acc * alpha[:, :, None] + np.einsum("hgt,htd->hgd", _bf16_round(pr), vt).astype(np.float32)
            m = mn
        o = ((acc / l[:, :, None]).astype(np.float32) * np.float32(p.v_scale)).astype(np.float32)
        out[b] = o.reshape(p.hq, D)
    return to_bf16(out)


# ---- selection cases ----------------------------------------------------------------------------------------------

POISON_PAGES = 3


def _page_order(total: int, mode: str) -> np.ndarray:
    """Where the logical pages of all sequences (in order) and then the poison pages lie physically."""
    i = np.arange(total)
    if mode == "identity":
        return i
    if mode == "reversed":
        return total - 1 - i
    assert mode == "scattered", mode
    step = next(s for s in range(max(2, (total * 5) // 8), 2 * total + 7) if math.gcd(s, total) == 1)
    return (i * step + 1) % total


def v_rows(pp, h, slot, page: int, hkv: int) -> np.ndarray:
    """The row of V at (physical page, KV head, slot): integers 1..15 that spell the triple's number in 3-bit digits,
    digit d % 7 plus d % 8 at position d.  Broadcasts over arrays."""
    code = (np.asarray(pp, dtype=np.int64) * hkv + h) * page + slot
    d = np.arange(D)
    return (1 + ((code[..., None] >> (3 * (d % 7))) & 7) + d % 8).astype(np.float32)


def boundary_tokens(n: int, page: int, cuts=()) -> list[int]:
    """The tokens of a sequence of ``n`` that a target has to visit: the first and the last, and both sides of every
    boundary of a 16-token half, a tile, a page and of every extra cut (a split's first token) that lies inside."""
    marks = {0, n - 1}
    for cut in [*range(16, n, 16), *range(page, n, page), *cuts]:
        if 0 < cut < n:
            marks |= {cut - 1, cut}
    return sorted(marks)


def split_cuts(n: int, splits: int) -> list[int]:
    """The first token of every split of a sequence of ``n`` tokens, as the kernel cuts it: whole tiles, the same
    count to every split but the last ones."""
    nt = -(-n // TILE)
    tps = -(-nt // splits)
    return [s * tps * TILE for s in range(1, splits) if s * tps * TILE < n]


def all_cuts(n: int) -> list[int]:
    """The cuts of a sequence of ``n`` tokens at every split count of ``SPLITS`` (at most 10 of them)."""
    return sorted({c for s in SPLITS for c in split_cuts(n, s)})


def pick_targets(n: int, page: int, cuts, heads: int, rot: int) -> list[int]:
    """The tokens ``heads`` heads of a sequence of ``n`` target, in order of priority.  First what has to be hit in
    every case: the first token, the last, and both sides of every cut.  Then the other :func:`boundary_tokens`
    (halves, tiles, pages), taken at even distances over the WHOLE sequence, so that a long sequence has targets in
    its steady loop and its drain and not only near its start.  ``rot`` (the sequence's number) turns both lists, so
    the sequences of a batch differ.  With no more heads than the first list holds, they take a window of the two
    lists joined, ``rot`` windows in: equal sequences then visit everything between them."""
    must = list(dict.fromkeys([0, n - 1, *(t for c in cuts if 0 < c < n for t in (c - 1, c))]))
    rest = [t for t in boundary_tokens(n, page, cuts) if t not in set(must)]
    if heads <= len(must):
        order = must + rest
        return [order[(i + rot * heads) % len(order)] for i in range(heads)]
    free, pool = heads - len(must), rest or must
    step = max(len(pool) / free, 1.0)
    r = rot % len(must)
    return must[r:] + must[:r] + [pool[(int(i * step) + rot) % len(pool)] for i in range(free)]


def selection_problem(kind: str, g: int, page: int, lens, *, tables: str = "scattered", hkv: int = 2, cuts=None,
                      extra_stride: int = 0, max_seq_len: int | None = None, over=(), shared: bool = False,
                      k_scale: float = 1.0, v_scale: float = 1.0, page_base: int = 0, below=None) -> Problem:
    """A selection case (module docstring) of ``len(lens)`` sequences.  The ``g * hkv`` heads of sequence b target
    the tokens of :func:`pick_targets` (``cuts``: per sequence, the first tokens of its splits), dealt to the KV heads
    in turn, the turn starting one KV head later every round (entry i goes to KV head ``(i + i // hkv) % hkv``): the
    two sides of a cut go to different KV heads, each KV head gets left sides and right sides, and each has targets
    along the whole sequence.  ``tables``: how physical pages are
    handed out; ``shared``: sequence 1 has sequence 0's block table (and must have its length); ``over``: sequences
    whose ``seq_lens`` entry is raised above ``max_seq_len``, which the kernel clamps; ``below``: ``{sequence: a
    negative seq_lens entry}`` for sequences of length 0, which the kernel clamps to 0; ``extra_stride``: columns of
    the block table beyond the longest sequence's need; ``page_base``: every physical page index is raised by it and
    the returned caches hold the pages from there on only."""
    lens = list(lens)
    nb = len(lens)
    hq = g * hkv
    w = walsh()
    max_seq_len = max(max(lens), 1) if max_seq_len is None else max_seq_len
    assert all(n <= max_seq_len for n in lens)
    npages = [-(-n // page) for n in lens]
    owners = [b for b in range(nb) if not (shared and b == 1)]
    if shared:
        assert nb >= 2 and lens[1] == lens[0]
    used = sum(npages[b] for b in owners)
    total = used + POISON_PAGES
    order = _page_order(total, tables)
    poison = [int(x) for x in order[used:]]
    stride = max(-(-max_seq_len // page), 1) + extra_stride
    table = np.empty((nb, stride), dtype=np.int32)
    at = 0
    for b in range(nb):
        table[b] = [poison[(b + i) % POISON_PAGES] for i in range(stride)]
        if shared and b == 1:
            table[1] = table[0]
            continue
        table[b, :npages[b]] = order[at:at + npages[b]]
        at += npages[b]

    k = np.empty((total, hkv, page, D), dtype=np.float32)
    v = np.full((total, hkv, page, D), np.nan, dtype=np.float32)
    k[:] = 32 * w[np.arange(page) % g][None, None]  # poison everywhere, then the owned slots
    want = np.zeros((nb, hq, D), dtype=np.float32)
    for b in range(nb):
        n = lens[b]
        if n == 0:
            continue
        t = np.arange(n)
        pp, slot = table[b][t // page].astype(np.int64), t % page
        tb = 0 if shared and b == 1 else b  # a shared table: the owner's targets
        picked = pick_targets(n, page, () if cuts is None else cuts[tb], hq, tb)
        for h in range(hkv):
            if b in owners:
                k[pp, h, slot] = 16 * w[16 + (t + 7 * h) % (D - 16)]
                v[pp, h, slot] = v_rows(pp + page_base, h, slot, page, hkv)
            targets = [tok for i, tok in enumerate(picked) if (i + i // hkv) % hkv == h]
            for tok in set(targets):
                if b in owners:
                    k[pp[tok], h, slot[tok]] = 16 * sum(w[gi] for gi in range(g) if targets[gi] == tok)
            for gi, tok in enumerate(targets):
                want[b, h * g + gi] = v_rows(pp[tok] + page_base, h, slot[tok], page, hkv) * v_scale
    seq_lens = np.array(lens, dtype=np.int32)
    for b in over:
        assert lens[b] == max_seq_len
        seq_lens[b] = max_seq_len + 1 + 1000 * b
    for b, value in (below or {}).items():
        assert lens[b] == 0 and -2 ** 31 <= value < 0
        seq_lens[b] = value
    q = np.tile(w[:g], (nb, hkv, 1)).reshape(nb, hq, D)
    kc, vc = torch.from_numpy(k), torch.from_numpy(v)
    kc, vc = (kc.bfloat16(), vc.bfloat16()) if kind == "bf16" else (kc.to(FP8), vc.to(FP8))
    return Problem(kind, to_bf16(q), kc, vc, torch.from_numpy(table + np.int32(page_base)), torch.from_numpy(seq_lens),
                   max_seq_len, (1.0 / math.sqrt(D)) / k_scale, k_scale, v_scale, to_bf16(want), page_base)


def targets(p: Problem) -> list[list[int]]:
    """The token every head of a selection case targets, ``[B][Hq]``, read back from ``want``: a row of V spells its
    (physical page, KV head, slot) in its first seven elements (:func:`v_rows`), and the sequence's block table
    says which token lies there.  A sequence of length 0 has none."""
    assert p.want is not None
    out = []
    for b, n in enumerate(p.lens()):
        out.append([])
        if n == 0:
            continue
        t = np.arange(n)
        pp, slot = p.block_table[b].numpy()[t // p.page].astype(np.int64), t % p.page
        _, v = p.gather(b)
        for j in range(p.hq):
            row = p.want[b, j].double().numpy() / p.v_scale
            code = sum(int(row[d] - 1 - d) << (3 * d) for d in range(7))
            (tok,) = np.nonzero((((pp * p.hkv + j // p.g) * p.page + slot) & ((1 << 21) - 1)) == code)[0]
            assert np.array_equal(v[j // p.g, tok], row * p.v_scale), (b, j, tok)
            out[b].append(int(tok))
    return out


def fp8_scales(kind: str) -> dict:
    """Powers of two for the selection cases of an e4m3 cache; a bf16 cache takes none."""
    return {} if kind == "bf16" else {"k_scale": 0.5, "v_scale": 2.0}


SHORT_LENS = (0, 1, 2, 15, 16, 17, 31, 32, 33)


def tile_counts(cfg, splits: int) -> list[int]:
    """Tiles PER SPLIT that matter to a configuration of W waves with F tiles in flight each: waves without a tile
    (1, 2, W - 1), a ragged round (W + 1, 2 W + 1), the short path with its conditional prologue (F W + 1: a wave
    with fewer than 2 F tiles), the counts at which some and then all waves enter the steady loop (2 F W - W + 1,
    2 F W), one more (2 F W + 1), and the drain behind a longer loop (3 F W + 2; left out at 8 splits to keep the
    cases small).  The dispatching entry point takes its own configuration's ("8w-f1")."""
    _, w, f = CFGS[DISPATCHED if cfg is None else cfg]
    counts = {1, 2, w - 1, w, w + 1, 2 * w + 1, f * w + 1, 2 * f * w - w + 1, 2 * f * w, 2 * f * w + 1}
    if splits < 8:
        counts.add(3 * f * w + 2)
    return sorted(counts)


def split_lengths(cfg, splits: int) -> list[int]:
    """Sequence lengths for ``splits`` splits: every :func:`tile_counts` count as the tiles of each split, the last
    tile ragged (17 tokens); and with more than one split, the lengths at which a split gets no token (fewer tiles
    than splits), the last split gets exactly one token, and the last split is one full tile."""
    out = {n * splits * TILE - 15 for n in tile_counts(cfg, splits)}
    if splits > 1:
        tps = min(3, splits)  # tiles per split, as the kernel then cuts: ceil((tps (splits - 1) + 1) / splits) = tps
        out |= {(splits - 1) * TILE - 3, tps * (splits - 1) * TILE + 1, tps * (splits - 1) * TILE + TILE}
    return sorted(out)


def chunks(xs, n: int = 5):
    xs = list(xs)
    return [xs[i:i + n] for i in range(0, len(xs), n)]


def short_cases(kind: str) -> list[tuple[str, Problem]]:
    """G in 1, 2, 4, 8, 16 with Hkv = 2, pages of 16 and 64, and ``SHORT_LENS``, five and four sequences to a batch."""
    return [(f"G {g}, page {page}, lengths {lens}", selection_problem(kind, g, page, lens, **fp8_scales(kind)))
            for g in (1, 2, 4, 8, 16) for page in (16, 64) for lens in chunks(SHORT_LENS)]


def split_cases(kind: str, cfg, splits: int) -> list[tuple[str, Problem]]:
    """:func:`split_lengths` in batches of five at G = 16 and pages of 16.  The 32 heads of every sequence target its
    first and its last token and both sides of every cut of every split count of ``SPLITS`` (22 tokens at most), so
    every split that has a token holds a target; the heads left over take half, tile and page boundaries at even
    distances over the whole sequence (:func:`pick_targets`).  ``tests/test_attn_decode_cases.py`` asserts that on
    the targets read back from ``want``."""
    return [(f"lengths {lens}", selection_problem(kind, 16, 16, lens, cuts=[all_cuts(n) for n in lens],
                                                  **fp8_scales(kind)))
            for lens in chunks(split_lengths(cfg, splits))]


def table_cases(kind: str) -> list[tuple[str, Problem]]:
    """Reversed and scattered page orders, a table shared by two sequences, a ``table_stride`` larger than needed, a
    batch that mixes 0 and short lengths with ``max_seq_len``, ``seq_lens`` above ``max_seq_len``, and ``seq_lens``
    of -1 and -2^31 next to a live sequence (rows of zeros)."""
    fs = fp8_scales(kind)
    return [
        ("reversed", selection_problem(kind, 4, 16, [100, 37, 64], tables="reversed", **fs)),
        ("scattered, page 64", selection_problem(kind, 8, 64, [300, 65, 129], tables="scattered", **fs)),
        ("shared", selection_problem(kind, 16, 16, [90, 90, 40], shared=True, **fs)),
        ("stride + 5", selection_problem(kind, 2, 16, [33, 70, 1], extra_stride=5, **fs)),
        ("mixed", selection_problem(kind, 4, 16, [0, 1100, 5, 0, 1100], max_seq_len=1100, **fs)),
        ("clamped", selection_problem(kind, 4, 16, [75, 20, 75], max_seq_len=75, over=(0, 2), **fs)),
        ("negative", selection_problem(kind, 4, 16, [0, 90, 0], below={0: -1, 2: -2 ** 31}, **fs)),
    ]


# ---- window cases -------------------------------------------------------------------------------------------------
#
# A selection case cannot tell whether a token was counted once: every weight is 0 or 1, so a token without a target
# may be dropped or repeated, and a target taken twice gives l = 2 and acc = 2 v, which is v again.  A window case
# gives head g a contiguous WINDOW of s tokens (s a power of two) with equal weights: ``k_t = 16 * sum of w_g`` over the
# heads whose window holds t, so a token scores 261.2 for those heads and 0 for the others, p is exactly 1 inside the
# window and exactly 0 outside, l = s, and every merge weight is exp2(0) or 0.  V is one-hot: token t holds the
# small integer c(t) at d = t % 128 and zeros elsewhere, so
#
#     O[g][d] = (sum of c over the window's tokens with t % 128 == d) / s * v_scale
#
# which is exact in bf16 whatever the order (an integer below 256 over a power of two) and is compared on the raw 16
# bits.  The windows of the G heads of a KV head cover the sequence, neighbours overlapping by at least a token:
# every token counts in some head's l, and every boundary between two tokens (every cut of a split or a tile) lies
# inside some head's window, so both sides' partials enter that head's row with weight exactly 1.

def window_spans(n: int, g: int) -> tuple[int, list[int]]:
    """``(s, starts)``: the window length of a sequence of ``n`` tokens under ``g`` heads and where the g windows
    begin.  s is the largest power of two <= n below 128 tokens, otherwise 128 r with r the smallest power of two at
    which g windows at even distances, the first at token 0 and the last ending at n - 1, overlap their neighbours by
    a token or more.  r <= 64: a column of V holds at most 64 tokens of a window."""
    if n < D:
        s = 1 << (n.bit_length() - 1)
    else:
        fits = [D * r for r in (1, 2, 4, 8, 16, 32, 64) if n == D * r or (g > 1 and -(-(n - D * r) // (g - 1)) < D * r)]
        assert fits, f"{g} windows of at most {64 * D} tokens do not cover {n}"
        s = fits[0]
    assert s == n or (g > 1 and -(-(n - s) // (g - 1)) < s), (n, g, s)
    return s, [(i * (n - s)) // max(g - 1, 1) for i in range(g)]


def window_weight_max(s: int) -> int:
    """c(t) lies in 1 .. this.  A column's sum (s / 128 tokens, at least one) stays below 128, where a bf16 step is
    at most 1/2: one token more or less moves its column by two steps or more.  At s = 8192 that leaves c = 1."""
    return min(15, 127 // max(s // D, 1))


def window_problem(kind: str, g: int, page: int, lens, *, hkv: int = 2, negative: bool = False,
                   tables: str = "scattered", max_seq_len: int | None = None, k_scale: float = 1.0,
                   v_scale: float = 1.0) -> Problem:
    """A window case (above) of ``len(lens)`` sequences.  Head i of KV head h owns window ``(i + h) % g`` of
    :func:`window_spans`.  ``negative``: ``k_t = -16 * (2 * sum of all w_g - sum of w_g over the heads whose window
    holds t)``, which scores -261.2 inside a window and -522.4 outside: every score of the case is far below zero, so
    a running maximum that starts at any finite value never comes down to them (G <= 8 keeps |k| <= 256, exact in
    e4m3).  Poison as in :func:`selection_problem`: slots at or past ``seq_len`` and the pages nobody owns hold
    ``k = 32 w``, which would win, and V = NaN."""
    lens = list(lens)
    nb, hq, w = len(lens), g * hkv, walsh()
    assert not negative or g <= 8
    max_seq_len = max(max(lens), 1) if max_seq_len is None else max_seq_len
    assert all(n <= max_seq_len for n in lens)
    npages = [-(-n // page) for n in lens]
    used = sum(npages)
    total = used + POISON_PAGES
    order = _page_order(total, tables)
    poison = np.array([int(x) for x in order[used:]], dtype=np.int32)
    stride = max(-(-max_seq_len // page), 1)
    table = np.empty((nb, stride), dtype=np.int32)
    k = np.empty((total, hkv, page, D), dtype=np.float32)
    v = np.full((total, hkv, page, D), np.nan, dtype=np.float32)
    k[:] = 32 * w[np.arange(page) % g][None, None]
    want = np.zeros((nb, hq, D))
    every = w[:g].sum(axis=0)
    at = 0
    for b, n in enumerate(lens):
        table[b] = poison[(b + np.arange(stride)) % POISON_PAGES]
        table[b, :npages[b]] = order[at:at + npages[b]]
        at += npages[b]
        if n == 0:
            continue
        s, starts = window_spans(n, g)
        t = np.arange(n)
        pp, slot = table[b][t // page].astype(np.int64), t % page
        for h in range(hkv):
            c = (1 + (3 * t + t // D + 5 * h + 7 * b) % window_weight_max(s)).astype(np.float32)
            held = np.zeros((n, D), dtype=np.float32)  # the sum of w_g over the heads whose window holds the token
            for i in range(g):
                a = starts[(i + h) % g]
                held[a:a + s] += w[i]
                want[b, h * g + i] = np.bincount(t[a:a + s] % D, weights=c[a:a + s], minlength=D) / s * v_scale
            k[pp, h, slot] = -16 * (2 * every - held) if negative else 16 * held
            rows = np.zeros((n, D), dtype=np.float32)
            rows[t, t % D] = c
            v[pp, h, slot] = rows
    assert np.abs(k).max() <= 256 and np.array_equal(to_bf16(want).double().numpy(), want)  # exact in both types
    q = np.tile(w[:g], (nb, hkv, 1)).reshape(nb, hq, D)
    kc, vc = torch.from_numpy(k), torch.from_numpy(v)
    kc, vc = (kc.bfloat16(), vc.bfloat16()) if kind == "bf16" else (kc.to(FP8), vc.to(FP8))
    return Problem(kind, to_bf16(q), kc, vc, torch.from_numpy(table), torch.tensor(lens, dtype=torch.int32),
                   max_seq_len, (1.0 / math.sqrt(D)) / k_scale, k_scale, v_scale, to_bf16(want))


def to_fp8(p: Problem, k_scale: float = 0.5, v_scale: float = 2.0) -> Problem:
    """An exact bf16 case with its caches stored as e4m3 under these scales (powers of two; every value of an exact
    case is an e4m3 number): what its builder returns for "fp8", without building it again."""
    assert p.kind == "bf16" and p.want is not None and p.k_scale == 1.0 and p.v_scale == 1.0
    return dataclasses.replace(p, kind="fp8", k_cache=p.k_cache.float().to(FP8), v_cache=p.v_cache.float().to(FP8),
                               scale=p.scale / k_scale, k_scale=k_scale, v_scale=v_scale,
                               want=(p.want.float() * v_scale).bfloat16())


def miscounts(n: int, tile: int = TILE) -> dict[str, list[tuple[int, int]]]:
    """``{what: the runs of tokens a wrong kernel visits}`` for a sequence of ``n`` tokens (for :func:`twin`'s
    ``ranges``): one tile taken twice and one left out, at the first, a middle and the last position; the second
    16-token half of a middle tile left out; a single token left out and one taken twice.  Empty with one tile."""
    base = tile_ranges(n, tile)
    nt = len(base)
    if nt < 2:
        return {}
    out = {}
    for where, i in (("first", 0), ("middle", nt // 2), ("last", nt - 1)):
        out[f"the {where} tile twice"] = base[:i + 1] + base[i:]
        out[f"the {where} tile left out"] = base[:i] + base[i + 1:]
    i = nt // 2 if base[nt // 2][1] - base[nt // 2][0] > 16 else nt // 2 - 1
    t0, t1 = base[i]
    out["a 16-token half left out"] = base[:i] + [(t0, t0 + 16)] + base[i + 1:]
    x = t0 + 5
    out["a token left out"] = base[:i] + [(t0, x), (x + 1, t1)] + base[i + 1:]
    out["a token twice"] = base[:i + 1] + [(x, x + 1)] + base[i + 1:]
    return out


def window_split_cases(kind: str, cfg, splits: int) -> list[tuple[str, Problem]]:
    """:func:`split_lengths` in batches of five, as :func:`split_cases` has them, as window cases at G = 16."""
    return [(f"windows, lengths {lens}", window_problem(kind, 16, 16, lens, **fp8_scales(kind)))
            for lens in chunks(split_lengths(cfg, splits))]


def negative_cases(kind: str) -> list[tuple[str, Problem]]:
    """Every score strictly negative (G = 8): one tile, ragged tiles, more than one wave's tiles, the steady loop."""
    return [(f"negative scores, lengths {lens}", window_problem(kind, 8, 16, lens, negative=True, **fp8_scales(kind)))
            for lens in ((1, 17, 33, 100, 600), (2033, 129))]


# Head counts, page sizes and groups no other case has: (Hkv, page, G, lengths around a tile and a page boundary)
OTHER_SHAPES = (
    (1, 32, 3, (31, 33, 63, 65, 129)),
    (3, 48, 7, (47, 49, 95, 97, 145)),
    (8, 128, 12, (127, 129, 257)),
    (3, 256, 12, (255, 257, 513)),
    (8, 32, 7, (0, 1, 64, 97)),
)


def other_shape_cases(kind: str) -> list[tuple[str, Problem]]:
    """``OTHER_SHAPES`` as window cases and as selection cases (addressing: a row of V names its page and slot)."""
    out = []
    for hkv, page, g, lens in OTHER_SHAPES:
        name = f"Hkv {hkv}, page {page}, G {g}, lengths {lens}"
        out.append((f"windows, {name}", window_problem(kind, g, page, lens, hkv=hkv, **fp8_scales(kind))))
        out.append((f"selection, {name}", selection_problem(kind, g, page, lens, hkv=hkv, **fp8_scales(kind))))
    return out


def more_split_lengths(cfg: int, splits: int) -> list[int]:
    """The lengths of a split count of ``MORE_SPLITS``: 1, W + 1 and 2 F W + 1 tiles per split (waves without a tile,
    a ragged round, the steady loop and its drain), the last tile ragged, and the three lengths of
    :func:`split_lengths` at which a split has no token, the last has one, and the last is one full tile."""
    _, w, f = CFGS[cfg]
    return sorted({n * splits * TILE - 15 for n in (1, w + 1, 2 * f * w + 1)}
                  | {(splits - 1) * TILE - 3, 3 * (splits - 1) * TILE + 1, 3 * (splits - 1) * TILE + TILE})


LONG = 8192  # a sequence above this gets a problem of its own: no host tensor much above 70 MB


@functools.lru_cache(maxsize=8)
def _window_case(kind: str, lens: tuple) -> Problem:
    return window_problem(kind, 16, 16, lens, **fp8_scales(kind))


def more_split_cases(kind: str, cfg: int, splits: int) -> list[tuple[str, Problem]]:
    """:func:`more_split_lengths` as window cases at G = 16, Hkv = 2: the lengths up to ``LONG`` in one batch, every
    longer one alone.  Configurations share lengths, so the last few problems are kept."""
    lens = more_split_lengths(cfg, splits)
    groups = [tuple(n for n in lens if n <= LONG), *((n,) for n in lens if n > LONG)]
    return [(f"windows, lengths {list(group)}", _window_case(kind, group)) for group in groups if group]


# The dispatcher at the smallest shapes where each of its rules decides: (name, Hkv, G, page, lengths, max_seq_len,
# the split count).  max_seq_len alone sets the count; one sequence is that long (less 15 tokens: a ragged last tile),
# the others are short, so the caches stay small.
DISPATCH_SHAPES = (
    ("the workload's default, 64 pairs", 8, 8, 16, (8177, 5, 0, 100, 33, 1, 700, 64), 8192, 4),
    ("2 pairs, 4 tiles per wave decide", 2, 16, 64, (8177,), 8192, 8),
    ("8 pairs, the profile's headline", 2, 8, 256, (40, 32753, 0, 300), 32768, 32),
    ("7 pairs, an odd count", 1, 16, 256, (17, 37873, 0, 1, 255, 257, 90), 37888, 37),
    ("4 pairs, the maximum", 1, 16, 256, (1, 65521, 64, 0), 65536, 64),
    ("3 pairs, 86 wanted", 1, 16, 256, (100, 65521, 7), 65536, 64),
)


def dispatch_cases(shape) -> dict[str, list[tuple[str, Problem]]]:
    """A window case and a selection case (targets on both sides of every cut of the dispatched split count) of one
    row of ``DISPATCH_SHAPES``, per cache type; the e4m3 ones are the bf16 ones stored as e4m3."""
    name, hkv, g, page, lens, max_seq_len, splits = shape
    assert pick(len(lens) * hkv, max_seq_len) == splits
    both = [(f"windows, {name}", window_problem("bf16", g, page, lens, hkv=hkv, max_seq_len=max_seq_len)),
            (f"selection, {name}", selection_problem("bf16", g, page, lens, hkv=hkv, max_seq_len=max_seq_len,
                                                     cuts=[split_cuts(n, splits) for n in lens]))]
    return {"bf16": both, "fp8": [(what, to_fp8(p)) for what, p in both]}


# ---- the contract's clamps and the e4m3 codes ---------------------------------------------------------------------

def _raw(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.uint8) if t.dtype == FP8 else t.view(torch.int16)


def page_clamp_problem(kind: str) -> Problem:
    """A page index at or above ``num_pages`` names page ``num_pages - 1``.  A selection case in which the block-table
    entry of a page in use (tokens 48 .. 63 of sequence 0, between two other pages of it) is ``num_pages + 1`` and that
    page's data lies in physical page ``num_pages - 1``; the caches hold three pages more than ``num_pages`` counts
    (``Problem.beyond``), all poison.  A kernel that clamps is exact; one that does not reads poison inside the
    allocation and fails the comparison, and nothing can fault.  A NEGATIVE page index is not tested: the unsigned
    minimum turns it into the last page as well, but a kernel without the clamp would read in front of the caches."""
    p = selection_problem(kind, 8, 16, [100, 37, 64], **fp8_scales(kind))
    n, b, entry = p.num_pages, 0, 3
    moved, spare = int(p.block_table[b, entry]), int(p.block_table[1, -1])  # spare: a poison page (37 tokens: 3 pages)
    assert p.table_stride > 3 and bool(torch.isnan(p.v_cache[spare].float()).all())
    perm = torch.arange(n)
    perm[moved], perm[n - 1] = n - 1, moved  # the new page j holds the old page perm[j]
    table = p.block_table.clone()
    table[p.block_table == n - 1] = moved
    table[b, entry] = n + 1
    caches = [_raw(c)[torch.cat([perm, torch.full((3,), spare)])].view(c.dtype) for c in (p.k_cache, p.v_cache)]
    return dataclasses.replace(p, k_cache=caches[0], v_cache=caches[1], block_table=table, beyond=3)


def fp8_codes_problem() -> tuple[Problem, np.ndarray]:
    """Every e4m3 code in V: ``(problem, codes[32][128])``.  A selection case of one sequence at G = 16, Hkv = 2 whose
    32 heads target 32 different tokens; the target row of head j holds ``codes[j]``, in which each of the 254
    codes that are no NaN stands at each of the 16 byte positions of a 16-B chunk (0x7F and 0xFF, the NaNs, are
    replaced by 0x7E and 0xFE), subnormals, -0 and 448 among them.  Every other token holds other finite codes.
    ``want`` is the value times ``v_scale``, exact in bf16; code 0x80 is -0 and the accumulate makes +0 of it, so
    zeros are compared by value.  K is converted by the same function as V and the random cases test where its
    operands land, so K has no sweep of its own."""
    g, hkv, page, n = 16, 2, 16, 261
    p = selection_problem("fp8", g, page, [n], **fp8_scales("fp8"))
    hit = targets(p)[0]
    assert len(set(hit)) == g * hkv
    def finite(x):  # 0x7F and 0xFF, the NaNs, become 0x7E and 0xFE
        return np.where(x % 128 == 127, x - 1, x).astype(np.uint8)

    j, d = np.meshgrid(np.arange(g * hkv), np.arange(D), indexing="ij")
    codes = finite((8 * j + d // 16 + 37 * (d % 16)) % 256)
    t = np.arange(n)
    pp, slot = p.block_table[0].numpy()[t // page].astype(np.int64), t % page
    v = p.v_cache.view(torch.uint8).clone()
    for h in range(hkv):
        v[pp, h, slot] = torch.from_numpy(finite((29 * t[:, None] + 11 * np.arange(D)[None] + 7 * h) % 256))
        for i in range(g):
            tok = hit[h * g + i]
            v[pp[tok], h, slot[tok]] = torch.from_numpy(codes[h * g + i])
    want = (torch.from_numpy(codes).view(FP8).float() * p.v_scale).bfloat16()[None]
    return dataclasses.replace(p, v_cache=v.view(FP8), want=want), codes


# ---- random cases -------------------------------------------------------------------------------------------------

def random_problem(kind: str, seed: int, g: int, page: int, lens, qscale: float, hkv: int = 2) -> Problem:
    """N(0, 1) K and V (rounded to the cache type), Q = N(0, 1) * qscale, pages handed out through a random
    permutation; unowned slots and three spare pages hold NaN."""
    gen = torch.Generator().manual_seed(seed)
    lens = list(lens)
    nb, hq = len(lens), g * hkv
    npages = [-(-n // page) for n in lens]
    total = sum(npages) + POISON_PAGES
    perm = torch.randperm(total, generator=gen).numpy()
    stride = max(npages + [1])
    table = np.empty((nb, stride), dtype=np.int32)
    k = torch.full((total, hkv, page, D), float("nan"))
    v = torch.full((total, hkv, page, D), float("nan"))
    at = 0
    for b, n in enumerate(lens):
        table[b] = perm[-1 - b % POISON_PAGES]
        table[b, :npages[b]] = perm[at:at + npages[b]]
        at += npages[b]
        t = np.arange(n)
        pp, slot = table[b][t // page].astype(np.int64), t % page
        k[pp, :, slot] = torch.randn(n, hkv, D, generator=gen)
        v[pp, :, slot] = torch.randn(n, hkv, D, generator=gen)
    q = (torch.randn(nb, hq, D, generator=gen) * qscale).bfloat16()
    scales = {} if kind == "bf16" else {"k_scale": 0.5, "v_scale": 1.5}
    kc, vc = (k.bfloat16(), v.bfloat16()) if kind == "bf16" else ((k / 0.5).to(FP8), (v / 1.5).to(FP8))
    return Problem(kind, q, kc, vc, torch.from_numpy(table), torch.tensor(lens, dtype=torch.int32), max(lens),
                   1.0 / math.sqrt(D), **scales)


def error_bound(p: Problem) -> tuple[np.ndarray, float, float]:
    """``(bound[B][Hq][D], two_ln2_dx, worst f / (u / 4 max |v|))`` of the module docstring, in fp64, against
    :func:`reference`.  A sequence of length 0 has bound 0: its row is exactly zero."""
    ref = reference(p)
    q = np.abs(p.q.to(torch.float64).numpy()).reshape(p.b, p.hkv, p.g, D)
    c = p.scale * LOG2E  # k is gathered dequantised: k_scale is in it
    s_max, vmax = 0.0, np.zeros((p.b, p.hkv, 1, D))
    for b, n in enumerate(p.lens()):
        if n:
            k, v = p.gather(b)
            s_max = max(s_max, float(np.einsum("hgd,htd->hgt", q[b], np.abs(k)).max()))
            vmax[b, :, 0] = np.abs(v).max(axis=1)
    t = max(p.lens())
    dx = (D + 2) * EPS * s_max * c + 2 * EPS * s_max * c + (t + 4) * EPS / math.log(2)
    rel = 2 * math.log(2) * dx
    vm = np.broadcast_to(vmax, (p.b, p.hkv, p.g, D)).reshape(p.b, p.hq, D)
    return U * vm + U * np.abs(ref) + rel * vm, rel, rel / (U / 4)


RANDOM_CASES = (  # (seed, G, page, lengths, q scale)
    (1, 8, 16, (600, 0, 33, 257, 1), 1.0),
    (2, 16, 64, (513, 64, 17), 0.5),
    (3, 4, 16, (1100, 95), 2.0),
    (4, 1, 64, (300, 31, 2), 2.0),
)
# Graded merge weights at 16, 32 and 64 splits (the window cases' are 0 or 1).  4096 tokens, two tiles to a split of
# 64, is the longest length this case may have: there f is still below u / 4 max |v| and the twin inside the bound.
RANDOM_MORE = (5, 8, 16, (4096, 45), 1.0)
RANDOM_MORE_SPLITS = (16, 32, 64)


def bits(t: torch.Tensor) -> torch.Tensor:
    """The raw 16 bits of a bf16 tensor, as int32 in 0..0xFFFF."""
    assert t.dtype == torch.bfloat16
    return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def assert_bits_equal(got: torch.Tensor, want: torch.Tensor, what: str, zeros_by_value: bool = False) -> None:
    """``zeros_by_value``: -0 and +0 count as equal; every other element has to match in all 16 bits."""
    g, w = bits(got.cpu()), bits(want)
    if zeros_by_value:
        g, w = g.masked_fill(g == 0x8000, 0), w.masked_fill(w == 0x8000, 0)
    bad = (g != w).nonzero()
    if len(bad):
        b, h, d = (int(x) for x in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.numel()} elements differ; first at sequence {b}, head {h}, "
                             f"d {d}: got {int(g[b, h, d]):#06x}, want {int(w[b, h, d]):#06x}")
