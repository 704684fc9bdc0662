"""Problems for the decode attention tests (native/kernels/attn_decode.hip): one new token per sequence, grouped-query
attention over a paged KV cache in bf16 or e4m3, D = 128.

Plain Python on torch and NumPy, no GPU.  Three things live here:

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
DISPATCHED = 2  # the configuration gsx_decode_attn runs (attn_pick() in attn_decode.hip)


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
        return self.page_base + self.k_cache.shape[0]

    @property
    def table_stride(self) -> int:
        return self.block_table.shape[1]

    def lens(self) -> list[int]:
        """The lengths the kernel uses: ``seq_lens`` clamped to ``max_seq_len``."""
        return [min(max(int(x), 0), self.max_seq_len) for x in self.seq_lens]

    def gather(self, b: int, dtype=np.float64, scaled: bool = True) -> tuple[np.ndarray, np.ndarray]:
        """``K[Hkv][len][D]`` and ``V[Hkv][len][D]`` of sequence ``b``, through its block table: dequantised, or
        (``scaled=False``) the stored values."""
        n = self.lens()[b]
        t = np.arange(n)
        pages = self.block_table[b].numpy()[t // self.page] - self.page_base
        slots = t % self.page
        k = self.k_cache[pages, :, slots].to(torch.float64).numpy() * (self.k_scale if scaled else 1.0)
        v = self.v_cache[pages, :, slots].to(torch.float64).numpy() * (self.v_scale if scaled else 1.0)  # [len][Hkv][D]
        return k.transpose(1, 0, 2).astype(dtype), v.transpose(1, 0, 2).astype(dtype)


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


def twin(p: Problem, tile: int = TILE) -> torch.Tensor:
    """The contract in NumPy, fp32 throughout, in tiles of ``tile`` tokens: bf16 ``[B][Hq][D]``."""
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
        for t0 in range(0, n, tile):
            kt, vt = k[:, t0:t0 + tile], v[:, t0:t0 + tile]
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
                      k_scale: float = 1.0, v_scale: float = 1.0, page_base: int = 0) -> Problem:
    """A selection case (module docstring) of ``len(lens)`` sequences.  The ``g * hkv`` heads of sequence b target
    the tokens of :func:`pick_targets` (``cuts``: per sequence, the first tokens of its splits), dealt to the KV heads
    in turn, the turn starting one KV head later every round (entry i goes to KV head ``(i + i // hkv) % hkv``): the
    two sides of a cut go to different KV heads, each KV head gets left sides and right sides, and each has targets
    along the whole sequence.  ``tables``: how physical pages are
    handed out; ``shared``: sequence 1 has sequence 0's block table (and must have its length); ``over``: sequences
    whose ``seq_lens`` entry is raised above ``max_seq_len``, which the kernel clamps; ``extra_stride``: columns of
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
    batch that mixes 0 and short lengths with ``max_seq_len``, and ``seq_lens`` above ``max_seq_len``."""
    fs = fp8_scales(kind)
    return [
        ("reversed", selection_problem(kind, 4, 16, [100, 37, 64], tables="reversed", **fs)),
        ("scattered, page 64", selection_problem(kind, 8, 64, [300, 65, 129], tables="scattered", **fs)),
        ("shared", selection_problem(kind, 16, 16, [90, 90, 40], shared=True, **fs)),
        ("stride + 5", selection_problem(kind, 2, 16, [33, 70, 1], extra_stride=5, **fs)),
        ("mixed", selection_problem(kind, 4, 16, [0, 1100, 5, 0, 1100], max_seq_len=1100, **fs)),
        ("clamped", selection_problem(kind, 4, 16, [75, 20, 75], max_seq_len=75, over=(0, 2), **fs)),
    ]


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


def bits(t: torch.Tensor) -> torch.Tensor:
    """The raw 16 bits of a bf16 tensor, as int32 in 0..0xFFFF."""
    assert t.dtype == torch.bfloat16
    return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def assert_bits_equal(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    g, w = bits(got.cpu()), bits(want)
    bad = (g != w).nonzero()
    if len(bad):
        b, h, d = (int(x) for x in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.numel()} elements differ; first at sequence {b}, head {h}, "
                             f"d {d}: got {int(g[b, h, d]):#06x}, want {int(w[b, h, d]):#06x}")
