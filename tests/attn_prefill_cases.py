"""Problems for the prefill attention tests (native/kernels/attn_prefill.hip): T new tokens per sequence attend,
causally, over a paged KV cache in bf16 or e4m3, D = 128.

Plain Python on torch and NumPy, no GPU.  Built on ``tests/attn_decode_cases.py`` (the cache layout, ``gather``, the
page orders, the V rows that name their place, the error bound's terms) and ``tests/kv_append_cases.py`` (the chained
case).  What lives here:

* :func:`reference`, the causal attention in fp64, and :func:`twin`, a NumPy transcription of the numeric contract in
  ``gsx_kernels.h`` for any tile size: fp32 scores times ``scale * k_scale * log2 e``, a token the row may not see
  replaced by -inf, ``exp2`` against a running maximum, ``l`` from the unrounded probabilities, P rounded to bf16 for
  the PV product, one rounding of ``(acc / l) * v_scale``;
* :func:`error_bound`: that of ``attn_decode_cases`` with the token count of a row equal to ``pos + 1`` and the
  largest ``|v|`` taken over the tokens the row sees;
* **staircase cases** (:func:`staircase_problem`), exact: every query is ``(2^11, 2^11, 0, ..)`` and token j has
  ``k_j = (j % 16, 16 * (j // 16), 0, ..)``, exact in bf16 for j < 4096 and in e4m3 for j < 256.  With
  ``scale = 128^-0.5`` the ``exp2`` argument rises by 261.2 per token, so the row's own position has probability
  exactly 1 and every earlier token exactly 0 (fp32 ``exp2(-261)`` is 0): O is row ``pos`` of V bit for bit.  V holds
  the small integers of ``attn_decode_cases.v_rows``.  A mask off by one upwards returns row ``pos + 1``, one that
  drops the diagonal row ``pos - 1``, a skipped or doubled tile another row or a scaled one;
* **count cases** (:func:`count_problem`): Q = 0 and V one-hot in column ``j % 128``, so ``O[row][d]`` is the number
  of visible tokens with ``j % 128 == d`` over ``pos + 1``; a token counted twice, missed or leaked from the future
  moves an element by ``1 / (pos + 1)``, far outside the bound;
* **random cases** (:func:`random_problem`).

Poison: slots at or past ``base + T`` and pages nobody owns hold a K that would win the softmax (``(255, 3840, 0, ..)``
in bf16, ``(448, 448, 0, ..)`` in e4m3) and V = NaN.  Unused block-table entries name a poison page, never an index
out of range: a wrong kernel fails a comparison and does not fault.
"""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np
import torch

from tests import attn_decode_cases as ac
from tests import kv_append_cases as kc

D = ac.D
KINDS = ac.KINDS
FP8 = ac.FP8
U, EPS, LOG2E = ac.U, ac.EPS, ac.LOG2E
POISON_PAGES = ac.POISON_PAGES

# the library's table (gsx_prefill_attn_cfg_name / _cfg_shape): name, query rows per workgroup, tokens per KV tile,
# waves per workgroup.  The GPU test asserts that the library says the same.
CFGS = {0: ("8w-q256-k64", 256, 64, 8)}
Q_ROWS, KV_TILE = CFGS[0][1], CFGS[0][2]


@dataclasses.dataclass(frozen=True)
class Problem:
    """One launch.  ``q`` is bf16 ``[B * T][Hq][D]``; the caches, ``block_table`` and ``max_seq_len`` as in
    ``attn_decode_cases.Problem``; ``seq_lens`` int32 ``[B]`` holds the lengths BEFORE the chunk.  ``want`` is the exact
    bf16 result ``[B * T][Hq][D]`` of a staircase case, None otherwise.  Tensors are shared: not to be written to."""
    kind: str
    q: torch.Tensor
    k_cache: torch.Tensor
    v_cache: torch.Tensor
    block_table: torch.Tensor
    seq_lens: torch.Tensor
    t: int
    max_seq_len: int
    scale: float
    k_scale: float = 1.0
    v_scale: float = 1.0
    want: torch.Tensor | None = None
    beyond: int = 0  # pages at the end of the caches that ``num_pages`` does not count

    @property
    def b(self) -> int:
        return self.seq_lens.shape[0]

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
        return self.k_cache.shape[0] - self.beyond

    @property
    def table_stride(self) -> int:
        return self.block_table.shape[1]

    def bases(self) -> list[int]:
        """The lengths the kernel starts from: ``seq_lens`` clamped to ``[0, max_seq_len]``."""
        return [min(max(int(x), 0), self.max_seq_len) for x in self.seq_lens]

    def live(self) -> list[int]:
        """Live rows per sequence: row t is live when ``base + t < max_seq_len``."""
        return [max(0, min(self.t, self.max_seq_len - x)) for x in self.bases()]

    def cache(self) -> ac.Problem:
        """The caches after the chunk as a decode problem of lengths ``base + live rows``: for its ``gather``."""
        ends = torch.tensor([x + n for x, n in zip(self.bases(), self.live())], dtype=torch.int32)
        return ac.Problem(self.kind, self.q[:self.b], self.k_cache, self.v_cache, self.block_table, ends,
                          self.max_seq_len, self.scale, self.k_scale, self.v_scale, beyond=self.beyond)

    def as_decode(self) -> ac.Problem:
        """A T == 1 problem as the decode attention takes it: lengths ``base + 1``."""
        assert self.t == 1 and all(n == 1 for n in self.live())
        return dataclasses.replace(self.cache(), q=self.q)


def reference(p: Problem) -> np.ndarray:
    """The causal attention in fp64, ``[B * T][Hq][D]``; a row that is not live gives zeros."""
    out = np.zeros((p.b * p.t, p.hq, D))
    q = p.q.to(torch.float64).numpy().reshape(p.b, p.t, p.hkv, p.g, D)
    cache = p.cache()
    for b, (base, n) in enumerate(zip(p.bases(), p.live())):
        if n == 0:
            continue
        k, v = cache.gather(b)
        x = np.einsum("thgd,hjd->thgj", q[b, :n], k) * p.scale
        seen = np.arange(base + n)[None, :] <= (base + np.arange(n))[:, None]  # [t][j]
        x = np.where(seen[:, None, None, :], x, -np.inf)
        w = np.exp(x - x.max(axis=3, keepdims=True))
        w /= w.sum(axis=3, keepdims=True)
        out[b * p.t:b * p.t + n] = np.einsum("thgj,hjd->thgd", w, v).reshape(n, p.hq, D)
    return out


def twin(p: Problem, tile: int = KV_TILE, wrong: str | None = None) -> torch.Tensor:
    """The contract in NumPy, fp32 throughout, in tiles of ``tile`` tokens from token 0: bf16 ``[B * T][Hq][D]``.
    ``wrong``, for the tests of the tests: "above" (the mask lets the next token through), "no diagonal" (a row does
    not see its own token), "skip" (the second tile is left out), "twice" (it is taken twice; a staircase case
    cannot see that, l and the accumulator double together, a count case does)."""
    out = np.zeros((p.b * p.t, p.hq, D), dtype=np.float32)
    q = p.q.float().numpy().reshape(p.b, p.t, p.hkv, p.g, D)
    c = np.float32(np.float32(np.float32(p.scale) * np.float32(p.k_scale)) * np.float32(LOG2E))
    cache = p.cache()
    shift = {"above": 1, "no diagonal": -1}.get(wrong, 0)
    for b, (base, n) in enumerate(zip(p.bases(), p.live())):
        if n == 0:
            continue
        k, v = cache.gather(b, np.float32, scaled=False)
        pos = base + np.arange(n) + shift
        m = np.full((n, p.hkv, p.g), -np.inf, dtype=np.float32)
        l = np.zeros((n, p.hkv, p.g), dtype=np.float32)
        acc = np.zeros((n, p.hkv, p.g, D), dtype=np.float32)
        tiles = ac.tile_ranges(base + n, tile)
        if wrong == "skip":
            tiles = tiles[:1] + tiles[2:]
        if wrong == "twice":
            tiles = tiles[:2] + tiles[1:]
        for j0, j1 in tiles:
            kt, vt = k[:, j0:j1], v[:, j0:j1]
            x = (np.einsum("thgd,hjd->thgj", q[b, :n], kt).astype(np.float32) * c).astype(np.float32)
            x = np.where((np.arange(j0, j1)[None, :] <= pos[:, None])[:, None, None, :], x, np.float32(-np.inf))
            mn = np.maximum(m, x.max(axis=3))
            ms = np.where(np.isinf(mn), np.float32(0), mn)
            alpha = np.exp2(m - ms).astype(np.float32)
            pr = np.exp2(x - ms[..., None]).astype(np.float32)
            l = (l * alpha + pr.sum(axis=3, dtype=np.float32)).astype(np.float32)
            acc = acc * alpha[..., None] + np.einsum("thgj,hjd->thgd", ac._bf16_round(pr), vt).astype(np.float32)
            m = mn
        with np.errstate(invalid="ignore", divide="ignore"):
            o = ((acc / l[..., None]).astype(np.float32) * np.float32(p.v_scale)).astype(np.float32)
        out[b * p.t:b * p.t + n] = np.where(l[..., None] > 0, o, 0).reshape(n, p.hq, D)
    return ac.to_bf16(out)


def error_bound(p: Problem) -> tuple[np.ndarray, np.ndarray, float]:
    """``(bound[B * T][Hq][D], reference, worst f / (u / 4 max |v|))``: the bound of ``attn_decode_cases`` per row,
    with ``pos + 1`` tokens in the fp32 term and the largest ``|v[j][d]|`` over the tokens j <= pos the row sees.  A
    row that is not live has bound 0: it is exactly zero."""
    ref = reference(p)
    bound = np.zeros_like(ref)
    q = np.abs(p.q.to(torch.float64).numpy()).reshape(p.b, p.t, p.hkv, p.g, D)
    c = p.scale * LOG2E  # k is gathered dequantised: k_scale is in it
    cache = p.cache()
    worst = 0.0
    kv = {b: cache.gather(b) for b, n in enumerate(p.live()) if n}
    # S, the largest sum of |q_d k_d|, is taken over the whole case, as attn_decode_cases takes it
    s_max = max((float(np.einsum("thgd,hjd->thgj", q[b, :p.live()[b]], np.abs(k)).max()) for b, (k, _) in kv.items()),
                default=0.0)
    for b, (base, n) in enumerate(zip(p.bases(), p.live())):
        if n == 0:
            continue
        k, v = kv[b]
        vmax = np.maximum.accumulate(np.abs(v), axis=1)[:, base:base + n]  # [Hkv][t][D]: over tokens 0 .. pos
        tokens = base + np.arange(n) + 1
        dx = (D + 2) * EPS * s_max * c + 2 * EPS * s_max * c + (tokens + 4) * EPS / math.log(2)
        rel = 2 * math.log(2) * dx  # [t]
        vm = np.broadcast_to(vmax.transpose(1, 0, 2)[:, :, None, :], (n, p.hkv, p.g, D)).reshape(n, p.hq, D)
        rows = slice(b * p.t, b * p.t + n)
        bound[rows] = U * vm + U * np.abs(ref[rows]) + rel[:, None, None] * vm
        worst = max(worst, float(rel.max()) / (U / 4))
    return bound, ref, worst


# ---- layout ------------------------------------------------------------------------------------------------------------

def _poison_k(kind: str) -> np.ndarray:
    row = np.zeros(D, dtype=np.float32)
    row[:2] = (255, 3840) if kind == "bf16" else (448, 448)
    return row


def _layout(page: int, ends, max_seq_len: int, tables: str, extra_stride: int, seed: int | None, clamp):
    """``(table[B][stride], total pages, beyond)``.  Sequence b owns the pages of its tokens ``0 .. ends[b] - 1``; every
    other entry names one of ``POISON_PAGES`` pages nobody owns.  ``tables``: a page order of ``attn_decode_cases``, or
    "random" (a permutation from ``seed``).  ``clamp = (b, column)``: that page's data lies in the LAST page that
    ``num_pages`` counts, its table entry says ``num_pages + 1``, and three more poison pages follow in the caches."""
    npages = [-(-n // page) for n in ends]
    used = sum(npages)
    total = used + POISON_PAGES
    if tables == "random":
        order = np.random.default_rng(seed).permutation(total)
    else:
        order = ac._page_order(total, tables).copy()
    stride = max(-(-max_seq_len // page), 1) + extra_stride
    if clamp is not None:
        at = sum(npages[:clamp[0]]) + clamp[1]
        assert clamp[1] < npages[clamp[0]]
        (last,) = np.nonzero(order == total - 1)[0]
        order[[at, last]] = order[[last, at]]
    poison = [int(x) for x in order[used:]]
    table = np.empty((len(ends), stride), dtype=np.int32)
    at = 0
    for b, n in enumerate(npages):
        table[b] = [poison[(b + i) % POISON_PAGES] for i in range(stride)]
        table[b, :n] = order[at:at + n]
        at += n
    return table, total, (3 if clamp is not None else 0)


def _assemble(kind: str, g: int, hkv: int, page: int, t: int, bases, q: np.ndarray, kfun, vfun, *,
              max_seq_len: int | None = None, tables: str = "scattered", extra_stride: int = 0, seed: int | None = None,
              seq_lens=None, clamp=None, k_scale: float = 1.0, v_scale: float = 1.0, want=None,
              poison_k: np.ndarray | None = None) -> Problem:
    """``kfun(b, h, j, pp, slot)`` and ``vfun(..)`` give the stored rows ``[len(j)][D]`` of tokens ``j`` of sequence b,
    KV head h, which lie at (physical page ``pp``, ``slot``).  ``seq_lens``: the raw entries, where they differ from
    ``bases`` (values the kernel clamps)."""
    bases = list(bases)
    nb = len(bases)
    max_seq_len = max(max(x + t for x in bases), 1) if max_seq_len is None else max_seq_len
    assert all(0 <= x <= max_seq_len for x in bases)
    ends = [min(x + t, max_seq_len) for x in bases]
    table, total, beyond = _layout(page, ends, max_seq_len, tables, extra_stride, seed, clamp)
    k = np.empty((total + beyond, hkv, page, D), dtype=np.float32)
    v = np.full((total + beyond, hkv, page, D), np.nan, dtype=np.float32)
    k[:] = _poison_k(kind) if poison_k is None else poison_k
    for b, n in enumerate(ends):
        j = np.arange(n)
        pp, slot = table[b][j // page].astype(np.int64), j % page
        for h in range(hkv):
            k[pp, h, slot] = kfun(b, h, j, pp, slot)
            v[pp, h, slot] = vfun(b, h, j, pp, slot)
    if clamp is not None:
        table[clamp] = total + 1
    kt, vt = torch.from_numpy(k), torch.from_numpy(v)
    kt, vt = (kt.bfloat16(), vt.bfloat16()) if kind == "bf16" else (kt.to(FP8), vt.to(FP8))
    lens = np.array(bases if seq_lens is None else seq_lens, dtype=np.int64).astype(np.int32)
    p = Problem(kind, ac.to_bf16(q), kt, vt, torch.from_numpy(table), torch.from_numpy(lens), t, max_seq_len,
                (1.0 / math.sqrt(D)) / k_scale, k_scale, v_scale, None, beyond)
    assert p.bases() == bases
    return p if want is None else dataclasses.replace(p, want=ac.to_bf16(want(p, table)))


def fp8_scales(kind: str) -> dict:
    return ac.fp8_scales(kind)


def staircase_problem(kind: str, g: int, page: int, t: int, bases, *, hkv: int = 2, **kw) -> Problem:
    """A staircase case (module docstring): ``len(bases)`` sequences of ``t`` new tokens behind ``bases[b]`` tokens."""
    top = 4096 if kind == "bf16" else 256
    q = np.zeros((len(list(bases)) * t, g * hkv, D), dtype=np.float32)
    q[:, :, :2] = 2.0 ** 11

    def kfun(b, h, j, pp, slot):
        assert j.max(initial=0) < top, "a staircase case is exact below this many tokens only"
        rows = np.zeros((len(j), D), dtype=np.float32)
        rows[:, 0], rows[:, 1] = j % 16, 16 * (j // 16)
        return rows

    def vfun(b, h, j, pp, slot):
        return ac.v_rows(pp, h, slot, page, hkv)

    def want(p, table):
        out = np.zeros((p.b * t, p.hq, D), dtype=np.float32)
        for b, (base, n) in enumerate(zip(p.bases(), p.live())):
            pos = base + np.arange(n)
            pp = np.minimum(table[b][pos // page], p.num_pages - 1).astype(np.int64)
            for h in range(hkv):
                rows = ac.v_rows(pp, h, pos % page, page, hkv) * p.v_scale
                out[b * t:b * t + n, h * g:(h + 1) * g] = rows[:, None, :]
        return out

    return _assemble(kind, g, hkv, page, t, bases, q, kfun, vfun, want=want, **kw)


def count_problem(kind: str, g: int, page: int, t: int, bases, *, hkv: int = 2, **kw) -> Problem:
    """A count case (module docstring).  K holds small integers that differ from token to token; with Q = 0 none of
    them matters, and a kernel that read Q from the wrong place would show."""
    q = np.zeros((len(list(bases)) * t, g * hkv, D), dtype=np.float32)

    def kfun(b, h, j, pp, slot):
        return (1 + (j[:, None] + 3 * np.arange(D)[None, :] + h) % 7).astype(np.float32)

    def vfun(b, h, j, pp, slot):
        rows = np.zeros((len(j), D), dtype=np.float32)
        rows[np.arange(len(j)), j % D] = 1.0
        return rows

    return _assemble(kind, g, hkv, page, t, bases, q, kfun, vfun, **kw)


def random_problem(kind: str, seed: int, g: int, page: int, t: int, bases, *, hkv: int = 2, qscale: float = 1.0) -> Problem:
    """N(0, 1) K and V (rounded to the cache type), Q = N(0, 1) * qscale, pages handed out through a random
    permutation; unowned slots and the spare pages hold NaN in K and in V."""
    rng = np.random.default_rng(seed)
    bases = list(bases)
    q = rng.standard_normal((len(bases) * t, g * hkv, D)).astype(np.float32) * np.float32(qscale)
    scales = {} if kind == "bf16" else {"k_scale": 0.5, "v_scale": 1.5}

    def kfun(b, h, j, pp, slot):
        return (rng.standard_normal((len(j), D)) / scales.get("k_scale", 1.0)).astype(np.float32)

    def vfun(b, h, j, pp, slot):
        return (rng.standard_normal((len(j), D)) / scales.get("v_scale", 1.0)).astype(np.float32)

    p = _assemble(kind, g, hkv, page, t, bases, q, kfun, vfun, tables="random", seed=seed,
                  poison_k=np.full(D, np.nan, dtype=np.float32), **scales)
    return dataclasses.replace(p, scale=1.0 / math.sqrt(D))


# ---- the cases the GPU runs ----------------------------------------------------------------------------------------------

T_VALUES = (1, 17, Q_ROWS - 1, Q_ROWS, Q_ROWS + 1, 2 * Q_ROWS + 1)
BASES = (0, 1, 15, 16, KV_TILE - 1, KV_TILE, 200)
PAGES = (16, 64, 256)


def _spread(i: int, xs):
    return xs[i % len(xs)]


@functools.lru_cache(maxsize=None)
def staircase_cases(kind: str) -> list[tuple[str, Problem]]:
    """Every T of ``T_VALUES`` with every base of ``BASES`` (three or four sequences to a launch, so every launch has
    more than one base), pages of 16, 64 and 256 and G of 1, 4 and 16 (1, 2 and 4 for the long chunks) in turn.  An e4m3 case is exact below 256 tokens
    only: there T stops at 17 and the long chunks start from bases that keep the end below 256 (T = 255 from 0)."""
    fs = fp8_scales(kind)
    out = []
    i = 0
    for t in T_VALUES:
        for group in (BASES[:4], BASES[4:]):
            bases = list(group)
            if kind == "fp8":
                bases = [x for x in bases if x + t <= 255]
                if not bases:
                    continue
            # the long chunks take small groups: the CPU twin of a case stays below a second
            g, page = _spread(i, (4, 16, 1) if t <= 17 else (2, 1, 4)), _spread(i, PAGES)
            i += 1
            out.append((f"T {t}, bases {bases}, G {g}, page {page}",
                        staircase_problem(kind, g, page, t, bases, **fs)))
    if kind == "fp8":  # the longest chunk e4m3 holds: one block of query rows, every tile of it on the diagonal
        out.append(("T 255, base 0, G 4, page 64", staircase_problem(kind, 4, 64, 255, [0], **fs)))
        out.append(("T 100, bases [1, 155], G 16, page 16", staircase_problem(kind, 16, 16, 100, [1, 155], **fs)))
    return out


@functools.lru_cache(maxsize=None)
def count_cases(kind: str) -> list[tuple[str, Problem]]:
    """T around one and two blocks of query rows from bases around a tile, Hkv 1 and 2."""
    fs = fp8_scales(kind)
    return [
        (f"T {Q_ROWS + 1}, bases [0, 63, 200], G 4, page 16", count_problem(kind, 4, 16, Q_ROWS + 1, [0, 63, 200], **fs)),
        (f"T 17, bases [15, 64, 1], G 16, page 64", count_problem(kind, 16, 64, 17, [15, 64, 1], **fs)),
        (f"T {2 * Q_ROWS + 1}, base 16, G 1, page 256, Hkv 1",
         count_problem(kind, 1, 256, 2 * Q_ROWS + 1, [16], hkv=1, **fs)),
        (f"T {Q_ROWS - 1}, bases [0, 200], G 2, page 16", count_problem(kind, 2, 16, Q_ROWS - 1, [0, 200], **fs)),
    ]


RANDOM_CASES = (  # (seed, G, Hkv, page, T, bases, q scale)
    (1, 4, 2, 16, Q_ROWS + 1, (0, 63, 200), 1.0),
    (2, 16, 1, 64, 17, (15, 64, 1), 0.5),
    (3, 1, 2, 256, 2 * Q_ROWS + 1, (16,), 2.0),
    (4, 4, 1, 16, Q_ROWS - 1, (1,), 1.0),
    (5, 1, 1, 64, 1, (200, 0, 64), 2.0),
    (6, 16, 2, 16, Q_ROWS, (63,), 1.0),
)


@functools.lru_cache(maxsize=None)
def random_cases(kind: str) -> list[tuple[str, Problem]]:
    return [(f"seed {s}, G {g}, Hkv {hkv}, page {page}, T {t}, bases {list(bases)}",
             random_problem(kind, s, g, page, t, bases, hkv=hkv, qscale=qs))
            for s, g, hkv, page, t, bases, qs in RANDOM_CASES]


@functools.lru_cache(maxsize=None)
def dead_row_cases(kind: str) -> list[tuple[str, Problem]]:
    """Rows past ``max_seq_len`` (zeros), ``seq_lens`` above ``max_seq_len`` and below 0 (clamped), a table stride wider
    than needed, and a page index past ``num_pages`` (the last page)."""
    fs = fp8_scales(kind)
    return [
        ("T 40 runs past max_seq_len 100", staircase_problem(kind, 4, 16, 40, [90, 61, 100, 0], max_seq_len=100, **fs)),
        ("seq_lens above max_seq_len and below 0",
         staircase_problem(kind, 4, 16, 17, [80, 0, 0, 30], max_seq_len=80, seq_lens=[1080, -1, -2 ** 31, 30], **fs)),
        ("a wider table, reversed", staircase_problem(kind, 16, 64, 70, [3, 130], tables="reversed", extra_stride=5,
                                                      **fs)),
        ("a page index past num_pages", staircase_problem(kind, 8, 16, 40, [50, 7], clamp=(0, 3), **fs)),
    ]


def t1_cases(kind: str) -> list[tuple[str, Problem]]:
    """T == 1 on random data: the decode attention's problem on lengths ``base + 1``."""
    return [(name, p) for name, p in random_cases(kind) if p.t == 1] + \
        [("seed 7, T 1, bases [599, 31, 0, 256]", random_problem(kind, 7, 8, 16, 1, (599, 31, 0, 256)))]


def all_cases(kind: str) -> list[tuple[str, Problem]]:
    return [*staircase_cases(kind), *count_cases(kind), *random_cases(kind), *dead_row_cases(kind), *t1_cases(kind)[-1:]]


def split_chunk(p: Problem, t1: int) -> tuple[Problem, Problem]:
    """The chunk of ``p`` as two launches over the same caches: rows ``0 .. t1 - 1`` from the same bases, then the rest
    from ``base + t1``.  No row is past ``max_seq_len``."""
    assert 0 < t1 < p.t and all(n == p.t for n in p.live())
    q = p.q.reshape(p.b, p.t, p.hq, D)
    first = dataclasses.replace(p, q=q[:, :t1].reshape(-1, p.hq, D).contiguous(), t=t1, want=None)
    later = torch.tensor([x + t1 for x in p.bases()], dtype=torch.int32)
    second = dataclasses.replace(p, q=q[:, t1:].reshape(-1, p.hq, D).contiguous(), t=p.t - t1, seq_lens=later,
                                 want=None)
    return first, second


def alone(p: Problem, b: int) -> Problem:
    """Sequence ``b`` of ``p`` as a launch of its own over the same caches."""
    return dataclasses.replace(p, q=p.q[b * p.t:(b + 1) * p.t].contiguous(), block_table=p.block_table[b:b + 1].clone(),
                               seq_lens=p.seq_lens[b:b + 1].clone(),
                               want=None if p.want is None else p.want[b * p.t:(b + 1) * p.t])


# ---- chained with the append ---------------------------------------------------------------------------------------------

def chain_append_problem(kind: str) -> kc.Problem:
    """The append of the chained test: 3 sequences of 70 new tokens at 8/2 heads and pages of 16 behind 0, 37 and 130
    tokens, random values, a real RoPE table, power-of-two cache scales.  The tokens before a base are whatever the
    caches held: the test fills them with the poison pattern of ``kv_append_cases``, which is a finite number in both
    cache types."""
    scales = {} if kind == "bf16" else {"k_inv": 4.0, "v_inv": 0.5}
    return kc.make_problem(kind, 3, 70, 8, 2, 16, [0, 37, 130], rope=kc.real_tables(256),
                           values=kc.random_values(11, 210, 12, 1.0), max_seq_len=200, **scales)


def chained_problem(a: kc.Problem, q_out: np.ndarray, k: np.ndarray, v: np.ndarray) -> Problem:
    """The prefill problem behind the append ``a``: ``q_out`` bits ``[B * T][Hq][D]`` and the caches the append left,
    bits or codes ``[num_pages][Hkv][page][D]`` (without guard pages)."""
    q = torch.from_numpy(q_out.view(np.int16).copy()).view(torch.bfloat16)
    if a.kind == "bf16":
        kt, vt = (torch.from_numpy(x.view(np.int16).copy()).view(torch.bfloat16) for x in (k, v))
    else:
        kt, vt = (torch.from_numpy(x.copy()).view(FP8) for x in (k, v))
    return Problem(a.kind, q, kt, vt, torch.from_numpy(a.table[:a.b].copy()), torch.from_numpy(a.seq_lens.copy()),
                   a.t, a.max_seq_len, 1.0 / math.sqrt(D), 1.0 / a.k_inv, 1.0 / a.v_inv)


# ---- validation ----------------------------------------------------------------------------------------------------------

# addresses 1 TiB apart: no legal shape makes Q and O overlap by accident.  Never launched with.
GOOD = dict(kind=0, Q=1 << 40, K=2 << 40, V=3 << 40, block_table=4 << 40, seq_lens=5 << 40, O=6 << 40, B=2, T=3, Hq=8,
            Hkv=2, D=128, page=16, num_pages=9, table_stride=4, max_seq_len=64, scale=0.0883883461356163, k_scale=1.0,
            v_scale=1.0)
INT32_MAX = 2 ** 31 - 1


def validate(a: dict) -> str | None:
    """The refusal of ``gsx_prefill_attn`` for these arguments (addresses as integers), without its prefix, or None: a
    transcription of the rules in ``gsx_kernels.h``, in the order the library applies them."""
    if a["kind"] not in (0, 1):
        return f"unknown kind {a['kind']}"
    if a["D"] != 128:
        return "need D == 128"
    if not 1 <= a["Hq"] <= 4096:
        return "need 1 <= Hq <= 4096"
    if a["Hkv"] < 1 or a["Hq"] % a["Hkv"] or a["Hq"] // a["Hkv"] > 16:
        return "need Hq % Hkv == 0 and Hq / Hkv <= 16"
    if a["page"] < 16 or a["page"] > 256 or a["page"] % 16:
        return "need page % 16 == 0 and 16 <= page <= 256"
    if a["B"] < 1 or a["T"] < 1:
        return "need B >= 1 and T >= 1"
    if a["B"] * a["T"] > INT32_MAX:
        return "B * T must stay below 2^31"
    if -(-a["T"] // Q_ROWS) * a["B"] * a["Hq"] > INT32_MAX:
        return "ceil(T / 256) * B * Hq must stay below 2^31"
    if a["num_pages"] < 1:
        return "need num_pages >= 1"
    if a["table_stride"] < 1:
        return "need table_stride >= 1"
    if a["max_seq_len"] < 1:
        return "need max_seq_len >= 1"
    if a["max_seq_len"] > a["table_stride"] * a["page"]:
        return "need max_seq_len <= table_stride * page"
    ptrs = [a[x] for x in ("Q", "K", "V", "O", "block_table", "seq_lens")]
    if not all(ptrs):
        return "Q, K_cache, V_cache, O, block_table and seq_lens must not be NULL"
    if any(a[x] % 16 for x in ("Q", "K", "V", "O")):
        return "Q, K_cache, V_cache and O must be 16-B aligned"
    if a["block_table"] % 4 or a["seq_lens"] % 4:
        return "block_table and seq_lens must be 4-B aligned"
    nbytes = a["B"] * a["T"] * a["Hq"] * D * 2
    if a["Q"] < a["O"] + nbytes and a["O"] < a["Q"] + nbytes:
        return "O must not overlap Q"
    f32 = [float(np.float32(a[x])) for x in ("scale", "k_scale", "v_scale")]
    if not all(math.isfinite(x) and x > 0 for x in f32):
        return "scale, k_scale and v_scale must be finite and > 0"
    if a["kind"] == 0 and (f32[1] != 1.0 or f32[2] != 1.0):
        return "a bf16 cache takes no scales: k_scale and v_scale must be 1.0"
    return None


def edges() -> list[tuple[dict, str | None]]:
    """``(arguments, refusal or None)``: each rule's last accepted and first refused value."""
    def g(**kw):
        return {**GOOD, **kw}

    row = 2 * 3 * 8 * D * 2  # bytes of GOOD's Q and O
    nan, inf = float("nan"), float("inf")
    return [
        (g(), None),
        (g(kind=1, k_scale=0.5, v_scale=2.0), None),
        (g(kind=2), "unknown kind 2"), (g(kind=-1), "unknown kind -1"),
        (g(D=64), "need D == 128"), (g(D=256), "need D == 128"),
        (g(Hq=0, Hkv=1), "need 1 <= Hq <= 4096"), (g(Hq=4096, Hkv=256), None),
        (g(Hq=4097, Hkv=4097), "need 1 <= Hq <= 4096"),
        (g(Hkv=0), "need Hq % Hkv == 0 and Hq / Hkv <= 16"), (g(Hkv=3), "need Hq % Hkv == 0 and Hq / Hkv <= 16"),
        (g(Hq=16, Hkv=1), None), (g(Hq=17, Hkv=1), "need Hq % Hkv == 0 and Hq / Hkv <= 16"),
        (g(page=0), "need page % 16 == 0 and 16 <= page <= 256"), (g(page=24), "need page % 16 == 0 and 16 <= page <= 256"),
        (g(page=256), None), (g(page=272, table_stride=1), "need page % 16 == 0 and 16 <= page <= 256"),
        (g(B=0), "need B >= 1 and T >= 1"), (g(T=0), "need B >= 1 and T >= 1"),
        (g(B=1, T=INT32_MAX, Hq=1, Hkv=1), None),
        (g(B=2, T=1 << 30, Hq=1, Hkv=1), "B * T must stay below 2^31"),
        (g(B=1 << 20, T=1, Hq=2048, Hkv=2048), "ceil(T / 256) * B * Hq must stay below 2^31"),
        (g(B=(1 << 20) - 1, T=1, Hq=2048, Hkv=2048), None),
        (g(num_pages=0), "need num_pages >= 1"), (g(num_pages=1), None),
        (g(table_stride=0), "need table_stride >= 1"),
        (g(max_seq_len=0), "need max_seq_len >= 1"), (g(max_seq_len=1), None),
        (g(max_seq_len=65), "need max_seq_len <= table_stride * page"),
        *[(g(**{x: 0}), "Q, K_cache, V_cache, O, block_table and seq_lens must not be NULL")
          for x in ("Q", "K", "V", "O", "block_table", "seq_lens")],
        *[(g(**{x: GOOD[x] + 8}), "Q, K_cache, V_cache and O must be 16-B aligned") for x in ("Q", "K", "V", "O")],
        *[(g(**{x: GOOD[x] + 2}), "block_table and seq_lens must be 4-B aligned") for x in ("block_table", "seq_lens")],
        (g(block_table=GOOD["block_table"] + 4, seq_lens=GOOD["seq_lens"] + 4), None),
        (g(O=GOOD["Q"]), "O must not overlap Q"), (g(O=GOOD["Q"] + row - 16), "O must not overlap Q"),
        (g(O=GOOD["Q"] + row), None), (g(Q=GOOD["O"] + row - 16), "O must not overlap Q"),
        *[(g(kind=1, **{x: bad}), "scale, k_scale and v_scale must be finite and > 0")
          for x in ("scale", "k_scale", "v_scale") for bad in (0.0, -1.0, nan, inf)],
        (g(k_scale=0.5), "a bf16 cache takes no scales: k_scale and v_scale must be 1.0"),
        (g(v_scale=2.0), "a bf16 cache takes no scales: k_scale and v_scale must be 1.0"),
    ]
