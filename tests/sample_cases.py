"""Problems, the exact twin and the fp64 reference of the token sampler (``gsx_sample``, native/kernels/sample.hip).

The twin follows the contract in ``native/kernels/gsx_kernels.h`` one fp32 operation at a time (NumPy ``float32``
arithmetic rounds every operation on its own) and keeps weights and masses as integers, so it says which token a row
gives, not an interval.  ``tests/test_sample_cases.py`` checks the twin itself on the CPU, ``tests/test_gpu_sample.py``
the kernel against it.  A ``flaw`` makes a twin that is wrong on purpose in one named way.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

F32 = np.float32
M64 = (1 << 64) - 1
KGOLDEN = 0x9E3779B97F4A7C15
LOG2E = F32(float.fromhex("0x1.715476p+0"))
COEF = tuple(F32(float.fromhex(h)) for h in ("0x1.62e4bcp-1", "0x1.ebdb30p-3", "0x1.c91e04p-5", "0x1.277576p-7",
                                              "0x1.e97886p-10"))  # c1 .. c5
FLAWS = ("ties_high", "k_plus_one", "p_before_k", "drop_crossing", "neg_zero_below", "fma")
NEG_INF, POS_INF, NAN, NEG_ZERO = 0xFF80, 0x7F80, 0x7FC0, 0x8000
POISON8 = 0xA5
INT_MAX = 2 ** 31 - 1


def mix64(z: int) -> int:
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw_word(seed: int, counter: int) -> int:
    a = mix64((seed + KGOLDEN) & M64)
    return mix64((a + ((counter + 1) & M64) * KGOLDEN) & M64)


def bf16_bits(x) -> np.ndarray:
    """fp32 to bf16 codes, round to nearest even; a NaN becomes the quiet NaN code."""
    x = np.ascontiguousarray(x, dtype=F32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(NAN), r).astype(np.uint16)


def bf16_value(bits) -> np.ndarray:
    return (np.asarray(bits).astype(np.uint32) << 16).view(F32)


def keys(bits, flaw: str | None = None) -> np.ndarray:
    """The 16-bit key that orders bf16 codes: -0 is +0, every NaN has key 0, below -inf."""
    b = np.asarray(bits).astype(np.int64)
    key = np.where(b & 0x8000, ~b & 0xFFFF, b | 0x8000)
    if flaw != "neg_zero_below":
        key = np.where(b == NEG_ZERO, 0x8000, key)
    return np.where((b & 0x7FFF) > 0x7F80, 0, key)


def poly(f: np.ndarray, fma: bool = False) -> np.ndarray:
    """g(f), near 2^f on [0, 1): fp32 Horner, every multiply and every add rounded on its own.  ``fma`` is the flaw:
    product and sum rounded once."""
    f = np.asarray(f, dtype=F32)
    g = np.full_like(f, COEF[4])
    for c in (COEF[3], COEF[2], COEF[1], COEF[0], F32(1)):
        if fma:
            g = (g.astype(np.float64) * f.astype(np.float64) + np.float64(c)).astype(F32)
        else:
            g = (g * f).astype(F32)
            g = (g + c).astype(F32)
    return g


def scale_c(temperature) -> np.float32:
    t = min(max(F32(temperature), F32(2.0 ** -16)), F32(2.0 ** 16))
    return F32(LOG2E / F32(t))


def weights(bits, first_bits: int, c: np.float32, fma: bool = False) -> np.ndarray:
    """The integer weights (uint64) of a row against the logit of ``first``."""
    with np.errstate(all="ignore"):
        lv = bf16_value(np.asarray(bits, dtype=np.uint16))
        lf = bf16_value(np.array([first_bits], dtype=np.uint16))[0]
        d = (lv - lf).astype(F32)
        x = (d * F32(c)).astype(F32)
        live = x >= F32(-32)  # false for a NaN
        xs = np.where(live, x, F32(0)).astype(F32)
        n = np.floor(xs).astype(F32)
        f = (xs - n).astype(F32)
        g = poly(f, fma)
        w = np.trunc(g.astype(np.float64) * np.exp2(32.0 + n.astype(np.float64)))  # exact: g has 24 bits
        return np.where(live, w, 0.0).astype(np.uint64)


def is_greedy(temperature) -> bool:
    return temperature is None or bool(np.isnan(F32(temperature))) or F32(temperature) <= 0


@dataclass
class Prepared:
    """A row and its parameters, up to the draw: ``greedy`` (a token), or N in index order with its prefix masses."""
    greedy: int | None = None
    n_idx: np.ndarray | None = None
    n_cum: np.ndarray | None = None
    zn: int = 0
    first: int = 0
    s_idx: np.ndarray | None = None

    def draw(self, seed: int, counter: int) -> int:
        if self.greedy is not None:
            return self.greedy
        target = (draw_word(int(seed), int(counter)) * self.zn) >> 64
        return int(self.n_idx[int(np.searchsorted(self.n_cum, np.uint64(target), side="right"))])


def prepare(bits, temperature, top_k, top_p, flaw: str | None = None) -> Prepared:
    bits = np.asarray(bits, dtype=np.uint16)
    v = bits.size
    key = keys(bits, flaw)
    top = np.flatnonzero(key == key.max())
    first = int(top[-1] if flaw == "ties_high" else top[0])
    finite = 0x007F < int(key[first]) < 0xFF80
    if is_greedy(temperature) or not finite:
        return Prepared(greedy=first, first=first)
    c = scale_c(temperature)
    w = weights(bits, int(bits[first]), c, fma=flaw == "fma")
    assert int(w[first]) == 1 << 32
    k = v if top_k is None or top_k <= 0 or top_k >= v else int(top_k)
    if flaw == "k_plus_one":
        k = min(k + 1, v)
    idx = np.arange(v)
    order = np.lexsort((-idx if flaw == "ties_high" else idx, -key))  # by descending key, then by index
    no_cut = top_p is None or bool(np.isnan(F32(top_p))) or F32(top_p) >= 1
    p = 0.0 if no_cut else float(max(F32(top_p), F32(0)))

    def nucleus(s: np.ndarray) -> np.ndarray:
        if no_cut:
            return s
        cum = np.cumsum(w[s], dtype=np.uint64)
        thr = p * float(int(cum[-1]))  # both exact in fp64, the product rounded once
        ends = np.flatnonzero(np.append(key[s][1:] != key[s][:-1], True))  # the last member of every group
        g = int(np.argmax(cum[ends].astype(np.float64) >= thr))
        if flaw == "drop_crossing" and g > 0:
            g -= 1
        return s[:ends[g] + 1]

    if flaw == "p_before_k":
        s = order[:k]
        n = nucleus(order)[:k]
    else:
        s = order[:k]
        n = nucleus(s)
    n = np.sort(n)
    cum = np.cumsum(w[n], dtype=np.uint64)
    return Prepared(n_idx=n, n_cum=cum, zn=int(cum[-1]), first=first, s_idx=np.sort(s))


def sample(bits, temperature, top_k, top_p, seed, counter, flaw: str | None = None) -> int:
    return prepare(bits, temperature, top_k, top_p, flaw).draw(0 if seed is None else seed, counter)


def reference_probs(values, temperature, top_k, top_p) -> np.ndarray:
    """softmax(l / T) in fp64, restricted by top-k (ties to the lowest indices) and then by top-p (groups of equal
    logits whole, up to the first at which the mass reaches p), renormalised."""
    lv = np.asarray(values, dtype=np.float64)
    v = lv.size
    order = np.lexsort((np.arange(v), -lv))
    k = v if top_k is None or top_k <= 0 or top_k >= v else int(top_k)
    s = order[:k]
    e = np.exp((lv[s] - lv[s[0]]) / float(temperature))
    if top_p is not None and top_p < 1:
        cum = np.cumsum(e)
        ends = np.flatnonzero(np.append(lv[s][1:] != lv[s][:-1], True))
        g = int(np.argmax(cum[ends] >= max(float(top_p), 0.0) * cum[-1]))
        s, e = s[:ends[g] + 1], e[:ends[g] + 1]
    out = np.zeros(v)
    out[s] = e / e.sum()
    return out


# ---- problems -----------------------------------------------------------------------------------------------------------

@dataclass
class Case:
    """One launch.  ``bits`` is [M][V], or [V] with a stride of 0.  A parameter array that is None is passed as NULL."""
    name: str
    bits: np.ndarray
    m: int
    temperature: np.ndarray | None
    top_k: np.ndarray | None
    top_p: np.ndarray | None
    seeds: np.ndarray | None
    counter: int = 0
    pad: int = 0  # elements behind every row (a stride above V)
    flaw_hint: str = ""
    _expected: np.ndarray | None = field(default=None, repr=False)

    @property
    def v(self) -> int:
        return int(self.bits.shape[-1])

    @property
    def shared(self) -> bool:
        return self.bits.ndim == 1

    def row_params(self, r: int):
        return (None if self.temperature is None else self.temperature[r],
                None if self.top_k is None else int(self.top_k[r]),
                None if self.top_p is None else self.top_p[r],
                0 if self.seeds is None else int(self.seeds[r]))

    def expected(self, flaw: str | None = None) -> np.ndarray:
        """The twin's tokens.  Rows that share logits and parameters share the work up to the draw."""
        if flaw is None and self._expected is not None:
            return self._expected
        memo: dict = {}
        out = np.zeros(self.m, dtype=np.int32)
        for r in range(self.m):
            t, k, p, seed = self.row_params(r)
            tag = (0 if self.shared else r, None if t is None else F32(t).tobytes(), k,
                   None if p is None else F32(p).tobytes())
            if tag not in memo:
                memo[tag] = prepare(self.bits if self.shared else self.bits[r], t, k, p, flaw)
            out[r] = memo[tag].draw(seed, self.counter)
        if flaw is None:
            self._expected = out
        return out


def _f32(x, m):
    """A scalar for every row, or a pattern repeated over the rows."""
    return None if x is None else np.resize(np.asarray(x, dtype=F32), m)


def _i32(x, m):
    return None if x is None else np.resize(np.asarray(x, dtype=np.int32), m)


def seeds_for(m: int, salt: int) -> np.ndarray:
    return np.array([mix64((salt << 32) + i + 1) for i in range(m)], dtype=np.uint64)


def make(name, bits, m=None, t=0.8, k=None, p=None, seeds="auto", counter=0, pad=0, salt=1) -> Case:
    bits = np.asarray(bits, dtype=np.uint16)
    m = bits.shape[0] if m is None else m
    if isinstance(seeds, str):
        seeds = None if t is None else seeds_for(m, salt)
    return Case(name, bits, m, _f32(t, m), _i32(k, m), _f32(p, m), seeds, counter, pad)


def random_bits(rng, shape, sigma=3.0) -> np.ndarray:
    return bf16_bits(rng.standard_normal(shape).astype(F32) * F32(sigma))


# The kernel's boundaries, in elements: a lane's 16-B chunk (8), a wave (512, also an index bin), the workgroup's
# stride (8192), the chunks a thread has in flight (32768).
BOUNDARIES = (8, 512, 8192, 32768)
GRID_V = (8, 248, 256, 264, 2056, 65544, 128256, 262144)
GRID_M = (1, 3, 17)


def grid_case(v: int, m: int) -> Case:
    """Random logits; every row has parameters of its own, row 0 the serving default."""
    rng = np.random.default_rng(1000 * m + v % 997)
    bits = random_bits(rng, (m, v))
    t = np.array([0.8, 1.0, 0.0, 0.3, 2.5, 100.0, 0.05][:m] + [0.7 + 0.1 * i for i in range(max(0, m - 7))], F32)[:m]
    k = np.array([50, 0, 5, 1, v - 1, 7, v + 3][:m] + [3 * i + 2 for i in range(max(0, m - 7))], np.int32)[:m]
    p = np.array([0.95, 1.0, 0.5, 0.9, 0.2, 0.999, 0.0][:m] + [0.05 * i for i in range(max(0, m - 7))], F32)[:m]
    return make(f"grid V={v} M={m}", bits, t=t, k=k, p=p, pad=8 * (m % 3), salt=v + m, counter=m)


def many_draws_case(v: int = 264, m: int = 4096) -> Case:
    rng = np.random.default_rng(7)
    return make(f"stride 0, {m} seeds, V={v}", random_bits(rng, v, 2.0), m=m, t=1.0, k=40, p=0.9, salt=99)


def all_codes_case() -> Case:
    """Every bf16 code once, shuffled: NaNs, infinities, both zeros.  The maximum is +inf, so every row is greedy."""
    rng = np.random.default_rng(3)
    return make("every bf16 code", rng.permutation(np.arange(65536, dtype=np.uint16)), m=4, t=[0.0, 1.0, 0.5, np.nan],
                k=[0, 3, 0, 0], p=[1.0, 0.5, 1.0, 1.0])


def finite_codes_case() -> Case:
    """Every finite bf16 code above -2^20 and below 2^4 once: the weights' whole range."""
    rng = np.random.default_rng(4)
    codes = np.arange(65536, dtype=np.uint16)
    val = bf16_value(codes)
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(val) & (val < 16) & (val > -2.0 ** 20)
    codes = rng.permutation(codes[keep])
    codes = codes[:codes.size // 8 * 8]
    return make("finite codes", codes, m=6, t=[1.0, 0.25, 4.0, 1.0, 1.0, 0.01], k=[0, 0, 0, 100, 3000, 0],
                p=[1.0, 0.99, 0.9, 1.0, 0.7, 1.0], salt=5)


def byte_cases() -> list[Case]:
    """Keys that differ only in the low byte (one high-byte bin) and only in the high byte."""
    rng = np.random.default_rng(5)
    low = (0x4000 + rng.integers(0, 256, 2056)).astype(np.uint16)  # 2.0 .. 3.99
    high = (rng.integers(0x38, 0x42, 2056) << 8).astype(np.uint16) | np.uint16(0x55)
    return [make("low byte only", low, m=16, t=0.5, k=[0, 1, 9, 100] * 4, p=[1, 0.3, 0.8, 0.99] * 4, salt=6),
            make("high byte only", high, m=16, t=1.5, k=[0, 1, 9, 100] * 4, p=[1, 0.3, 0.8, 0.99] * 4, salt=7)]


def equal_and_two_valued_cases() -> list[Case]:
    rng = np.random.default_rng(6)
    eq = np.full(8200, 0x3F80, np.uint16)
    two = np.where(rng.random(8200) < 0.3, 0x4000, 0x3F80).astype(np.uint16)
    two[:8] = 0x3F80
    return [make("all equal", eq, m=32, t=1.0, k=[0, 1, 2, 8199, 513, 8, 9, 4097] * 4,
                 p=[1.0, 1.0, 0.5, 0.0] * 8, salt=8),
            make("all equal, greedy", eq, m=2, t=None),
            make("two values", two, m=32, t=[1.0, 0.1] * 16, k=[0, 5, 3000, 2460] * 8, p=[1.0, 0.5, 0.9, 0.0] * 8,
                 salt=9)]


def straddle_positions(v: int) -> list[int]:
    pos = sorted({q for b in BOUNDARIES for q in (b - 1, b, 2 * b - 1, 2 * b) if q < v} | {0, v - 1})
    return pos


def maximum_straddle_cases() -> list[Case]:
    """The maximum at indices on either side of every boundary: each alone (is it seen at all), then all tied."""
    v = 65544
    rng = np.random.default_rng(8)
    base = random_bits(rng, v, 1.0)
    pos = straddle_positions(v)
    rows = np.tile(base, (len(pos), 1))
    for r, q in enumerate(pos):
        rows[r, q] = 0x4200  # 32
    tied = base.copy()
    tied[pos[3:]] = 0x4200
    return [make("maximum alone at a boundary, greedy", rows, t=None),
            make("maximum alone at a boundary, sampled", rows, t=0.01, k=2, p=0.5, salt=10),
            make("maxima tied across boundaries, greedy", tied, m=1, t=None),
            make("maxima tied across boundaries, sampled", tied, m=64, t=1.0, k=0, p=0.0, salt=11)]


def tie_cut_cases() -> list[Case]:
    """The k-th key's tie group, its members on either side of every boundary, cut by top-k after its first member, in
    the middle and at its last member; two larger keys stand above it."""
    v = 65544
    rng = np.random.default_rng(9)
    base = bf16_bits(-np.abs(rng.standard_normal(v)).astype(F32) - F32(1))
    pos = straddle_positions(v)
    base[pos] = 0x4000  # the group: 2.0
    base[5], base[40000] = 0x4040, 0x4020  # 3.0 and 2.5
    g = len(pos)
    out = []
    for label, k in (("first", 3), ("second", 4), ("middle", 2 + g // 2), ("odd", 2 + g // 2 + 1), ("last but one", 1 + g),
                     ("last", 2 + g), ("past", 3 + g)):
        out.append(make(f"tie group cut at its {label} member", base, m=96, t=2.0, k=k, p=[1.0, 0.999, 0.4], salt=12 + k))
    return out


def top_p_edge_cases() -> list[Case]:
    """Masses that are powers of two: with T = fl32(log2 e), c is 1 and a logit l below the maximum 0 weighs
    2^(32 + l).  Tokens at 0, -1, .., -32 weigh 2^33 - 1 together; with one more token at -32 Z is 2^33 and the first
    group, 2^32, is exactly p Z at p = 0.5; with none it is one unit less and the first group still reaches it; with
    two it is one unit more and the first group falls short.  Then p one ulp below and above a half at Z = 2^33."""
    v = 520
    rng = np.random.default_rng(13)
    rows = np.full((3, v), NEG_INF, np.uint16)
    where = rng.permutation(v)
    for r, extra in enumerate((0, 1, 2)):
        rows[r, where[:33]] = bf16_bits(-np.arange(33, dtype=F32))
        rows[r, where[33:33 + extra]] = 0xC200  # -32
    out = [make(f"top-p edge: Z = 2^33 {label}", rows[r], m=48, t=LOG2E, k=0, p=0.5, salt=30 + r)
           for r, label in enumerate(("- 1", "exactly", "+ 1"))]
    out.append(make("top-p edge: p an ulp below and above a half", rows[1], m=48, t=LOG2E, k=0,
                    p=[np.nextafter(F32(0.5), F32(0)), np.nextafter(F32(0.5), F32(1)), 0.5], salt=33))
    return out


def special_value_cases() -> list[Case]:
    rng = np.random.default_rng(10)
    v = 2056
    scattered = random_bits(rng, (4, v))
    where = rng.random((4, v))
    scattered[where < 0.2] = NEG_INF
    scattered[(where >= 0.2) & (where < 0.4)] = NAN
    scattered[(where >= 0.4) & (where < 0.45)] = 0xFFC1  # a negative NaN with a payload
    scattered[(where >= 0.45) & (where < 0.5)] = 0x7F81
    all_ninf = np.full((2, v), NEG_INF, np.uint16)
    all_nan = np.full((2, v), NAN, np.uint16)
    all_nan[1, 1000:] = 0xFFFF
    pinf = random_bits(rng, (3, v))
    pinf[0, [1500, 70]] = POS_INF
    pinf[1, 2055] = POS_INF
    pinf[2, 0] = POS_INF
    pinf[2, 9] = NAN
    zeros = np.full((2, v), 0xC000, np.uint16)  # -2
    zeros[0, 600], zeros[0, 700] = NEG_ZERO, 0x0000
    zeros[1, 600], zeros[1, 700] = 0x0000, NEG_ZERO
    nan_ninf = np.full((1, v), NAN, np.uint16)
    nan_ninf[0, 1234] = NEG_INF
    prm = dict(t=[1.0, 0.5, 1.0, 2.0], k=[0, 10, 100, 3], p=[1.0, 0.9, 0.5, 1.0])
    cut = {name: val[:2] for name, val in prm.items()}
    return [make("-inf and NaN scattered", scattered, salt=40, **prm),
            make("all -inf", all_ninf, salt=41, **cut), make("all NaN", all_nan, salt=42, **cut),
            make("with +inf", pinf, t=[1.0, 0.5, 1.0], k=[0, 10, 100], p=[1.0, 0.9, 0.5], salt=43),
            make("-0 and +0 tie", zeros, t=None),
            make("-0 and +0 tie, sampled", np.repeat(zeros, 16, axis=0), t=1.0, k=1, p=1.0, salt=45),
            make("NaN below -inf", nan_ninf, t=[1.0], salt=46)]


def parameter_cases() -> list[Case]:
    """Every value of T, k and p of the issue against each other, different in every row; then NULL arrays."""
    rng = np.random.default_rng(11)
    v = 264
    bits = random_bits(rng, v, 2.0)
    ts = [np.nan, -1.0, 0.0, 2.0 ** -20, 1.0, 2.0 ** 20]
    ks = [-1, 0, 1, v - 1, v, v + 1]
    ps = [np.nan, -1.0, 0.0, 0.5, 1.0, 2.0]
    grid = [(t, k, p) for t in ts for k in ks for p in ps]
    t, k, p = (np.array(c) for c in zip(*grid))
    out = [make("T x k x p", bits, m=len(grid), t=t, k=k, p=p, salt=50),
           make("INT_MIN and INT_MAX k, infinite T and p", bits, m=4, t=[np.inf, 1.0, -np.inf, 1.0],
                k=[-2 ** 31, INT_MAX, 3, -2 ** 31], p=[np.inf, -np.inf, 0.5, 1e-30], salt=51)]
    rows = random_bits(rng, (5, v), 2.0)
    out += [make("NULL temperature, seeds, k and p", rows, t=None),
            make("NULL temperature, the rest given", rows, t=None, k=3, p=0.5, seeds=seeds_for(5, 52)),
            make("NULL k", rows, t=1.0, p=0.7, salt=53), make("NULL p", rows, t=1.0, k=4, salt=54),
            make("NULL k and p", rows, t=[1.0, 0.0, 3.0, 0.2, 1.0], salt=55)]
    return out


def counter_cases() -> list[Case]:
    rng = np.random.default_rng(12)
    bits = random_bits(rng, 2056, 1.5)
    return [make(f"counter {c}", bits, m=24, t=1.0, k=0, p=1.0, counter=c, salt=60) for c in (0, 1, M64)]


def _find_fma_case() -> tuple[np.ndarray, np.float32, int]:
    """A row on which an FMA in g moves the top-p cut: the maximum at index 0 and V - 1 tokens of one smaller logit
    whose weight the FMA changes by a unit.  Z differs by V - 1 units between the twins, and p is an fp32 value at
    which the first group reaches p Z with the right weights and falls short with the others (or the other way
    round)."""
    v = 65544
    c = scale_c(1.0)
    codes = np.arange(0xC000, 0xC100, dtype=np.uint16)  # -2 .. -8
    w_ok, w_fma = weights(codes, 0, c), weights(codes, 0, c, fma=True)
    for i in np.flatnonzero(w_ok != w_fma):
        z_ok, z_fma = (1 << 32) + (v - 1) * int(w_ok[i]), (1 << 32) + (v - 1) * int(w_fma[i])
        lo, hi = min(z_ok, z_fma), max(z_ok, z_fma)
        p = F32((1 << 32) / ((lo + hi) / 2))
        if float(p) * float(lo) <= float(1 << 32) < float(p) * float(hi):
            bits = np.full(v, codes[i], np.uint16)
            bits[0] = 0
            return bits, p, i
    raise AssertionError("no logit found whose weight an FMA changes")


def fma_case() -> Case:
    bits, p, _ = _find_fma_case()
    return make("an FMA in g moves the top-p cut", bits, m=8, t=1.0, k=0, p=p, salt=70)


def flaw_cases() -> dict[str, list[Case]]:
    """For every flaw, the cases on which the flawed twin must give another token than the right one."""
    eq = equal_and_two_valued_cases()
    sp = special_value_cases()
    two = np.full(16, 0xC000, np.uint16)
    two[[3, 9]] = 0x3F80, 0x3F00  # 1.0 and 0.5 over -2
    k1 = make("k = 1 over two close logits", two, m=32, t=1.0, k=1, p=1.0, salt=80)
    spread = bf16_bits(np.linspace(0, -6, 64).astype(F32))
    order = make("k = 4, p = 0.5 over a slope", spread, m=64, t=1.0, k=4, p=0.5, salt=81)
    cross = make("p = 0.6 over a slope", spread, m=64, t=1.0, k=0, p=0.6, salt=82)
    return {"ties_high": [eq[1], maximum_straddle_cases()[2]], "k_plus_one": [k1], "p_before_k": [order],
            "drop_crossing": [cross, top_p_edge_cases()[2]], "neg_zero_below": [sp[4], sp[5]], "fma": [fma_case()]}


def sample_cases() -> list[Case]:
    """Everything but the size grid."""
    return [many_draws_case(), all_codes_case(), finite_codes_case(), *byte_cases(), *equal_and_two_valued_cases(),
            *maximum_straddle_cases(), *tie_cut_cases(), *top_p_edge_cases(), *special_value_cases(),
            *parameter_cases(), *counter_cases(), fma_case()]


# ---- gsx_embed_gather ---------------------------------------------------------------------------------------------------

def embed_reference(table: np.ndarray, tokens: np.ndarray, h: int) -> np.ndarray:
    """table is [V][stride] codes; a token outside [0, V) gives zeros."""
    v = table.shape[0]
    out = np.zeros((tokens.size, h), dtype=table.dtype)
    ok = (tokens >= 0) & (tokens < v)
    out[ok] = table[tokens[ok], :h]
    return out


# ---- refusals -----------------------------------------------------------------------------------------------------------

SAMPLE_REFUSALS = ("need M >= 1", "need 8 <= V <= 262144 and V % 8 == 0", "need logits_stride == 0, or logits_stride >= V",
                   "logits and tokens_out must not be NULL", "seeds may be NULL only when temperature is NULL",
                   "logits must be 16-B aligned", "temperature, top_k, top_p and tokens_out must be 4-B aligned",
                   "seeds must be 8-B aligned", "tokens_out must not overlap")
