"""Problems for the add + RMSNorm and SwiGLU tests (native/kernels/norm_act.hip), an fp64 reference, the error bound
of the contract in ``gsx_kernels.h`` as functions, and an fp32 NumPy twin of the kernels' order.

Plain Python on NumPy (torch only where a test compares with it), no GPU.  The number formats (bf16 bits, the explicit
e4m3 encoder) are those of ``tests/kv_append_cases.py``.

The contract is a bound: the kernel's fp32 value ``y32`` lies within a relative error delta of the exact value, and
the output is the rounding of ``y32``.  So a result passes when EVERY element lies in
``[RN(exact (1 - delta)), RN(exact (1 + delta))]`` (:func:`bf16_interval`; the rounding from fp64 straight to bf16,
never through fp32).  No element is ever left out.  The reference (:func:`norm_reference`, :func:`silu_reference`) is
fp64 on the exact bf16 inputs; ``h = bf16(fl32(x + r))`` is computed exactly as specified (one IEEE fp32 addition, one
rounding to bf16), and ``R_out`` is compared byte for byte.

delta, with u = 2^-24 per correctly rounded fp32 operation (the derivation the header gives):

* norm: :func:`norm_delta` ``= (n_chain + n_tree + 6) u``.  A thread adds the squares of its chunks in turn, 8 per
  chunk and ``ceil(H / 2048)`` chunks (n_chain; every square of a bf16 value is exact, so an FMA changes nothing), a
  wave combines over 6 shuffle levels and the four waves over 2 (n_tree = 8): all terms are positive, so ``ss`` is off
  by at most ``(n_chain + n_tree) u``, which is 72 u at H = 16384 and 16 u up to H = 2048.  ``ss / H``, ``+ eps``
  (eps >= 0), ``sqrtf`` and ``1 / x`` are correctly rounded (the kernel's code holds the division and square-root
  sequences with their fix-ups, no v_rsq_f32); with ``h * rinv`` and ``* w`` that is 6 u.  The square root halves the
  error in front of it; the bound does not use that.
* silu: :func:`silu_delta` ``(g) = (4 + |g|) 2^-23``.  ``t = fl(g * fl(-log2 e))`` is off by 2 u |t|, which the
  exponential turns into ``2 u |t| ln 2 = |g| 2^-23`` relative; ``v_exp_f32`` 2^-23; ``1 + e`` u; ``v_rcp_f32`` 2^-23;
  two multiplies 2 u: ``(|g| + 3.5) 2^-23``.
* e4m3 output: the kernel writes ``scale = fl(amax / 448)`` and encodes ``fl(y32 * fl(448 / amax))``, which is within
  3 u of ``y32 / scale``: :data:`FP8_EXTRA`.  Checked with the kernel's own ``scale_out`` read back
  (:func:`check_fp8`): the scale lies between ``max |exact| (1 - delta) (1 - 3 u) / 448`` and ``max |exact| (1 + delta)
  (1 + 3 u) / 448``; every code lies between the e4m3 encodings (:func:`e4m3_encode64`, the encoder of
  ``kv_append_cases`` on fp64) of the ends ``exact (1 -+ (delta + 3 u)) / scale``; the row's largest element is 0x7e or
  0xfe; a row of zeros has scale 1.0 and codes 0x00.

A test shows little where an interval holds more than one value: :func:`ambiguous_fraction` is asserted to be at most
1 % for every random case (tests/test_norm_act_cases.py).  The SwiGLU cases take a random ``u``: with a constant ``u``
and tiny gates ``silu(g) u`` is linear in ``g`` and lands on exact rounding ties.

The twins (:func:`norm_twin`, :func:`silu_twin`) follow the kernels' order in fp32, the transcendental instructions
replaced by correctly rounded NumPy ones; their ``wrong=`` variants are the tests of the tests.
"""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

from tests import kv_append_cases as kc

U32 = 2.0 ** -24
FP8_EXTRA = 3 * U32
KINDS = ("bf16", "fp8")
THREADS = 256
GUARD_ROWS = 3  # poison rows on either side of every output
POISON8 = kc.POISON8
NORM_WRONG = ("unrounded h", "no eps", "no weight", "drop a chunk", "double a chunk", "amax of bf16")
SILU_WRONG = ("swap gate and up", "amax of bf16")


# ---- the bound -------------------------------------------------------------------------------------------------------

def chunks_per_thread(n: int) -> int:
    """Chunks of 8 elements the busiest of 256 threads owns in a row of ``n`` elements."""
    return math.ceil(n / 8 / THREADS)


def norm_delta(h: int) -> float:
    n_chain, n_tree = 8 * chunks_per_thread(h), 6 + 2
    assert n_chain + n_tree <= 96
    return (n_chain + n_tree + 6) * U32


def silu_delta(g):
    return (4.0 + np.abs(np.asarray(g, dtype=np.float64))) * 2.0 ** -23


# ---- number formats --------------------------------------------------------------------------------------------------

def bf16_round64(x) -> np.ndarray:
    """fp64 -> the nearest bf16 value (ties to even), as fp32, rounded once: 8 significant bits above 2^-126, steps of
    2^-133 below, inf from 2^128 (1 - 2^-9) on."""
    x = np.asarray(x, dtype=np.float64)
    _, e = np.frexp(x)  # |x| = m 2^e, m in [0.5, 1)
    step = np.exp2(np.maximum(e - 8, -133).astype(np.float64))
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.rint(x / step) * step  # the division is exact (a power of two); rint rounds to even
        # r has 8 significant bits: exact in fp32, or 2^128 and beyond, which becomes inf
        return np.where(np.isfinite(x), r, x).astype(np.float32)


def bf16_interval(exact, delta):
    """``(lo, hi)`` as fp32 values of bf16: the roundings of ``exact (1 - delta)`` and ``exact (1 + delta)``, sorted."""
    exact = np.asarray(exact, dtype=np.float64)
    a, b = bf16_round64(exact * (1.0 - delta)), bf16_round64(exact * (1.0 + delta))
    return np.minimum(a, b), np.maximum(a, b)


def e4m3_encode64(x) -> np.ndarray:
    """``kv_append_cases.e4m3_encode`` on fp64, rounded once: round to nearest even onto OCP e4m3fn, saturating."""
    x = np.asarray(x, dtype=np.float64)
    sign = np.where(np.signbit(x), 0x80, 0).astype(np.uint8)
    nan = np.isnan(x)
    a = np.minimum(np.abs(np.where(nan, 0, x)), 448.0)
    _, e = np.frexp(a)
    step = np.exp2(np.maximum(e - 1, -6) - 3.0)
    val = np.rint(a / step) * step
    m, e = np.frexp(val)
    normal = ((e - 1 + 7) * 8 + np.rint((2 * m - 1) * 8)).astype(np.int64)
    code = np.where(val < 2.0 ** -6, np.rint(val * 512.0).astype(np.int64), normal)
    assert code.max(initial=0) <= 0x7E
    return np.where(nan, 0x7F, code).astype(np.uint8) | sign


def e4m3_value(codes) -> np.ndarray:
    return kc.e4m3_values()[np.asarray(codes, dtype=np.uint8)]


# ---- problems --------------------------------------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class NormProblem:
    """``x`` bf16 bits ``[M][x_stride]``, ``r`` bits ``[M][r_stride]`` or None (R_in NULL), ``w`` bits ``[H]``.
    ``r_out``: "new" (a buffer of its own), "inplace" (R_out == R_in) or None (R_out NULL).  Arrays are shared: not to
    be written to."""
    x: np.ndarray
    r: np.ndarray | None
    w: np.ndarray
    h: int
    eps: float
    r_out: str | None = "new"
    r_stride: int = 0  # of a "new" R_out without R_in (0: H)
    y_pad: int = 0

    def __post_init__(self):
        assert self.r_out in ("new", "inplace", None) and (self.r_out != "inplace" or self.r is not None)

    @property
    def m(self) -> int:
        return self.x.shape[0]

    @property
    def x_stride(self) -> int:
        return self.x.shape[1]

    @property
    def rs(self) -> int:
        return self.r.shape[1] if self.r is not None else (self.r_stride or self.h)

    @property
    def y_stride(self) -> int:
        return self.h + self.y_pad


@dataclasses.dataclass(frozen=True)
class SiluProblem:
    """``gu`` bf16 bits ``[M][gu_stride]``: ``i`` gate values, then ``i`` up values."""
    gu: np.ndarray
    i: int
    y_pad: int = 0

    @property
    def m(self) -> int:
        return self.gu.shape[0]

    @property
    def gu_stride(self) -> int:
        return self.gu.shape[1]

    @property
    def y_stride(self) -> int:
        return self.i + self.y_pad


@dataclasses.dataclass
class Result:
    """What a launch leaves, without padding: ``y`` bf16 bits or e4m3 codes ``[M][n]``, ``scale`` fp32 ``[M]`` (fp8
    kind), ``r_out`` bf16 bits ``[M][H]`` (the norm, if it has one)."""
    y: np.ndarray
    scale: np.ndarray | None = None
    r_out: np.ndarray | None = None


def _padded(a: np.ndarray, pad: int) -> np.ndarray:
    """bf16 bits of fp32 ``a[M][n]`` with ``pad`` elements of poison behind every row."""
    bits = kc.bf16_bits(a)
    return np.concatenate([bits, np.full((a.shape[0], pad), kc.POISON16, np.uint16)], axis=1) if pad else bits


def make_norm(x, r, w, eps: float, *, r_out="new", pad: int = 0) -> NormProblem:
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    rb = None if r is None else _padded(np.asarray(r, np.float32), 2 * pad)
    return NormProblem(_padded(x, pad), rb, kc.bf16_bits(w), x.shape[1], float(np.float32(eps)), r_out,
                       r_stride=x.shape[1] + 2 * pad, y_pad=3 * pad)


def make_silu(g, u, *, pad: int = 0) -> SiluProblem:
    g, u = np.asarray(g, np.float32), np.asarray(u, np.float32)
    return SiluProblem(_padded(np.concatenate([g, u], axis=1), pad), g.shape[1], y_pad=2 * pad)


def norm_h_bits(p: NormProblem) -> np.ndarray:
    """``h = bf16(fl32(x + r))`` as bits ``[M][H]``, exactly as the contract specifies it; ``x``'s own bits without
    ``r``."""
    xb = p.x[:, :p.h]
    if p.r is None:
        return xb
    with np.errstate(invalid="ignore", over="ignore"):
        return kc.bf16_bits(kc.bf16_value(xb) + kc.bf16_value(p.r[:, :p.h]))


def norm_reference(p: NormProblem) -> np.ndarray:
    """The exact ``y`` in fp64 ``[M][H]``."""
    h = kc.bf16_value(norm_h_bits(p)).astype(np.float64)
    ss = np.array([math.fsum(row * row) for row in h])
    rinv = 1.0 / np.sqrt(ss / p.h + float(p.eps))
    return h * rinv[:, None] * kc.bf16_value(p.w).astype(np.float64)[None]


def silu_inputs(p: SiluProblem):
    return kc.bf16_value(p.gu[:, :p.i]), kc.bf16_value(p.gu[:, p.i:2 * p.i])


def silu_reference(p: SiluProblem):
    """``(exact y in fp64, delta per element)``, both ``[M][I]``."""
    g, u = (a.astype(np.float64) for a in silu_inputs(p))
    return g / (1.0 + np.exp(-g)) * u, silu_delta(g)


# ---- checks ----------------------------------------------------------------------------------------------------------

def _first(bad: np.ndarray) -> tuple:
    return tuple(int(i) for i in np.argwhere(bad)[0])


def check_bf16(got_bits: np.ndarray, exact: np.ndarray, delta, what: str) -> None:
    lo, hi = bf16_interval(exact, delta)
    got = kc.bf16_value(got_bits)
    with np.errstate(invalid="ignore"):
        bad = ~((got >= lo) & (got <= hi))  # a NaN is in no interval
    if bad.any():
        at = _first(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside their interval; first at {at}: "
                             f"got {got[at]!r} ({int(got_bits[at]):#06x}), interval [{lo[at]!r}, {hi[at]!r}], exact "
                             f"{exact[at]!r}")


def check_fp8(got_codes: np.ndarray, got_scale: np.ndarray, exact: np.ndarray, delta, what: str) -> None:
    delta = np.broadcast_to(np.asarray(delta, np.float64), exact.shape)
    mag = np.abs(exact)
    amax = mag.max(axis=1)
    lo_s = (mag * (1 - delta)).max(axis=1) * (1 - FP8_EXTRA) / 448.0
    hi_s = (mag * (1 + delta)).max(axis=1) * (1 + FP8_EXTRA) / 448.0
    scale = got_scale.astype(np.float64)
    zero = amax == 0
    bad_s = np.where(zero, scale != 1.0, ~((scale >= lo_s) & (scale <= hi_s)))
    if bad_s.any():
        m = int(np.argwhere(bad_s)[0][0])
        raise AssertionError(f"{what}: scale_out[{m}] = {got_scale[m]!r}, want "
                             + ("1.0 (a row of zeros)" if zero[m] else f"[{lo_s[m]!r}, {hi_s[m]!r}]"))
    if zero.any():
        assert not got_codes[zero].any(), f"{what}: a row of zeros has nonzero codes"
    safe = np.where(zero, 1.0, scale)[:, None]
    a = e4m3_value(e4m3_encode64(exact * (1 - (delta + FP8_EXTRA)) / safe))
    b = e4m3_value(e4m3_encode64(exact * (1 + (delta + FP8_EXTRA)) / safe))
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    got = e4m3_value(got_codes)
    with np.errstate(invalid="ignore"):
        bad = ~((got >= lo) & (got <= hi))
    if bad.any():
        at = _first(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} codes outside their interval; first at {at}: got "
                             f"{int(got_codes[at]):#04x} ({got[at]!r}), interval [{lo[at]!r}, {hi[at]!r}], exact "
                             f"{exact[at]!r}, scale {got_scale[at[0]]!r}")
    top = got_codes[np.arange(len(amax)), mag.argmax(axis=1)]
    want = np.where(exact[np.arange(len(amax)), mag.argmax(axis=1)] < 0, 0xFE, 0x7E)
    bad_t = ~zero & (top != want)
    assert not bad_t.any(), (f"{what}: the largest element of row {int(np.argwhere(bad_t)[0][0])} is "
                             f"{int(top[bad_t][0]):#04x}, want {int(want[bad_t][0]):#04x}")


def check(kind: str, got: Result, exact: np.ndarray, delta, what: str) -> None:
    if kind == "bf16":
        assert got.scale is None
        check_bf16(got.y, exact, delta, what)
    else:
        check_fp8(got.y, got.scale, exact, delta, what)


def check_norm(p: NormProblem, kind: str, got: Result, what: str) -> None:
    if p.r_out is not None:
        want = norm_h_bits(p)
        bad = got.r_out != want
        if bad.any():
            at = _first(bad)
            raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements of R_out differ; first at {at}: got "
                                 f"{int(got.r_out[at]):#06x}, want {int(want[at]):#06x}")
    check(kind, got, norm_reference(p), norm_delta(p.h), what)


def check_silu(p: SiluProblem, kind: str, got: Result, what: str) -> None:
    exact, delta = silu_reference(p)
    check(kind, got, exact, delta, what)


def ambiguous_fraction(kind: str, exact: np.ndarray, delta) -> float:
    """The share of elements whose interval holds more than one value (e4m3: with the exact row maximum as amax)."""
    delta = np.broadcast_to(np.asarray(delta, np.float64), exact.shape)
    if kind == "bf16":
        lo, hi = bf16_interval(exact, delta)
        return float((lo != hi).mean())
    scale = np.maximum(np.abs(exact).max(axis=1), 2.0 ** -100)[:, None] / 448.0
    a = e4m3_encode64(exact * (1 - (delta + FP8_EXTRA)) / scale)
    b = e4m3_encode64(exact * (1 + (delta + FP8_EXTRA)) / scale)
    return float((e4m3_value(a) != e4m3_value(b)).mean())


# ---- the twins: the kernels' order in fp32 ---------------------------------------------------------------------------

def _block_sum(per_thread: np.ndarray) -> np.ndarray:
    """``[M][256]`` fp32 -> ``[M]``: xor shuffles over 32 .. 1 inside each wave of 64, then (s0 + s1) + (s2 + s3)."""
    v = per_thread.reshape(-1, 4, 64).astype(np.float32)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o]
    s = v[:, :, 0]
    return (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])


def sum_of_squares(h: np.ndarray, wrong: str | None = None) -> np.ndarray:
    """``h[M][H]`` fp32 -> the kernel's sum of squares: thread t adds the 8 squares of chunk t, then of chunk t + 256,
    and so on; then :func:`_block_sum`.  ``wrong``: "drop a chunk" (the row's last chunk is left out) or "double a
    chunk" (it is added twice)."""
    m, n = h.shape
    u = chunks_per_thread(n)
    sq = np.zeros((m, u * THREADS * 8), np.float32)
    sq[:, :n] = h * h
    if wrong == "drop a chunk":
        sq[:, n - 8:n] = 0
    sq = sq.reshape(m, u, THREADS, 8)
    acc = np.zeros((m, THREADS), np.float32)
    for j in range(u):
        for e in range(8):
            acc = acc + sq[:, j, :, e]
    if wrong == "double a chunk":
        t = (n // 8 - 1) % THREADS
        for e in range(8):
            acc[:, t] = acc[:, t] + h[:, n - 8 + e] * h[:, n - 8 + e]
    assert acc.dtype == np.float32
    return _block_sum(acc)


def _store(kind: str, y32: np.ndarray, wrong: str | None) -> Result:
    if kind == "bf16":
        return Result(kc.bf16_bits(y32))
    amax = np.abs(kc.bf16_round(y32) if wrong == "amax of bf16" else y32).max(axis=1).astype(np.float32)
    zero = amax == 0
    safe = np.where(zero, np.float32(1), amax)
    scale = np.where(zero, np.float32(1), safe / np.float32(448)).astype(np.float32)
    inv = np.where(zero, np.float32(0), np.float32(448) / safe).astype(np.float32)
    codes = kc.e4m3_encode(y32 * inv[:, None])
    codes[zero] = 0
    return Result(codes, scale)


def norm_twin(p: NormProblem, kind: str, wrong: str | None = None) -> Result:
    assert wrong is None or wrong in NORM_WRONG
    hb = norm_h_bits(p)
    h = kc.bf16_value(hb)
    if wrong == "unrounded h" and p.r is not None:
        h = kc.bf16_value(p.x[:, :p.h]) + kc.bf16_value(p.r[:, :p.h])
    ss = sum_of_squares(h, wrong)
    mean = ss / np.float32(p.h)
    t = mean if wrong == "no eps" else mean + np.float32(p.eps)
    w = np.ones(p.h, np.float32) if wrong == "no weight" else kc.bf16_value(p.w)
    with np.errstate(divide="ignore", invalid="ignore"):  # a wrong twin may divide by zero
        rinv = np.float32(1) / np.sqrt(t)
        y32 = (h * rinv[:, None]) * w[None]
    assert y32.dtype == np.float32
    out = _store(kind, y32, wrong)
    out.r_out = hb if p.r_out is not None else None
    return out


def silu_twin(p: SiluProblem, kind: str, wrong: str | None = None) -> Result:
    assert wrong is None or wrong in SILU_WRONG
    g, u = silu_inputs(p)
    if wrong == "swap gate and up":
        g, u = u, g
    with np.errstate(over="ignore"):
        e = np.exp2(g * np.float32(-1.44269504088896341)).astype(np.float32)
        y32 = (g * (np.float32(1) / (np.float32(1) + e))) * u
    assert y32.dtype == np.float32
    return _store(kind, y32, wrong)


# ---- cases -----------------------------------------------------------------------------------------------------------

NORM_SHAPES = ((1, 8, 0), (3, 2040, 8), (17, 2048, 0), (3, 2056, 16), (3, 4104, 0), (1, 8192, 8), (3, 16384, 0),
               (17, 16384, 8))  # (M, H, pad): one chunk, 255 / 256 / 257 chunks, 2 -> 4 and 8 chunks a thread
SILU_SHAPES = ((1, 8, 0), (3, 2040, 8), (17, 2048, 0), (3, 2056, 16), (3, 4088, 0), (3, 4104, 8), (17, 16384, 0))
SILU_SHAPES_FP8 = (*SILU_SHAPES, (3, 32768, 0))
EPS = 1e-5


def _rows_scale(m: int) -> np.ndarray:
    """A size per row: 1, and where there are rows to spare a large one, and a small one at which eps matters."""
    s = np.ones((m, 1), np.float32)
    if m >= 3:
        s[1], s[2] = 2.0 ** 12, 2.0 ** -9
    return s


@functools.lru_cache(maxsize=None)
def norm_random_cases() -> tuple:
    """``(name, problem)``: Gaussian ``x`` and ``r``, weights around 1, over :data:`NORM_SHAPES` and the residual
    variants (R_in NULL, R_out NULL, in place)."""
    out = []
    for k, (m, h, pad) in enumerate(NORM_SHAPES):
        rng = np.random.default_rng(100 + k)
        s = _rows_scale(m)
        x = rng.standard_normal((m, h)).astype(np.float32) * s
        r = rng.standard_normal((m, h)).astype(np.float32) * s
        w = (1 + 0.25 * rng.standard_normal(h)).astype(np.float32)
        variant = (("new", True), ("inplace", True), (None, True), ("new", False))[k % 4]
        out.append((f"M{m} H{h} pad{pad} R_out {variant[0]} R_in {'yes' if variant[1] else 'NULL'}",
                    make_norm(x, r if variant[1] else None, w, EPS, r_out=variant[0], pad=pad)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def silu_random_cases(kind: str) -> tuple:
    """Gaussian gates (sigma 3) with every fourth row uniform over [-64, 64], random ``u``."""
    out = []
    for k, (m, i, pad) in enumerate(SILU_SHAPES_FP8 if kind == "fp8" else SILU_SHAPES):
        rng = np.random.default_rng(200 + k)
        g = (3 * rng.standard_normal((m, i))).astype(np.float32)
        g[::4] = rng.uniform(-64, 64, (len(g[::4]), i))
        g = np.clip(kc.bf16_round(g), -64, 64)
        u = rng.standard_normal((m, i)).astype(np.float32)
        out.append((f"M{m} I{i} pad{pad}", make_silu(g, u, pad=pad)))
    return tuple(out)


def boundary_columns(n: int) -> list[int]:
    """Columns at which a row of ``n`` elements can lose or double one: element 0 and 7 of the first and the last
    chunk, of every wave's first and last lane, in the first and last chunk a thread owns and on either side of every
    group of four chunks in flight together."""
    nchunks, u = n // 8, chunks_per_thread(n)
    js = sorted({j for j in (0, 3, 4, 7, 8, 11, 12, 15) if j < u} | {u - 1})
    chunks = {0, nchunks - 1} | {t + THREADS * j for t in (0, 63, 64, 127, 128, 191, 192, 255) for j in js}
    cols = []
    for k, c in enumerate(sorted(c for c in chunks if c < nchunks)):
        cols.append(8 * c + (0, 7)[k % 2])
    return cols


def norm_one_hot(h: int) -> NormProblem:
    """Row i holds one nonzero element, +-2^k, at :func:`boundary_columns` [i]; eps 0 and weights of 1 and 2: the
    result is +-sqrt(H) w there and zero elsewhere.  A dropped element gives inf or NaN, a doubled one is off by
    sqrt 2."""
    cols = boundary_columns(h)
    x = np.zeros((len(cols), h), np.float32)
    for i, c in enumerate(cols):
        x[i, c] = (-1) ** i * 2.0 ** (i % 7 - 3)
    w = np.where(np.arange(h) % 3 == 0, 2.0, 1.0).astype(np.float32)
    return make_norm(x, None, w, 0.0, r_out=None)


def silu_one_hot(i: int) -> SiluProblem:
    """Row r holds one nonzero gate at :func:`boundary_columns` [r] (silu(0) u = 0 elsewhere) and a random ``u``."""
    cols = boundary_columns(i)
    g = np.zeros((len(cols), i), np.float32)
    for r, c in enumerate(cols):
        g[r, c] = (-1) ** r * (1 + r % 5)
    u = kc.bf16_round(np.random.default_rng(7).uniform(0.5, 2.0, (len(cols), i)).astype(np.float32))
    return make_silu(g, u)


def norm_exact(kind: str, m: int = 5, h: int = 2048):
    """``(problem, y, scale)`` with an exact result: ``x + r = +-2^k`` over a row (k by row), eps 0 and weights 2^j:
    ``ss = H 4^k`` in any order (every partial sum is a small multiple of 4^k), ``y = +-2^j`` and the codes ``+-448 *
    2^(j - jmax)``, whatever delta."""
    col = np.arange(h)
    sign = np.where((col * 7 // 3 + col // 5) % 2 == 0, 1.0, -1.0)
    k = np.arange(m)[:, None] - 2
    hval = (sign[None] * 2.0 ** k).astype(np.float32)
    x, r = (hval * 0.75).astype(np.float32), (hval * 0.25).astype(np.float32)
    j = (col % 4) - 2
    w = (2.0 ** j).astype(np.float32)
    y = np.broadcast_to(sign * w, (m, h)).astype(np.float32)
    p = make_norm(x, r, w, 0.0, r_out="new")
    if kind == "bf16":
        return p, kc.bf16_bits(y), None
    scale = np.full(m, np.float32(2.0) / np.float32(448), np.float32)
    return p, kc.e4m3_encode(y * np.float32(224)), scale


def silu_exact(kind: str, m: int = 4, i: int = 1024):
    """Gates 0, 32 and 64: ``exp(-g)`` is 1 or below 2^-46, so ``y = g u`` to far less than delta, and with ``u =
    +-2^k`` that is a bf16 value and, over the row's largest, an e4m3 code."""
    col = np.arange(i)
    g = np.broadcast_to(np.choose(col % 3, [64.0, 0.0, 32.0]), (m, i)).astype(np.float32)
    u = (np.where(col % 2 == 0, 1.0, -1.0)[None] * 2.0 ** ((col[None] // 3 + np.arange(m)[:, None]) % 3 - 1)
         ).astype(np.float32)
    y = g * u
    p = make_silu(g, u)
    if kind == "bf16":
        return p, kc.bf16_bits(y), None
    amax = np.abs(y).max(axis=1).astype(np.float32)
    return p, kc.e4m3_encode(y * (np.float32(448) / amax)[:, None]), amax / np.float32(448)
