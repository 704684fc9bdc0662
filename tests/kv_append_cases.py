"""Problems for the RoPE + KV-append tests (native/kernels/kv_append.hip), and a NumPy twin of the contract in
``gsx_kernels.h``.

Plain Python on NumPy (torch only where a test compares with it), no GPU.  What lives here:

* :func:`twin`, the contract one fp32 operation at a time: half-split rotation ``x1' = fl(fl(x1 c) - fl(x2 s))``,
  ``x2' = fl(fl(x2 c) + fl(x1 s))``, :func:`bf16_round` (round to nearest even on the bits) and :func:`e4m3_encode`, an
  explicit encoder onto OCP e4m3fn that saturates.  It returns every buffer the kernel may write (``Q_out``, both
  caches with their guard pages, ``lens_out``), pre-filled with the poison the GPU test fills them with, so a whole
  buffer is compared and a stray write fails.  Its ``wrong=`` variants (an FMA in the rotation, a token dropped, a
  token one slot late, a bad page index clamped) are the tests of the tests;
* :func:`reference64`, rotation and quantisation in fp64, and :func:`error_bound` (below);
* **addressing cases** (:func:`addressing_cases`): identity tables and small integers that name their (token, head
  row, d), exact in both cache types, over batch sizes, chunk lengths, head counts, page sizes, start lengths, table
  orders and strides; **dropped-page cases**; **rotation cases** with a real table; the **cancellation case**; the
  **code sweeps** of all 65,536 bf16 codes.

Every cache carries ``GUARD`` poison pages on either side of what ``num_pages`` describes and the block table one
spare row: a bad entry is -3..-1 or num_pages..num_pages + 2, so a kernel that clamps or follows it writes into a guard
page of the test's own allocation and fails a comparison instead of faulting.

The bound of the fp64 comparison.  With eps = 2^-24 each of the two products is off by eps of itself and the
difference by eps of itself, so ``|x1' - (x1 c - x2 s)| <= eps (|x1 c| + |x2 s|) + eps |x1'| <= 3 eps (|x1| + |x2|)``
for ``|c|, |s| <= 1`` (first order; the factor 3 has room for the second).  The multiplication by an inverse scale adds
one more eps.  Then one rounding to the output format: u = 2^-8 relative for bf16; for e4m3 2^-4 relative to the
value, or half the subnormal step 2^-10 absolute, and nothing beyond +-448, where the result saturates.  So

    bf16:  |got - ref| <= u |ref| + 3 eps (|x1| + |x2|) (1 + u)
    e4m3:  |got - sat(ref inv)| <= max(2^-4 |ref inv|, 2^-10) + 4 eps (|x1| + |x2|) inv (1 + 2^-4)
"""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

D = 128
HALF = 64
KINDS = ("bf16", "fp8")
GUARD = 3  # poison pages on either side of the caches
POISON8 = 0xA5  # what every writable buffer is filled with before a launch, byte by byte
POISON16 = 0xA5A5
POISON32 = np.int32(-0x5A5A5A5B)  # 0xA5A5A5A5
EPS = 2.0 ** -24
U = 2.0 ** -8


# ---- number formats --------------------------------------------------------------------------------------------------

def bf16_bits(x: np.ndarray) -> np.ndarray:
    """fp32 -> the 16 bits of its bf16, round to nearest even; a NaN keeps its top bits and stays a NaN."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    nan = (u & 0x7F800000) == 0x7F800000
    special = ((u >> 16) | np.where(u & 0xFFFF, 0x40, 0)).astype(np.uint32)
    rounded = (u.astype(np.uint64) + 0x7FFF + ((u >> 16) & 1)) >> 16
    return np.where(nan, special, rounded.astype(np.uint32)).astype(np.uint16)


def bf16_value(bits: np.ndarray) -> np.ndarray:
    """The fp32 value of bf16 bits: exact."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x: np.ndarray) -> np.ndarray:
    return bf16_value(bf16_bits(x))


def to_bits(x) -> np.ndarray:
    """Values that are exact in bf16, as bits."""
    x = np.asarray(x, dtype=np.float32)
    b = bf16_bits(x)
    assert np.array_equal(bf16_value(b), x, equal_nan=True)
    return b


def e4m3_encode(x: np.ndarray) -> np.ndarray:
    """fp32 -> the OCP e4m3fn code, round to nearest even, SATURATING: every finite value beyond +-448 and +-inf give
    +-448 (0x7e / 0xfe); a NaN gives 0x7f with its sign.  Spelt out from the format: 4 bits of exponent with bias 7,
    3 of mantissa, exponent 0 subnormal with step 2^-9."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    sign = ((x.view(np.uint32) >> 24) & 0x80).astype(np.uint8)
    nan = np.isnan(x)
    a = np.minimum(np.abs(np.where(nan, 0, x)).astype(np.float64), 448.0)
    _, e = np.frexp(a)  # a = m 2^e with m in [0.5, 1): the binade of a is e - 1
    step = np.exp2(np.maximum(e - 1, -6) - 3.0)
    val = np.rint(a / step) * step  # the division is exact (a power of two) and rint rounds to even
    m, e = np.frexp(val)
    normal = ((e - 1 + 7) * 8 + np.rint((2 * m - 1) * 8)).astype(np.int64)
    code = np.where(val < 2.0 ** -6, np.rint(val * 512.0).astype(np.int64), normal)
    assert code.max(initial=0) <= 0x7E
    return np.where(nan, 0x7F, code).astype(np.uint8) | sign


@functools.lru_cache(maxsize=None)
def e4m3_values() -> np.ndarray:
    """The value of each of the 256 codes in fp64, from the format (NaN at 0x7f and 0xff)."""
    c = np.arange(256)
    e, m = (c >> 3) & 15, c & 7
    v = np.where(e == 0, m / 8 * 2.0 ** -6, (1 + m / 8) * np.exp2(e - 7.0)) * np.where(c & 128, -1.0, 1.0)
    v[[0x7F, 0xFF]] = np.nan
    return v


def e4m3_midpoints() -> np.ndarray:
    """The 126 midpoints between neighbouring non-negative codes 0x00..0x7e, each with its fp32 neighbour below and
    above, and all of them negated: fp32, ``[2][126][3]``."""
    v = e4m3_values()[:0x7F]
    mid = ((v[:-1] + v[1:]) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (v[:-1] + v[1:]) / 2)
    trio = np.stack([np.nextafter(mid, np.float32(0)), mid, np.nextafter(mid, np.float32(1000))], axis=1)
    return np.stack([trio, -trio])


def same_e4m3(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Equal codes; the two NaN codes 0x7f and 0xff count as one."""
    a, b = np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint8)
    return (a == b) | (((a & 0x7F) == 0x7F) & ((b & 0x7F) == 0x7F))


# ---- problems --------------------------------------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class Problem:
    """One launch.  ``qkv`` holds bf16 bits ``[B * T][qkv_stride]``; ``table`` is int32 ``[B + 1][table_stride]`` (one
    spare row) and ``seq_lens`` int32 ``[B]``; ``cos`` and ``sin`` fp32 ``[rope_len][64]``.  The caches of the launch
    are ``[GUARD + num_pages + GUARD][Hkv][page][128]`` and the kernel is handed the address of page ``GUARD``.
    Arrays are shared: not to be written to."""
    kind: str
    qkv: np.ndarray
    b: int
    t: int
    hq: int
    hkv: int
    page: int
    num_pages: int
    table: np.ndarray
    seq_lens: np.ndarray
    max_seq_len: int
    cos: np.ndarray
    sin: np.ndarray
    k_inv: float = 1.0
    v_inv: float = 1.0

    @property
    def qkv_stride(self) -> int:
        return self.qkv.shape[1]

    @property
    def table_stride(self) -> int:
        return self.table.shape[1]

    @property
    def rope_len(self) -> int:
        return self.cos.shape[0]

    @property
    def rows(self) -> int:
        return self.hq + 2 * self.hkv

    def base(self) -> list[int]:
        """The lengths the kernel starts from: ``seq_lens`` clamped to ``[0, max_seq_len]``."""
        return [min(max(int(x), 0), self.max_seq_len) for x in self.seq_lens]

    def live(self) -> list[tuple[int, int, int]]:
        """``(token n, physical page, slot)`` of every live token, in order."""
        out = []
        for n in range(self.b * self.t):
            b, t = divmod(n, self.t)
            pos = self.base()[b] + t
            if pos < self.max_seq_len and 0 <= int(self.table[b, pos // self.page]) < self.num_pages:
                out.append((n, int(self.table[b, pos // self.page]), pos % self.page))
        return out


@dataclasses.dataclass
class Result:
    """What a launch leaves: bf16 bits of ``q_out[B * T][Hq][128]``, the caches with their guard pages (uint16 bits or
    uint8 codes), ``lens_out`` int32 ``[B]``."""
    q_out: np.ndarray
    k: np.ndarray
    v: np.ndarray
    lens_out: np.ndarray


def rotate(x1, x2, c, s, wrong=None):
    """The contract's rotation in fp32, one rounding per operation.  ``wrong``: "fuse x1c" and "fuse x2s" contract that
    product of the subtraction into an FMA (the product exact in fp64, one rounding of the difference)."""
    x1, x2, c, s = (np.asarray(a, dtype=np.float32) for a in (x1, x2, c, s))
    with np.errstate(invalid="ignore", over="ignore"):
        if wrong == "fuse x1c":
            y1 = (x1.astype(np.float64) * c - (x2 * s).astype(np.float64)).astype(np.float32)
        elif wrong == "fuse x2s":
            y1 = ((x1 * c).astype(np.float64) - x2.astype(np.float64) * s).astype(np.float32)
        else:
            y1 = x1 * c - x2 * s
        y2 = x2 * c + x1 * s
    assert y1.dtype == y2.dtype == np.float32
    return y1, y2


def empty_result(p: Problem) -> Result:
    pages = GUARD + p.num_pages + GUARD
    cdt, fill = (np.uint16, POISON16) if p.kind == "bf16" else (np.uint8, POISON8)
    return Result(np.full((p.b * p.t, p.hq, D), POISON16, dtype=np.uint16),
                  np.full((pages, p.hkv, p.page, D), fill, dtype=cdt),
                  np.full((pages, p.hkv, p.page, D), fill, dtype=cdt),
                  np.full((p.b,), POISON32, dtype=np.int32))


def twin(p: Problem, wrong: str | None = None) -> Result:
    """The contract in NumPy.  ``wrong``: None, a rotation of :func:`rotate`, "drop a token" (the last live token
    writes nothing to the caches), "a slot late" (every token lands one slot on, wrapping inside its page) or "clamp"
    (a bad page index is clamped into [0, num_pages) instead of dropped)."""
    out = empty_result(p)
    base = p.base()
    out.lens_out[:] = [min(x + p.t, p.max_seq_len) for x in base]
    out.q_out[:] = 0
    n_live = len(p.live())
    seen = 0
    for n in range(p.b * p.t):
        b, t = divmod(n, p.t)
        pos = base[b] + t
        if pos >= p.max_seq_len:
            continue
        pp = int(p.table[b, pos // p.page])
        if not 0 <= pp < p.num_pages:
            if wrong != "clamp":
                continue
            pp = min(max(pp, 0), p.num_pages - 1)
        else:
            seen += 1
        x = bf16_value(p.qkv[n, :p.rows * D]).reshape(p.rows, D)
        rot = x[:p.hq + p.hkv]
        y1, y2 = rotate(rot[:, :HALF], rot[:, HALF:], p.cos[pos], p.sin[pos], wrong)
        y = np.concatenate([y1, y2], axis=1)
        out.q_out[n] = bf16_bits(y[:p.hq])
        if wrong == "drop a token" and seen == n_live and 0 <= int(p.table[b, pos // p.page]) < p.num_pages:
            continue
        slot = pos % p.page
        if wrong == "a slot late":
            slot = (slot + 1) % p.page
        kx, vx = y[p.hq:], x[p.hq + p.hkv:]
        if p.kind == "bf16":
            out.k[GUARD + pp, :, slot] = bf16_bits(kx)
            out.v[GUARD + pp, :, slot] = p.qkv[n, (p.hq + p.hkv) * D:p.rows * D].reshape(p.hkv, D)
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                out.k[GUARD + pp, :, slot] = e4m3_encode(kx * np.float32(p.k_inv))
                out.v[GUARD + pp, :, slot] = e4m3_encode(vx * np.float32(p.v_inv))
    return out


def reference64(p: Problem):
    """Rotation in fp64 of every row of ``qkv`` at its token's position (dead tokens at position 0):
    ``(rotated[B * T][Hq + Hkv][128], v[B * T][Hkv][128], magnitude[B * T][Hq + Hkv][128])`` with magnitude
    ``|x1| + |x2|`` of an element's pair."""
    base = p.base()
    x = bf16_value(p.qkv[:, :p.rows * D]).astype(np.float64).reshape(-1, p.rows, D)
    pos = np.array([min(base[n // p.t] + n % p.t, p.rope_len - 1) for n in range(p.b * p.t)])
    c, s = p.cos[pos].astype(np.float64)[:, None], p.sin[pos].astype(np.float64)[:, None]
    x1, x2 = x[:, :p.hq + p.hkv, :HALF], x[:, :p.hq + p.hkv, HALF:]
    mag = np.abs(x1) + np.abs(x2)
    return (np.concatenate([x1 * c - x2 * s, x2 * c + x1 * s], axis=2), x[:, p.hq + p.hkv:],
            np.concatenate([mag, mag], axis=2))


def error_bound(ref: np.ndarray, mag: np.ndarray, kind: str, inv: float = 1.0, ops: int = 3):
    """``(target, bound)`` of the module docstring for values ``ref`` with pair magnitudes ``mag``: the bf16 value, or
    the saturated scaled value of an e4m3 code.  ``ops``: fp32 roundings in front of the scaling (3 for a rotation, 0
    for V)."""
    if kind == "bf16":
        return ref, U * np.abs(ref) + ops * EPS * mag * (1 + U)
    scaled = np.clip(ref * inv, -448.0, 448.0)
    return scaled, np.maximum(2.0 ** -4 * np.abs(scaled), 2.0 ** -10) + (ops + 1) * EPS * mag * inv * (1 + 2.0 ** -4)


# ---- tables ----------------------------------------------------------------------------------------------------------

def identity_tables(rope_len: int):
    return np.ones((rope_len, HALF), dtype=np.float32), np.zeros((rope_len, HALF), dtype=np.float32)


@functools.lru_cache(maxsize=4)
def real_tables(rope_len: int, theta: float = 10000.0):
    """cos and sin of ``pos * theta^(-i / 64)``, computed in fp64 and rounded to fp32."""
    ang = np.arange(rope_len, dtype=np.float64)[:, None] * theta ** (-np.arange(HALF, dtype=np.float64) / HALF)[None]
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def _page_order(total: int, mode: str) -> np.ndarray:
    i = np.arange(total)
    if mode == "identity":
        return i
    if mode == "reversed":
        return total - 1 - i
    assert mode == "scattered", mode
    step = next(s for s in range(max(2, (total * 5) // 8), 2 * total + 7) if math.gcd(s, total) == 1)
    return (i * step + 1) % total


def names(tokens: int, rows: int) -> np.ndarray:
    """Small integers 1..15 (exact in bf16 and e4m3) that name (token, head row, d): fp32 ``[tokens][rows][128]``.
    Neighbouring tokens, rows and elements all differ."""
    n, r, d = np.meshgrid(np.arange(tokens), np.arange(rows), np.arange(D), indexing="ij")
    return (1 + (7 * n + 5 * r + 3 * d + n // 15 + (r * d) // 7 + d // 16) % 15).astype(np.float32)


def make_problem(kind: str, b: int, t: int, hq: int, hkv: int, page: int, starts, *, max_seq_len: int | None = None,
                 tables: str = "scattered", extra_stride: int = 0, pad: int = 0, values: np.ndarray | None = None,
                 rope=None, bad: dict | None = None, k_inv: float = 1.0, v_inv: float = 1.0,
                 spare_pages: int = 2, reserve: int = 0) -> Problem:
    """``b`` sequences of ``t`` new tokens behind ``starts[b]`` tokens.  Every sequence owns the pages its positions up
    to ``max_seq_len`` (default: the longest end) need, or those of its first ``reserve`` positions if that is more;
    ``tables``: how physical pages are handed out;
    ``extra_stride``: columns of the block table nobody needs (they hold a page nobody owns); ``pad``: elements of
    poison behind every row of ``qkv``; ``values``: fp32 ``[b * t][rows][128]``, exact in bf16 (default
    :func:`names`); ``rope``: ``(cos, sin)`` (default the identity); ``bad``: ``{(sequence, table column): entry}``
    written over the table."""
    starts = list(starts)
    assert len(starts) == b
    rows = hq + 2 * hkv
    clamped = [min(max(s, 0), 1 << 30) for s in starts]
    max_seq_len = max(max(c + t for c in clamped), 1) if max_seq_len is None else max_seq_len
    need = [-(-max(min(min(c, max_seq_len) + t, max_seq_len), min(reserve, max_seq_len)) // page) for c in clamped]
    num_pages = sum(need) + spare_pages
    order = _page_order(num_pages, tables)
    stride = -(-max_seq_len // page) + extra_stride
    table = np.empty((b + 1, stride), dtype=np.int32)
    table[:] = order[sum(need):][np.arange(stride) % spare_pages][None] if spare_pages else 0
    at = 0
    for i in range(b):
        table[i, :need[i]] = order[at:at + need[i]]
        at += need[i]
    for (i, col), entry in (bad or {}).items():
        table[i, col] = entry
    values = names(b * t, rows) if values is None else values
    qkv = np.full((b * t, rows * D + pad), POISON16, dtype=np.uint16)
    qkv[:, :rows * D] = to_bits(values).reshape(b * t, rows * D)
    cos, sin = identity_tables(max_seq_len) if rope is None else rope
    assert cos.shape[0] >= max_seq_len and (rows * D + pad) % 8 == 0
    return Problem(kind, qkv, b, t, hq, hkv, page, num_pages, table, np.array(starts, dtype=np.int64).astype(np.int32),
                   max_seq_len, cos, sin, k_inv, v_inv)


HEADS = ((1, 1), (16, 1), (21, 3), (8, 2), (64, 8))


def addressing_cases(kind: str) -> list[tuple[str, Problem]]:
    """Identity tables and :func:`names`.  B in 1..5; T in 1, 2, 3, 17 and 2 page + 1; every pair of ``HEADS``; pages
    of 16, 64 and 256; up to 1030 tokens; start lengths of 0, mid-page, page - 1 and exactly max_seq_len - T; lengths
    that run past max_seq_len; lengths of -1 and -2^31; reversed, scattered and wider-stride tables; a qkv_stride with
    poison in the padding.  Every case has tokens on both sides of a page boundary."""
    mk = functools.partial(make_problem, kind)
    return [
        ("B 1, T 17, 1/1 heads, page 16, from 0", mk(1, 17, 1, 1, 16, [0], tables="identity")),
        ("B 2, T 1, 16/1 heads, page 16, page - 1 and the slot behind", mk(2, 1, 16, 1, 16, [15, 16])),
        ("B 3, T 2, 21/3 heads, page 64, mid-page and page - 1", mk(3, 2, 21, 3, 64, [30, 63, 127], tables="reversed")),
        ("B 4, T 3, 8/2 heads, page 16, exactly max_seq_len - T", mk(4, 3, 8, 2, 16, [0, 14, 45, 29], max_seq_len=48)),
        ("B 5, T 33, 64/8 heads, page 16, wider stride, padded rows",
         mk(5, 33, 64, 8, 16, [0, 7, 15, 16, 40], extra_stride=5, pad=24)),
        ("B 2, T 513, 8/2 heads, page 256, 1026 tokens", mk(2, 513, 8, 2, 256, [255, 100], tables="reversed", pad=8)),
        ("B 5, T 206, 1/1 heads, page 64, 1030 tokens", mk(5, 206, 1, 1, 64, [0, 63, 64, 1, 130])),
        ("B 3, T 129, 16/1 heads, page 64, T = 2 page + 1", mk(3, 129, 16, 1, 64, [0, 63, 17])),
        ("B 4, T 17, 21/3 heads, page 16, past max_seq_len",
         mk(4, 17, 21, 3, 16, [40, 64, 50, 1000], max_seq_len=64, extra_stride=1)),
        ("B 4, T 3, 8/2 heads, page 16, lengths of -1 and -2^31",
         mk(4, 3, 8, 2, 16, [-1, 15, -2 ** 31, 14], max_seq_len=40)),
    ]


def dropped_page_cases(kind: str) -> list[tuple[str, Problem]]:
    """Block-table entries of -3..-1 and num_pages..num_pages + 2 under tokens that would otherwise be live, next to
    live tokens of the same and of other sequences."""
    out = []
    for hq, hkv, page, t, starts in ((8, 2, 16, 35, [0, 10, 16]), (16, 1, 64, 70, [62, 0, 190])):
        p = make_problem(kind, 3, t, hq, hkv, page, starts)
        cols = sorted({(b, (s + i) // page) for b, s in enumerate(starts) for i in range(t)})
        entries = [-3, -2, -1, p.num_pages, p.num_pages + 1, p.num_pages + 2]
        step = 2 if len(cols) % 2 else 3
        bad = {cols[(step * i + 1) % len(cols)]: e for i, e in enumerate(entries)}
        assert len(bad) == 6
        p = make_problem(kind, 3, t, hq, hkv, page, starts, bad=bad)
        assert 0 < len(p.live()) < 3 * t
        out.append((f"{hq}/{hkv} heads, page {page}, T {t}: entries {sorted(set(bad.values()))}", p))
    return out


def random_values(seed: int, tokens: int, rows: int, scale: float = 1.0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return bf16_round((rng.standard_normal((tokens, rows, D)) * scale).astype(np.float32))


def rotation_cases(kind: str) -> list[tuple[str, Problem]]:
    """Random bf16 rows against a real table with positions up to 4095, and zeros of both signs."""
    scales = {} if kind == "bf16" else {"k_inv": 1 / 1.5, "v_inv": 0.75}
    rope = real_tables(4096)
    far = make_problem(kind, 3, 5, 8, 2, 16, [4091, 2047, 0], max_seq_len=4096, rope=rope,
                       values=random_values(1, 15, 12, 2.0), **scales)
    big = make_problem(kind, 2, 40, 21, 3, 64, [1000, 3000], max_seq_len=4096, rope=rope,
                       values=random_values(2, 80, 27, 30.0), **scales)
    z = np.zeros((6, 6, D), dtype=np.float32)
    z[:, :, ::2] = -0.0
    z[:, ::2, :HALF] *= -1
    z[1::2, :, 5::7] = 1.0
    zeros = make_problem(kind, 2, 3, 2, 2, 16, [14, 100], max_seq_len=4096, rope=rope, values=z, **scales)
    return [("positions up to 4095", far), ("larger values, page 64", big), ("zeros of both signs", zeros)]


def cancellation_problem(kind: str = "bf16") -> Problem:
    """``x1 = x2`` and ``s = c (1 + k 2^-20)``: ``x1 c - x2 s`` cancels to about 2^-20 of the products, so whether a
    product was rounded before the subtraction shows in the leading bits of the result.  32 tokens of one head row."""
    rng = np.random.default_rng(7)
    t = 32
    half = bf16_round(rng.uniform(1.0, 2.0, (t, 1, HALF)).astype(np.float32))
    values = np.concatenate([half, half], axis=2).repeat(3, axis=1)  # Q, K and V rows
    c = rng.uniform(0.5, 1.0, (t, HALF)).astype(np.float32)
    k = rng.integers(1, 16, (t, HALF)).astype(np.float32)
    s = (c * (1 + k * np.float32(2.0 ** -20))).astype(np.float32)
    scales = {} if kind == "bf16" else {"k_inv": 2.0 ** 20, "v_inv": 1.0}
    return make_problem(kind, 1, t, 1, 1, 16, [0], rope=(c, s), values=values, tables="identity", **scales)


def all_codes() -> np.ndarray:
    """All 65,536 bf16 codes as bits ``[512][128]``, in an order that puts neighbours into different rows."""
    return ((np.arange(65536, dtype=np.uint32) * 40503) & 0xFFFF).astype(np.uint16).reshape(512, D)


def sweep_problem(kind: str, through: str, inv: float) -> Problem:
    """512 tokens of one sequence at 1/1 heads, identity table.  ``through`` "v": the V row of token n is row n of
    :func:`all_codes`, Q and K rows hold :func:`names`.  ``through`` "k0" and "k1" (one half of the codes each): the K
    row of token n < 256 holds 64 codes in its first half and zeros in its second, and of token n >= 256 the other
    way round, so that every code meets the rotation as x1 or as x2 with a zero for a partner (x' = x for every finite
    x; the partner slot holds +-0, or a NaN where x is inf or NaN); Q and V rows are zeros."""
    codes = all_codes()
    qkv = np.zeros((512, 3, D), dtype=np.uint16)
    if through == "v":
        qkv[:, :2] = to_bits(names(512, 2))
        qkv[:, 2] = codes
    else:
        flat = codes.reshape(1024, HALF)[512 * int(through[1]):][:512]
        qkv[:256, 1, :HALF] = flat[:256]
        qkv[256:, 1, HALF:] = flat[256:]
    p = make_problem(kind, 1, 512, 1, 1, 16, [0], tables="scattered", values=np.zeros((512, 3, D), dtype=np.float32),
                     k_inv=inv if through != "v" else 1.0, v_inv=inv if through == "v" else 1.0)
    return dataclasses.replace(p, qkv=qkv.reshape(512, 3 * D))


def chain_problem(kind: str, steps: int = 33):
    """Decode steps for the chained test: ``(problems, start)``, one T = 1 problem per step over the same block table,
    3 sequences at 8/2 heads and pages of 16 whose lengths cross the 32-token tile, with a real table; the third
    reaches ``max_seq_len`` three steps before the end and its last tokens are dropped.  Step i starts from the
    lengths step i - 1 left."""
    starts = [0, 20, 40]
    scales = {} if kind == "bf16" else {"k_inv": 4.0, "v_inv": 2.0}
    max_seq_len = 70
    rope = real_tables(4096)
    first = make_problem(kind, 3, 1, 8, 2, 16, starts, max_seq_len=max_seq_len, rope=rope, reserve=max_seq_len,
                         **scales)
    out, lens = [], starts
    for i in range(steps):
        vals = random_values(100 + i, 3, 12, 1.0)
        p = make_problem(kind, 3, 1, 8, 2, 16, starts, max_seq_len=max_seq_len, rope=rope, values=vals,
                         reserve=max_seq_len, **scales)
        assert np.array_equal(p.table, first.table)
        out.append(dataclasses.replace(p, seq_lens=np.array(lens, dtype=np.int32), num_pages=first.num_pages))
        lens = [min(x + 1, max_seq_len) for x in lens]
    return out, lens


def chain_twin(problems) -> Result:
    """The caches and lengths the chain leaves, and the last step's ``q_out``: every step's twin laid over the last."""
    acc = None
    for p in problems:
        r = twin(p)
        if acc is None:
            acc = r
            continue
        for mine, new in ((acc.k, r.k), (acc.v, r.v)):
            for _, pp, slot in p.live():
                mine[GUARD + pp, :, slot] = new[GUARD + pp, :, slot]
        acc.q_out, acc.lens_out = r.q_out, r.lens_out
    return acc
