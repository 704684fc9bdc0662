"""A reference of what the step functions of ``samples/workload/main.py`` launch, and a check of every launch.

Plain Python on NumPy and torch, no GPU.  The step functions (``server_steps``, ``layer_steps``, ``generate_steps``,
``prefill_steps``) compose the library's kernels over rings of weights and KV caches by pointer arithmetic.  What lives
here, written from the module docstring of ``main.py`` and the contracts in ``gsx_kernels.h``:

* :func:`stages`: for a :class:`Config`, the launches a run has to make, in order.  A :class:`Stage` names the kernel
  (the method of the workload's ``Kernels``), and for every argument of that method either the named buffer and byte
  offset a pointer has to be (``None``: NULL) or the scalar's value.  Weights come from slot ``i % w_layers``, the
  cache from slot ``i % kv_layers``, the norm weights are row 0 or 1 of that weight slot, the plan is plan ``i``, the
  lengths ping-pong between ``lens0`` and ``lens1`` with ``start`` as the input of every step ``k % window == 0``, and
  the tokens alternate between ``tokens0`` and ``tokens1`` by step parity.
* :func:`check_trace`: given the initial bytes of every buffer and a trace (one :class:`Launch` per launch: the
  resolved arguments and the bytes of its outputs afterwards), it keeps a host mirror, compares every launch with its
  stage, computes the stage's reference from the mirror, that is from the inputs as the launch had them, and holds the
  outputs to that kernel's own contract: ``gemm_decode_cases.error_bound`` for every GEMM, ``kv_append_cases.twin``
  bit for bit (and every slot that was not written byte-equal to the mirror), the fp64 reference and bound of
  ``attn_decode_cases`` / ``attn_prefill_cases``, ``norm_act_cases.check_norm`` / ``check_silu`` (with SwiGLU's
  ``|g| <= 64`` precondition), ``moe_cases.route`` / ``weight_bound`` / ``combine`` and ``sample_cases.sample``.  No
  tolerance is new.  Every reference has a nonzero element in every row, so that no bound is met by zeros.  A failure
  is a :class:`StageError` that names the stage.
* :func:`simulate`: a whole trace made on the CPU by the kernels' twins (the GEMMs: an fp32 matmul rounded to bf16; the
  router's weights: ``weights64`` cast to fp32) from seeded initial buffers.  The checker accepts it.  With one of
  ``FLAWS`` it simulates a workload that is wrong in that way, and the checker rejects it at the stage
  :func:`flaw_cases` names.  ``tests/test_workload_cases.py`` checks all of this.
* :class:`Tracer` and :func:`run_traced`: the wrapper that stands where a step function expects its ``Kernels`` and
  records a trace.  With the library behind it (``tests/test_gpu_workload.py``) it forwards every launch to the GPU;
  with nothing behind it the twins compute every launch into the step function's own tensors in host memory, so the
  step functions' pointer arithmetic is held to :func:`stages` without a GPU too.
"""
from __future__ import annotations

import dataclasses
import functools
import inspect
import math
import types

import numpy as np
import torch

from tests import attn_decode_cases as ac
from tests import attn_prefill_cases as pc
from tests import gemm_decode_cases as dc
from tests import kv_append_cases as kc
from tests import moe_cases as mo
from tests import norm_act_cases as nc
from tests import sample_cases as sc

D = 128
WINDOW = 64  # steps after which the lengths start again (or the context, if that is less)
EPS = 1e-5
POISON = kc.POISON8  # what the tests fill every buffer with that the workload allocates and does not initialise


@dataclasses.dataclass(frozen=True)
class Config:
    name: str
    workload: str  # server, layer, generate or prefill
    steps: int
    kv_dtype: str = "bf16"
    batch: int = 3
    context: int = 40
    heads: int = 2
    kv_heads: int = 1
    page: int = 16
    ffn: int = 64
    w_layers: int = 2
    kv_layers: int = 2
    experts: int = 0
    active: int = 0
    chunk: int = 1
    vocab: int = 0
    temperature: float = 0.8
    top_k: int = 50
    top_p: float = 0.95
    seed: int = 0

    hidden = property(lambda c: c.heads * D)
    nqkv = property(lambda c: (c.heads + 2 * c.kv_heads) * D)
    per_seq = property(lambda c: -(-c.context // c.page))
    pages = property(lambda c: c.batch * c.per_seq)
    window = property(lambda c: min(WINDOW, c.context))
    layers = property(lambda c: max(c.w_layers, c.kv_layers))
    rows = property(lambda c: c.batch * c.chunk)
    pairs = property(lambda c: c.batch * max(c.active, 1))
    esz = property(lambda c: 2 if c.kv_dtype == "bf16" else 1)
    cache_bytes = property(lambda c: c.pages * c.kv_heads * c.page * D * c.esz)
    start = property(lambda c: c.context - (c.chunk if c.workload == "prefill" else c.window))

    def final_lens(self) -> int:
        """The lengths the last step leaves: ``window`` steps give ``context``."""
        return self.start + (self.steps - 1) % self.window + 1


_SERVER = dict(batch=3, heads=2, kv_heads=1, page=16, context=40, w_layers=2, kv_layers=3)
_LAYER = dict(batch=3, heads=4, kv_heads=2, ffn=64, context=80, w_layers=3, kv_layers=2)
_MOE = dict(experts=16, active=2, batch=5, heads=2, kv_heads=1, ffn=64, context=40, w_layers=2, kv_layers=2)
_GEN = dict(_LAYER, vocab=512, temperature=0.8, top_k=50, top_p=0.95, seed=7)
_PREFILL = dict(batch=2, chunk=64, context=80, heads=2, kv_heads=1, ffn=64, w_layers=2, kv_layers=3)
# The smallest runs at which each thing can still go wrong.  server: the window is the context (40), start is 0, the
# last page is partial, the window restarts once, the rings differ in length.  layer: the window is 64 and start 16, so
# the attention reads the caches' random initial contents, and layers 0 and 2 share a cache within a step.  MoE: 10
# pairs, and the plan's maximum of 128.  prefill: the second step rewrites the first.
CONFIGS = (
    Config("server-bf16", "server", 42, **_SERVER),
    Config("server-fp8", "server", 42, kv_dtype="fp8", **_SERVER),
    Config("layer-bf16", "layer", 3, **_LAYER),
    Config("layer-fp8", "layer", 3, kv_dtype="fp8", **_LAYER),
    Config("moe", "layer", 3, **_MOE),
    Config("moe-128-pairs", "layer", 2, **dict(_MOE, batch=16, active=8)),
    Config("generate", "generate", 5, **_GEN),
    Config("generate-moe", "generate", 3, **dict(_GEN, experts=16, active=2)),
    Config("generate-greedy", "generate", 3, **dict(_GEN, temperature=0.0)),
    Config("prefill-bf16", "prefill", 2, **_PREFILL),
    Config("prefill-fp8", "prefill", 2, kv_dtype="fp8", **_PREFILL),
)


def config(name: str) -> Config:
    return next(c for c in CONFIGS if c.name == name)


# ---- the buffers -----------------------------------------------------------------------------------------------------

def buffer_shapes(c: Config) -> dict[str, tuple[str, tuple]]:
    """``{name: (element type, shape)}`` of every tensor a step function addresses: bf16, kv (the cache's type), i32,
    f32, i64 or u8."""
    h, bf = c.hidden, "bf16"
    cache = ("kv", (c.kv_layers, c.pages, c.kv_heads, c.page, D))
    common = {"wqkv": (bf, (c.w_layers, c.nqkv, h)), "wo": (bf, (c.w_layers, h, h)), "kc": cache, "vc": cache,
              "table": ("i32", (c.batch, c.per_seq)), "cos": ("f32", (c.context, D // 2)),
              "sin": ("f32", (c.context, D // 2)), "x0": (bf, (c.rows, h)), "qkv": (bf, (c.rows, c.nqkv)),
              "q": (bf, (c.rows, c.heads, D)), "o": (bf, (c.rows, c.heads, D))}
    if c.workload == "prefill":
        common["lens"] = ("i32", (c.batch,))
    else:
        common.update({"start": ("i32", (c.batch,)), "lens0": ("i32", (c.batch,)), "lens1": ("i32", (c.batch,)),
                       "ws": ("u8", (_ws_bytes(c),))})
    if c.workload == "server":
        return {**common, "x1": (bf, (c.batch, h)), "x2": (bf, (c.batch, h))}
    nexp, rows = max(c.experts, 1), (c.rows if c.workload == "prefill" else c.pairs)
    out = {**common, "wgu": (bf, (c.w_layers, nexp * 2 * c.ffn, h)), "wdown": (bf, (c.w_layers, nexp * h, c.ffn)),
           "ln": (bf, (c.w_layers, 2, h)), "resid": (bf, (c.rows, h)), "xn": (bf, (c.rows, h)),
           "sub": (bf, (c.rows, h)), "gu": (bf, (rows, 2 * c.ffn)), "act": (bf, (rows, c.ffn))}
    if c.workload == "prefill":
        return out
    out.update({"router": (bf, (c.w_layers, c.experts, h)), "rlogits": (bf, (c.batch, c.experts)),
                "ids": ("i32", (c.pairs,)), "tw": ("f32", (c.pairs,)), "yexp": (bf, (c.pairs, h)),
                "plans": ("i32", (c.layers if c.experts else 0, mo.PLAN_INTS))})
    if c.workload == "generate":
        out.update({"embed": (bf, (c.vocab, h)), "head": (bf, (c.vocab, h)), "lnf": (bf, (h,)),
                    "logits": (bf, (c.batch, c.vocab)), "tokens0": ("i32", (c.batch,)), "tokens1": ("i32", (c.batch,)),
                    "temp": ("f32", (c.batch,)), "topk": ("i32", (c.batch,)), "topp": ("f32", (c.batch,)),
                    "seeds": ("i64", (c.batch,))})
    return out


def _ws_bytes(c: Config) -> int:
    """The simulation's attention workspace: room for every split's partial (the library tells the workload its own
    size; the checker takes any that the buffer holds)."""
    return c.batch * c.heads * ac.MAX_SPLITS * ac.PARTIAL_BYTES


# what the workload allocates without initialising it; the tests fill these with POISON before the first step
UNINITIALISED = {"server": ("qkv", "q", "o", "ws"),
                 "layer": ("qkv", "q", "o", "gu", "act", "ws", "rlogits", "ids", "tw", "yexp"),
                 "generate": ("qkv", "q", "o", "gu", "act", "ws", "rlogits", "ids", "tw", "yexp", "logits"),
                 "prefill": ("qkv", "q", "o", "gu", "act")}
_WRITTEN = {"server": ("kc", "vc", "lens0", "lens1", "x1", "x2"),
            "layer": ("kc", "vc", "lens0", "lens1", "resid", "xn", "sub", "plans"),
            "generate": ("kc", "vc", "lens0", "lens1", "resid", "xn", "sub", "plans", "x0", "tokens0", "tokens1"),
            "prefill": ("kc", "vc", "resid", "xn", "sub")}


def read_only(c: Config) -> list[str]:
    """The buffers no launch may change: weights, norm weights, the block table, ``start``, the RoPE tables, the input
    of layer 0 outside generate, the sampler's parameters, the embedding and the LM head."""
    return [n for n in buffer_shapes(c) if n not in UNINITIALISED[c.workload] and n not in _WRITTEN[c.workload]]


_NP = {"bf16": np.uint16, "i32": np.int32, "f32": np.float32, "i64": np.int64, "u8": np.uint8}


def initial_buffers(c: Config, seed: int = 0) -> dict[str, np.ndarray]:
    """Seeded initial bytes of every buffer, as the step functions make them: weights normal over the square root of
    their input width, norm weights 1, caches normal in the cache's type, the table a permutation of the pages."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, (kind, shape) in buffer_shapes(c).items():
        dt = (np.uint16 if c.kv_dtype == "bf16" else np.uint8) if kind == "kv" else _NP[kind]
        if name in UNINITIALISED[c.workload]:
            a = np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, POISON, np.uint8)
        elif kind == "kv":
            x = rng.standard_normal(shape).astype(np.float32)
            a = kc.bf16_bits(x) if c.kv_dtype == "bf16" else kc.e4m3_encode(x)
        elif name in ("wqkv", "wo", "wgu", "wdown", "router", "head"):
            a = kc.bf16_bits((rng.standard_normal(shape) / math.sqrt(shape[-1])).astype(np.float32))
        elif name in ("x0", "embed"):
            a = kc.bf16_bits(rng.standard_normal(shape).astype(np.float32))
        elif name in ("ln", "lnf"):
            a = kc.bf16_bits(np.ones(shape, np.float32))
        elif name == "table":
            a = rng.permutation(c.pages).astype(np.int32).reshape(shape)
        elif name in ("cos", "sin"):
            a = rope_tables(c.context)[name == "sin"]
        elif name in ("tokens0", "tokens1"):
            a = rng.integers(0, c.vocab, shape).astype(np.int32)
        else:
            fill = {"start": c.start, "lens": c.start, "temp": c.temperature, "topk": c.top_k, "topp": c.top_p}
            a = np.full(shape, fill.get(name, 0), dt)
            if name == "seeds":
                a = (np.arange(c.batch) + c.seed).astype(np.int64)
        out[name] = np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()
    return out


def rope_tables(rope_len: int):
    """cos and sin of ``pos * 10000^(-i / 64)``: fp64 rounded once to fp32."""
    inv = 10000.0 ** (-np.arange(D // 2, dtype=np.float64) / (D // 2))
    ang = np.arange(rope_len, dtype=np.float64)[:, None] * inv[None]
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def check_initial(c: Config, mem: dict[str, np.ndarray]) -> None:
    """What the checks below rely on in the buffers a run starts from."""
    shapes = buffer_shapes(c)
    for name, (kind, shape) in shapes.items():
        size = int(np.prod(shape)) * (c.esz if kind == "kv" else np.dtype(_NP[kind]).itemsize)
        if name == "ws":  # the library's own size
            assert len(mem[name]) >= 16, "ws"
            continue
        assert len(mem[name]) == size, f"{name}: {len(mem[name])} bytes, expected {size}"
    assert sorted(mem["table"].view(np.int32).tolist()) == list(range(c.pages)), "the block table is no permutation"
    assert (mem["lens" if c.workload == "prefill" else "start"].view(np.int32) == c.start).all(), "start"
    for name, tab in zip(("cos", "sin"), kc.real_tables(c.context)):
        assert np.abs(mem[name].view(np.float32).reshape(tab.shape).astype(np.float64) - tab).max() <= 2.0 ** -23, name
    if c.workload == "generate":
        assert mem["seeds"].view(np.int64).tolist() == [c.seed + r for r in range(c.batch)], "seeds"
        for name, dt, v in (("temp", np.float32, c.temperature), ("topk", np.int32, c.top_k),
                            ("topp", np.float32, c.top_p)):
            assert (mem[name].view(dt) == dt(v)).all(), name


# ---- the kernels' arguments ------------------------------------------------------------------------------------------

# the pointer arguments of each method of the workload's Kernels, and which of them the kernel writes
POINTERS = {"decode_gemm": ("a", "b", "c", "sa", "sb"), "gemm": ("a", "b", "c"),
            "kv_append": ("qkv", "q_out", "kc", "vc", "table", "lens", "lens_out", "cos", "sin"),
            "decode_attn": ("q", "kc", "vc", "table", "lens", "o", "ws"),
            "prefill_attn": ("q", "kc", "vc", "table", "lens", "o"),
            "add_rmsnorm": ("x", "r_in", "r_out", "w", "y"), "silu_mul": ("gu", "y"),
            "sample": ("logits", "temperature", "top_k", "top_p", "seeds", "tokens_out"),
            "embed_gather": ("table", "tokens", "out"), "moe_route": ("logits", "ids", "w", "plan"),
            "moe_gemm_nt": ("a", "b", "c", "plan", "sa", "sb"), "moe_combine": ("y", "w", "out")}
OUTPUTS = {"decode_gemm": ("c",), "gemm": ("c",), "kv_append": ("q_out", "kc", "vc", "lens_out"),
           "decode_attn": ("o", "ws"), "prefill_attn": ("o",), "add_rmsnorm": ("r_out", "y"), "silu_mul": ("y",),
           "sample": ("tokens_out",), "embed_gather": ("out",), "moe_route": ("ids", "w", "plan"),
           "moe_gemm_nt": ("c",), "moe_combine": ("out",)}
WS = "the workspace's size"  # ws_bytes: whatever the library asked for, inside the buffer


def extents(kernel: str, a: dict) -> dict[str, int]:
    """Bytes behind every pointer argument that the kernel may touch, from the scalars of the launch."""
    if kernel in ("decode_gemm", "gemm"):
        return {"a": a["m"] * a["k"] * 2, "b": a["n"] * a["k"] * 2, "c": a["m"] * a["n"] * 2}
    if kernel in ("kv_append", "decode_attn", "prefill_attn"):
        t = a.get("t", 1)
        cache = a["num_pages"] * a["hkv"] * a["page"] * D * (2 if a["kv_dtype"] == "bf16" else 1)
        qo = a["b"] * t * a["hq"] * D * 2
        out = {"kc": cache, "vc": cache, "table": a["b"] * a["table_stride"] * 4, "lens": a["b"] * 4}
        if kernel == "kv_append":
            return {**out, "qkv": a["b"] * t * a["qkv_stride"] * 2, "q_out": qo, "lens_out": a["b"] * 4,
                    "cos": a["rope_len"] * D * 2, "sin": a["rope_len"] * D * 2}
        return {**out, "q": qo, "o": qo, **({"ws": a["ws_bytes"]} if kernel == "decode_attn" else {})}
    if kernel == "add_rmsnorm":
        return {**{p: a["m"] * a["h"] * 2 for p in ("x", "r_in", "r_out", "y")}, "w": a["h"] * 2}
    if kernel == "silu_mul":
        return {"gu": a["m"] * a["i"] * 4, "y": a["m"] * a["i"] * 2}
    if kernel == "sample":
        return {"logits": a["m"] * a["v"] * 2, "temperature": a["m"] * 4, "top_k": a["m"] * 4, "top_p": a["m"] * 4,
                "seeds": a["m"] * 8, "tokens_out": a["m"] * 4}
    if kernel == "embed_gather":
        return {"table": a["v"] * a["h"] * 2, "tokens": a["m"] * 4, "out": a["m"] * a["h"] * 2}
    pairs = a["m"] * a["topk"]
    if kernel == "moe_route":
        return {"logits": a["m"] * a["e"] * 2, "ids": pairs * 4, "w": pairs * 4, "plan": mo.PLAN_INTS * 4}
    if kernel == "moe_gemm_nt":
        return {"a": -(-pairs // a["a_div"]) * a["k"] * 2, "b": a["e"] * a["n"] * a["k"] * 2, "c": pairs * a["n"] * 2,
                "plan": mo.PLAN_INTS * 4}
    assert kernel == "moe_combine", kernel
    return {"y": pairs * a["h"] * 2, "w": pairs * 4, "out": a["m"] * a["h"] * 2}


@dataclasses.dataclass(frozen=True)
class Stage:
    """One launch as it has to be: ``args`` holds, by the method's parameter names, ``(buffer, byte offset)`` or None
    for a pointer and the value of a scalar."""
    step: int
    layer: int | None
    label: str
    kernel: str
    args: dict

    def __str__(self):
        where = "" if self.layer is None else f"layer {self.layer}, "
        return f"step {self.step}, {where}{self.label} ({self.kernel})"


@dataclasses.dataclass
class Launch:
    """One launch as it was: the arguments resolved like a stage's, and the bytes behind every output pointer after
    it (``{parameter: uint8 array}``; a NULL output has none)."""
    kernel: str
    args: dict
    outputs: dict


class StageError(AssertionError):
    def __init__(self, index: int, stage: Stage | None, msg: str):
        super().__init__(f"launch {index}, {stage}: {msg}")
        self.index, self.stage = index, stage


# ---- the reference decoder: what is launched -------------------------------------------------------------------------

FLAWS = ("weight slot shifted", "cache slot shifted", "ln2 for ln1", "residual not restarted", "sub not added",
         "lengths not advanced", "attention on lens_in", "window never restarts", "rope a position late",
         "a_div 1 on up", "a_div topk on down", "swiglu on batch rows", "plan of layer 0", "combine reversed",
         "gate and up swapped", "tokens not alternated", "counter constant", "final norm into the residual",
         "prefill lengths after the chunk")
_NUMERIC = ("combine reversed", "gate and up swapped", "prefill lengths after the chunk")  # wrong inside a launch


def flaw_cases() -> dict[str, tuple[str, tuple]]:
    """``{flaw: (configuration that exposes it, (step, layer, label) of the first wrong stage)}``."""
    return {"weight slot shifted": ("layer-bf16", (0, 0, "norm1")),
            "cache slot shifted": ("layer-fp8", (0, 0, "append")),
            "ln2 for ln1": ("layer-bf16", (0, 0, "norm1")), "residual not restarted": ("layer-bf16", (0, 0, "norm1")),
            "sub not added": ("layer-bf16", (0, 1, "norm1")), "lengths not advanced": ("layer-bf16", (1, 0, "append")),
            "attention on lens_in": ("server-bf16", (0, 0, "attn")),
            "window never restarts": ("server-bf16", (40, 0, "append")),
            "rope a position late": ("server-fp8", (0, 0, "append")), "a_div 1 on up": ("moe", (0, 0, "up")),
            "a_div topk on down": ("moe", (0, 0, "down")), "swiglu on batch rows": ("moe", (0, 0, "swiglu")),
            "plan of layer 0": ("moe", (0, 1, "route")), "combine reversed": ("moe-128-pairs", (0, 0, "combine")),
            "gate and up swapped": ("layer-bf16", (0, 0, "swiglu")),
            "tokens not alternated": ("generate", (0, None, "sample")),
            "counter constant": ("generate", (1, None, "sample")),
            "final norm into the residual": ("generate", (0, None, "final norm")),
            "prefill lengths after the chunk": ("prefill-bf16", (0, 0, "attn"))}


def stages(c: Config, flaw: str | None = None) -> list[Stage]:
    """The launches of ``c.steps`` steps, in order.  ``flaw``: the launches of a workload that is wrong in that way
    (the flaws that are wrong inside a launch change nothing here: :func:`simulate` takes them)."""
    assert flaw is None or flaw in FLAWS
    h, out = c.hidden, []
    scale = 1.0 / math.sqrt(D)
    gemm = "gemm" if c.workload == "prefill" else "decode_gemm"

    def product(k, i, label, a, b, cc, m, n, kk):
        args = {"a": a, "b": b, "c": cc, "m": m, "n": n, "k": kk}
        if gemm == "decode_gemm":
            args.update({"dtype": "bf16", "sa": None, "sb": None})
        out.append(Stage(k, i, label, gemm, args))

    def norm(k, i, label, x, r_in, r_out, w, rows=c.rows):
        out.append(Stage(k, i, label, "add_rmsnorm", {"x": (x, 0), "r_in": r_in and (r_in, 0),
                                                      "r_out": r_out and (r_out, 0), "w": w, "y": ("xn", 0),
                                                      "m": rows, "h": h, "eps": EPS}))

    def lengths(k):
        if c.workload == "prefill":
            return "lens", None
        kk = k if flaw == "window never restarts" else k % c.window
        lens_in = "start" if kk == 0 or flaw == "lengths not advanced" else f"lens{(kk - 1) % 2}"
        return lens_in, f"lens{kk % 2}"

    def attention(k, i, x, wi, y):
        """The attention half of layer ``i``: QKV projection of ``x``, RoPE and append, attention, output projection
        into ``y``."""
        lens_in, lens_out = lengths(k)
        ci = ((i + 1) if flaw == "cache slot shifted" else i) % c.kv_layers
        kci, vci = ("kc", ci * c.cache_bytes), ("vc", ci * c.cache_bytes)
        late = D * 2 if flaw == "rope a position late" else 0  # one row of a table
        geometry = {"kv_dtype": c.kv_dtype, "kc": kci, "vc": vci, "table": ("table", 0), "b": c.batch, "hq": c.heads,
                    "hkv": c.kv_heads, "page": c.page, "num_pages": c.pages, "table_stride": c.per_seq,
                    "max_seq_len": c.context}
        product(k, i, "qkv", (x, 0), ("wqkv", wi * c.nqkv * h * 2), ("qkv", 0), c.rows, c.nqkv, h)
        out.append(Stage(k, i, "append", "kv_append", {
            **geometry, "qkv": ("qkv", 0), "qkv_stride": c.nqkv, "q_out": ("q", 0), "lens": (lens_in, 0),
            "lens_out": lens_out and (lens_out, 0), "cos": ("cos", late), "sin": ("sin", late),
            "rope_len": c.context - (1 if late else 0), "t": c.chunk}))
        if c.workload == "prefill":
            out.append(Stage(k, i, "attn", "prefill_attn", {**geometry, "q": ("q", 0), "lens": ("lens", 0),
                                                            "o": ("o", 0), "t": c.chunk, "scale": scale}))
        else:
            seen = lens_in if flaw == "attention on lens_in" else lens_out
            out.append(Stage(k, i, "attn", "decode_attn", {**geometry, "q": ("q", 0), "lens": (seen, 0), "o": ("o", 0),
                                                           "scale": scale, "ws": ("ws", 0), "ws_bytes": WS}))
        product(k, i, "out", ("o", 0), ("wo", wi * h * h * 2), (y, 0), c.rows, h, h)

    def mlp(k, i, wi):
        if not c.experts:
            product(k, i, "up", ("xn", 0), ("wgu", wi * 2 * c.ffn * h * 2), ("gu", 0), c.rows, 2 * c.ffn, h)
            out.append(Stage(k, i, "swiglu", "silu_mul", {"gu": ("gu", 0), "y": ("act", 0), "m": c.rows, "i": c.ffn}))
            product(k, i, "down", ("act", 0), ("wdown", wi * h * c.ffn * 2), ("sub", 0), c.rows, h, c.ffn)
            return
        e, topk = c.experts, c.active
        plan = ("plans", (0 if flaw == "plan of layer 0" else i) * mo.PLAN_INTS * 4)
        grouped = {"dtype": "bf16", "plan": plan, "m": c.batch, "topk": topk, "e": e, "sa": None, "sb": None, "mode": 0}
        product(k, i, "router", ("xn", 0), ("router", wi * e * h * 2), ("rlogits", 0), c.batch, e, h)
        out.append(Stage(k, i, "route", "moe_route", {"logits": ("rlogits", 0), "ids": ("ids", 0), "w": ("tw", 0),
                                                      "plan": plan, "m": c.batch, "e": e, "topk": topk}))
        out.append(Stage(k, i, "up", "moe_gemm_nt", {**grouped, "a": ("xn", 0),
                                                     "b": ("wgu", wi * e * 2 * c.ffn * h * 2),
                                                     "a_div": 1 if flaw == "a_div 1 on up" else topk, "c": ("gu", 0),
                                                     "n": 2 * c.ffn, "k": h}))
        out.append(Stage(k, i, "swiglu", "silu_mul", {"gu": ("gu", 0), "y": ("act", 0), "i": c.ffn,
                                                      "m": c.batch if flaw == "swiglu on batch rows" else c.pairs}))
        out.append(Stage(k, i, "down", "moe_gemm_nt", {**grouped, "a": ("act", 0),
                                                       "b": ("wdown", wi * e * h * c.ffn * 2),
                                                       "a_div": topk if flaw == "a_div topk on down" else 1,
                                                       "c": ("yexp", 0), "n": h, "k": c.ffn}))
        out.append(Stage(k, i, "combine", "moe_combine", {"y": ("yexp", 0), "w": ("tw", 0), "out": ("sub", 0),
                                                          "m": c.batch, "topk": topk, "h": h}))

    for k in range(c.steps):
        if c.workload == "server":
            for i in range(c.layers):
                wi = ((i + 1) if flaw == "weight slot shifted" else i) % c.w_layers
                attention(k, i, "x0" if i == 0 else f"x{1 + i % 2}", wi, f"x{1 + (i + 1) % 2}")
            continue
        if c.workload == "generate":
            src = 0 if flaw == "tokens not alternated" else k % 2
            out.append(Stage(k, None, "gather", "embed_gather", {"table": ("embed", 0), "tokens": (f"tokens{src}", 0),
                                                                 "out": ("x0", 0), "m": c.batch, "h": h, "v": c.vocab}))
        for i in range(c.layers):
            wi = ((i + 1) if flaw == "weight slot shifted" else i) % c.w_layers
            ln1 = ("ln", (wi * 2 + (1 if flaw == "ln2 for ln1" else 0)) * h * 2)
            if i == 0 and flaw != "residual not restarted":  # the residual stream starts afresh
                norm(k, i, "norm1", "x0", None, "resid", ln1)
            elif i > 0 and flaw == "sub not added":
                norm(k, i, "norm1", "sub", None, "resid", ln1)
            else:
                norm(k, i, "norm1", "sub", "resid", "resid", ln1)
            attention(k, i, "xn", wi, "sub")
            norm(k, i, "norm2", "sub", "resid", "resid", ("ln", (wi * 2 + 1) * h * 2))
            mlp(k, i, wi)
        if c.workload == "generate":
            dst = 0 if flaw == "tokens not alternated" else (k + 1) % 2
            norm(k, None, "final norm", "sub", "resid", "resid" if flaw == "final norm into the residual" else None,
                 ("lnf", 0))
            product(k, None, "head", ("xn", 0), ("head", 0), ("logits", 0), c.batch, c.vocab, h)
            out.append(Stage(k, None, "sample", "sample", {
                "logits": ("logits", 0), "temperature": ("temp", 0), "top_k": ("topk", 0), "top_p": ("topp", 0),
                "seeds": ("seeds", 0), "counter": 0 if flaw == "counter constant" else k,
                "tokens_out": (f"tokens{dst}", 0), "m": c.batch, "v": c.vocab}))
    return out


# ---- one launch: its inputs from the mirror, its twin, its check -----------------------------------------------------

class Memory:
    """The host mirror: ``{name: uint8 array}``, read and written through ``(name, byte offset)``."""

    def __init__(self, buffers: dict[str, np.ndarray]):
        self.b = {n: np.array(a, dtype=np.uint8).reshape(-1) for n, a in buffers.items()}

    def read(self, ptr, shape, dtype) -> np.ndarray:
        name, off = ptr
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        assert 0 <= off and off + n <= len(self.b[name]), f"{name} + {off}: {n} bytes run past its {len(self.b[name])}"
        return self.b[name][off:off + n].copy().view(dtype).reshape(shape)

    def write(self, ptr, data: np.ndarray) -> None:
        name, off = ptr
        raw = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        assert 0 <= off and off + len(raw) <= len(self.b[name]), f"{name} + {off}: {len(raw)} bytes run past its end"
        self.b[name][off:off + len(raw)] = raw


def _t16(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def _nonzero_rows(ref, what: str) -> None:
    ref = np.asarray(ref)
    assert bool((ref.reshape(ref.shape[0], -1) != 0).any(axis=1).all()), f"{what}: a row of the reference is all zeros"


def _gemm_operands(kernel: str, a: dict, mem: Memory):
    """``(A rows [P][K], B rows [P or 1][N][K])`` as bf16 tensors: one B for all rows, or a pair's expert's."""
    if kernel != "moe_gemm_nt":
        return (_t16(mem.read(a["a"], (a["m"], a["k"]), np.uint16)),
                _t16(mem.read(a["b"], (1, a["n"], a["k"]), np.uint16)))
    pairs = a["m"] * a["topk"]
    n_active, p, e, expert, begin, count, rows = mo.plan_fields(mem.read(a["plan"], (mo.PLAN_INTS,), np.int32))
    assert (p, e) == (pairs, a["e"]), f"the plan is for {p} pairs of {e} experts"
    of = np.full(pairs, -1)
    for s in range(n_active):
        of[rows[begin[s]:begin[s] + count[s]]] = expert[s]
    assert (of >= 0).all() and (of < e).all(), "the plan leaves a pair without an expert"
    am = _t16(mem.read(a["a"], (-(-pairs // a["a_div"]), a["k"]), np.uint16))
    bm = _t16(mem.read(a["b"], (e, a["n"], a["k"]), np.uint16))
    return am[np.arange(pairs) // a["a_div"]], bm[of]


def _append_problem(a: dict, mem: Memory) -> kc.Problem:
    rows = a["b"] * a["t"]
    return kc.Problem(a["kv_dtype"], mem.read(a["qkv"], (rows, a["qkv_stride"]), np.uint16), a["b"], a["t"], a["hq"],
                      a["hkv"], a["page"], a["num_pages"], mem.read(a["table"], (a["b"], a["table_stride"]), np.int32),
                      mem.read(a["lens"], (a["b"],), np.int32), a["max_seq_len"],
                      mem.read(a["cos"], (a["rope_len"], D // 2), np.float32),
                      mem.read(a["sin"], (a["rope_len"], D // 2), np.float32))


def _append_twin(a: dict, mem: Memory):
    """``(problem, q_out, K cache, V cache, written[page][head][slot], lens_out)``: the caches as the mirror has them
    with the twin's slots of the live tokens laid over."""
    p = _append_problem(a, mem)
    r = kc.twin(p)
    shape = (p.num_pages, p.hkv, p.page, D)
    cdt = np.uint16 if p.kind == "bf16" else np.uint8
    k, v = mem.read(a["kc"], shape, cdt), mem.read(a["vc"], shape, cdt)
    written = np.zeros(shape[:3], bool)
    for _, pp, slot in p.live():
        k[pp, :, slot], v[pp, :, slot] = r.k[kc.GUARD + pp, :, slot], r.v[kc.GUARD + pp, :, slot]
        written[pp, :, slot] = True
    return p, r.q_out, k, v, written, r.lens_out


def _cache(a: dict, mem: Memory, ptr) -> torch.Tensor:
    shape = (a["num_pages"], a["hkv"], a["page"], D)
    if a["kv_dtype"] == "bf16":
        return _t16(mem.read(ptr, shape, np.uint16))
    return torch.from_numpy(mem.read(ptr, shape, np.uint8)).view(ac.FP8)


def _attn_problem(kernel: str, a: dict, mem: Memory, after_chunk: bool = False):
    t = a.get("t", 1)
    q = _t16(mem.read(a["q"], (a["b"] * t, a["hq"], D), np.uint16))
    table = torch.from_numpy(mem.read(a["table"], (a["b"], a["table_stride"]), np.int32))
    lens = torch.from_numpy(mem.read(a["lens"], (a["b"],), np.int32))
    k, v = _cache(a, mem, a["kc"]), _cache(a, mem, a["vc"])
    if kernel == "decode_attn":
        return ac.Problem(a["kv_dtype"], q, k, v, table, lens, a["max_seq_len"], a["scale"])
    return pc.Problem(a["kv_dtype"], q, k, v, table, lens + (t if after_chunk else 0), t, a["max_seq_len"], a["scale"])


def _norm_problem(a: dict, mem: Memory) -> nc.NormProblem:
    m, h = a["m"], a["h"]
    r = None if a["r_in"] is None else mem.read(a["r_in"], (m, h), np.uint16)
    mode = None if a["r_out"] is None else "inplace" if a["r_out"] == a["r_in"] else "new"
    return nc.NormProblem(mem.read(a["x"], (m, h), np.uint16), r, mem.read(a["w"], (h,), np.uint16), h,
                          float(np.float32(a["eps"])), mode)


def _sample_rows(a: dict, mem: Memory):
    m = a["m"]
    return (mem.read(a["logits"], (m, a["v"]), np.uint16), mem.read(a["temperature"], (m,), np.float32),
            mem.read(a["top_k"], (m,), np.int32), mem.read(a["top_p"], (m,), np.float32),
            mem.read(a["seeds"], (m,), np.int64))


def run_twin(kernel: str, a: dict, mem: Memory, flaw: str | None = None) -> dict[str, np.ndarray]:
    """The launch on the CPU, by the kernel's twin: ``{output parameter: array}`` (NULL outputs left out)."""
    if kernel in ("decode_gemm", "gemm", "moe_gemm_nt"):
        am, bm = _gemm_operands(kernel, a, mem)
        return {"c": _bits(torch.einsum("pk,pnk->pn", am.float(), bm.float().expand(am.shape[0], -1, -1)).bfloat16())}
    if kernel == "kv_append":
        _, q_out, k, v, _, lens_out = _append_twin(a, mem)
        return {"q_out": q_out, "kc": k, "vc": v, **({} if a["lens_out"] is None else {"lens_out": lens_out})}
    if kernel == "decode_attn":
        ws = mem.read(a["ws"], (len(mem.b[a["ws"][0]]) - a["ws"][1],), np.uint8)
        return {"o": _bits(ac.twin(_attn_problem(kernel, a, mem))), "ws": ws}
    if kernel == "prefill_attn":
        return {"o": _bits(pc.twin(_attn_problem(kernel, a, mem, flaw == "prefill lengths after the chunk")))}
    if kernel == "add_rmsnorm":
        r = nc.norm_twin(_norm_problem(a, mem), "bf16")
        return {"y": r.y, **({} if r.r_out is None else {"r_out": r.r_out})}
    if kernel == "silu_mul":
        p = nc.SiluProblem(mem.read(a["gu"], (a["m"], 2 * a["i"]), np.uint16), a["i"])
        return {"y": nc.silu_twin(p, "bf16", "swap gate and up" if flaw == "gate and up swapped" else None).y}
    if kernel == "moe_route":
        ids, w64, plan = mo.route(mem.read(a["logits"], (a["m"], a["e"]), np.uint16), a["topk"])
        return {"ids": ids, "w": w64.astype(np.float32), "plan": plan}
    if kernel == "moe_combine":
        y = mem.read(a["y"], (a["m"] * a["topk"], a["h"]), np.uint16)
        w = mem.read(a["w"], (a["m"], a["topk"]), np.float32)
        # the flaw: the weights meet the experts' outputs in the reverse order of ids
        return {"out": mo.combine(y, w[:, ::-1] if flaw == "combine reversed" else w)}
    if kernel == "embed_gather":
        return {"out": sc.embed_reference(mem.read(a["table"], (a["v"], a["h"]), np.uint16),
                                          mem.read(a["tokens"], (a["m"],), np.int32), a["h"])}
    assert kernel == "sample", kernel
    bits, temp, topk, topp, seeds = _sample_rows(a, mem)
    return {"tokens_out": np.array([sc.sample(bits[r], temp[r], int(topk[r]), topp[r], int(seeds[r]), a["counter"])
                                    for r in range(a["m"])], np.int32)}


def _differ(got: np.ndarray, want: np.ndarray, what: str) -> None:
    bad = np.argwhere(got != want)
    assert not len(bad), (f"{what}: {len(bad)} of {got.size} elements differ, first at {bad[0].tolist()}: got "
                          f"{int(got[tuple(bad[0])]):#x}, want {int(want[tuple(bad[0])]):#x}")


def check_launch(c: Config, kernel: str, a: dict, mem: Memory, out: dict[str, np.ndarray]) -> None:
    """The outputs ``out`` (raw bytes by parameter) of one launch against the reference of its inputs in ``mem``, under
    the kernel's own contract."""
    def got(param, shape, dtype):
        return out[param].view(dtype).reshape(shape)

    if kernel in ("decode_gemm", "gemm", "moe_gemm_nt"):
        am, bm = _gemm_operands(kernel, a, mem)
        a64, b64 = am.double(), bm.double().expand(am.shape[0], -1, -1)
        ref, mag = torch.einsum("pk,pnk->pn", a64, b64), torch.einsum("pk,pnk->pn", a64.abs(), b64.abs())
        _nonzero_rows(ref.numpy(), "the product")
        err = (_t16(got("c", tuple(ref.shape), np.uint16)).double() - ref).abs()
        bad = ~(err <= dc.error_bound(ref, mag, a["k"]))  # a NaN is inside no bound
        if bool(bad.any()):
            r, n = (int(x) for x in bad.nonzero()[0])
            raise AssertionError(f"{int(bad.sum())} of {bad.numel()} elements outside the bound, first at ({r}, {n}): "
                                 f"off by {float(err[r, n])!r} from {float(ref[r, n])!r}")
    elif kernel == "kv_append":
        p, q_out, k, v, written, lens_out = _append_twin(a, mem)
        assert len(p.live()) == p.b * p.t, "a new token has no slot: the lengths ran past the context"
        _nonzero_rows(kc.bf16_value(q_out), "Q_out")
        _differ(got("q_out", q_out.shape, np.uint16), q_out, "Q_out")
        for name, param, want in (("K_cache", "kc", k), ("V_cache", "vc", v)):
            g = got(param, want.shape, want.dtype)
            same = (g == want) | (written[..., None] & kc.same_e4m3(g, want) if p.kind == "fp8" else False)
            _differ(np.where(same, want, g), want, name)  # an unwritten slot: byte for byte
        if a["lens_out"] is not None:
            assert got("lens_out", (p.b,), np.int32).tolist() == lens_out.tolist(), "lens_out"
    elif kernel in ("decode_attn", "prefill_attn"):
        p = _attn_problem(kernel, a, mem)
        ref, bound = (ac.reference(p), ac.error_bound(p)[0]) if kernel == "decode_attn" else pc.error_bound(p)[1::-1]
        _nonzero_rows(ref, "the attention")
        err = np.abs(kc.bf16_value(got("o", ref.shape, np.uint16)).astype(np.float64) - ref)
        bad = ~(err <= bound)
        if bad.any():
            at = tuple(int(x) for x in np.argwhere(bad)[0])
            raise AssertionError(f"{int(bad.sum())} of {bad.size} elements of O outside the bound, first at (row, "
                                 f"head, d) {at}: off by {err[at]!r} from {ref[at]!r}, bound {bound[at]!r}")
    elif kernel == "add_rmsnorm":
        p = _norm_problem(a, mem)
        _nonzero_rows(nc.norm_reference(p), "the norm")
        r_out = None if a["r_out"] is None else got("r_out", (p.m, p.h), np.uint16)
        nc.check_norm(p, "bf16", nc.Result(got("y", (p.m, p.h), np.uint16), None, r_out), "add + RMSNorm")
    elif kernel == "silu_mul":
        p = nc.SiluProblem(mem.read(a["gu"], (a["m"], 2 * a["i"]), np.uint16), a["i"])
        assert float(np.abs(nc.silu_inputs(p)[0]).max()) <= 64, "a gate beyond the contract's |g| <= 64"
        _nonzero_rows(nc.silu_reference(p)[0], "SwiGLU")
        nc.check_silu(p, "bf16", nc.Result(got("y", (a["m"], a["i"]), np.uint16)), "SwiGLU")
    elif kernel == "moe_route":
        bits = mem.read(a["logits"], (a["m"], a["e"]), np.uint16)
        ids, w64, plan = mo.route(bits, a["topk"])
        _nonzero_rows(w64, "the router's weights")
        assert np.array_equal(got("ids", ids.shape, np.int32), ids), f"ids, want {ids.tolist()}"
        _differ(got("plan", plan.shape, np.int32), plan, "the plan")
        w, bound = got("w", ids.shape, np.float32).astype(np.float64), mo.weight_bound(bits, ids, w64)
        assert not np.isnan(w).any() and (np.abs(w - w64) <= bound).all(), \
            f"a weight is off by {np.abs(w - w64).max()!r}"
        assert np.array_equal(w[bound == 0], w64[bound == 0]), "a weight that is exactly 0 or 1 is not"
    elif kernel == "moe_combine":
        want = run_twin(kernel, a, mem)["out"]
        _nonzero_rows(want, "the combine")
        g = got("out", want.shape, np.uint16)
        nan = (want & 0x7FFF) > 0x7F80
        assert (((g & 0x7FFF) > 0x7F80) == nan).all(), "NaN where none is due, or none where one is"
        _differ(np.where(nan, want, g), want, "out")
    elif kernel == "embed_gather":
        tokens = mem.read(a["tokens"], (a["m"],), np.int32)
        assert ((tokens >= 0) & (tokens < a["v"])).all(), f"a token outside [0, {a['v']}): {tokens.tolist()}"
        want = run_twin(kernel, a, mem)["out"]
        _nonzero_rows(want, "the gather")
        _differ(got("out", want.shape, np.uint16), want, "the rows")
    else:
        assert kernel == "sample", kernel
        assert mem.read(a["seeds"], (a["m"],), np.int64).tolist() == [c.seed + r for r in range(a["m"])], "seeds"
        want = run_twin(kernel, a, mem)["tokens_out"]
        assert got("tokens_out", want.shape, np.int32).tolist() == want.tolist(), \
            f"tokens {got('tokens_out', want.shape, np.int32).tolist()}, want {want.tolist()} at counter {a['counter']}"


def same_args(st: Stage | None, kernel: str, args: dict, room: int) -> None:
    """The launch ``kernel(args)`` is the stage ``st``; ``room``: the bytes of the attention's workspace buffer."""
    assert st is not None, f"a launch too many ({kernel})"
    assert kernel == st.kernel, f"{kernel} was launched"
    assert sorted(args) == sorted(st.args), f"arguments {sorted(args)}, expected {sorted(st.args)}"
    for name, want in st.args.items():
        have = args[name]
        if want is WS:
            assert 0 <= have <= room and (have == room or room == 16), f"ws_bytes {have} with a workspace of {room}"
        elif isinstance(want, tuple):
            assert have == want, f"{name} is " + ("NULL" if have is None else f"{have[0]} + {have[1]}") \
                + f", expected {want[0]} + {want[1]}"
        else:
            assert have == want and type(have) is type(want), f"{name} is {have!r}, expected {want!r}"


def check_trace(c: Config, initial: dict[str, np.ndarray], trace: list[Launch], step_ends=None) -> Memory:
    """Every launch of ``trace`` against :func:`stages` and its own reference; returns the mirror after the last.
    ``step_ends``, if given, holds every buffer's bytes as they were after each step: they have to equal the mirror's,
    so that a launch that wrote what it does not own is found."""
    check_initial(c, initial)
    mem = Memory(initial)
    want = stages(c)
    sampled = None
    for i, la in enumerate(trace):
        st = want[i] if i < len(want) else None
        try:
            same_args(st, la.kernel, la.args, len(mem.b.get("ws", ())))
            ext = extents(la.kernel, la.args)
            for param in OUTPUTS[la.kernel]:
                if la.args[param] is not None:
                    assert param in la.outputs and len(la.outputs[param]) == ext[param], f"the output {param}"
            if st.label == "gather" and sampled is not None:
                assert la.args["tokens"] == sampled[0] and np.array_equal(
                    mem.read(la.args["tokens"], (c.batch,), np.int32), sampled[1]), "not the tokens of the step before"
            check_launch(c, la.kernel, la.args, mem, la.outputs)
        except AssertionError as e:
            raise StageError(i, st, str(e)) from e
        for param, data in la.outputs.items():
            mem.write(la.args[param], data)
        if st.label == "sample":
            sampled = (la.args["tokens_out"], la.outputs["tokens_out"].view(np.int32).copy())
        last = i + 1 == len(want) or want[i + 1].step != st.step
        if last and step_ends is not None:
            for name, have in step_ends[st.step].items():
                if not np.array_equal(np.asarray(have).reshape(-1).view(np.uint8), mem.b[name]):
                    at = int(np.flatnonzero(np.asarray(have).reshape(-1).view(np.uint8) != mem.b[name])[0])
                    raise StageError(i, st, f"after step {st.step} {name} differs from what its launches wrote, first "
                                            f"at byte {at}: something else wrote it")
    if len(trace) != len(want):
        raise StageError(len(trace), want[len(trace)], "was never launched")
    for name in read_only(c):
        assert np.array_equal(mem.b[name], np.asarray(initial[name]).reshape(-1).view(np.uint8)), f"{name} was written"
    if c.workload != "prefill":
        k = (c.steps - 1) % c.window
        assert mem.b[f"lens{k % 2}"].view(np.int32).tolist() == [c.final_lens()] * c.batch, "the final lengths"
    return mem


def covered_buffers(c: Config) -> set[str]:
    """The buffers some stage of ``c`` addresses."""
    return {v[0] for st in stages(c) for k, v in st.args.items() if k in POINTERS[st.kernel] and v is not None}


# ---- the simulation --------------------------------------------------------------------------------------------------

def simulate(c: Config, steps: int | None = None, flaw: str | None = None, seed: int = 0):
    """``(config, initial buffers, trace, step_ends)`` of ``steps`` steps (default: the configuration's) run by the
    twins.  ``flaw``: the workload is wrong in that way."""
    c = c if steps is None else dataclasses.replace(c, steps=steps)
    initial = initial_buffers(c, seed)
    mem = Memory(initial)
    trace, step_ends = [], []
    todo = stages(c, flaw)
    for i, st in enumerate(todo):
        a = dict(st.args)
        if a.get("ws_bytes") is WS:
            a["ws_bytes"] = len(mem.b["ws"])
        try:
            out = {p: np.ascontiguousarray(v).reshape(-1).view(np.uint8).copy()
                   for p, v in run_twin(st.kernel, a, mem, flaw if flaw in _NUMERIC else None).items()}
        except (AssertionError, IndexError):
            if flaw is None:
                raise
            trace.append(Launch(st.kernel, a, {}))  # a launch the twins cannot follow: the trace ends with it
            break
        for p, data in out.items():
            mem.write(a[p], data)
        trace.append(Launch(st.kernel, a, out))
        if i + 1 == len(todo) or todo[i + 1].step != st.step:
            step_ends.append({n: b.copy() for n, b in mem.b.items()})
    return c, initial, trace, step_ends


@functools.lru_cache(maxsize=None)
def simulated(name: str):
    """The simulation of a configuration of ``CONFIGS``, made once and shared: not to be written to."""
    return simulate(config(name))


# ---- the step functions themselves, traced ---------------------------------------------------------------------------

def tensor_bytes(t) -> np.ndarray:
    """A copy of a tensor's bytes, from the device or the host."""
    return t.reshape(-1).view(torch.uint8).cpu().numpy().copy() if t.numel() else np.zeros(0, np.uint8)


def download(buffers) -> dict[str, np.ndarray]:
    return {n: tensor_bytes(t) for n, t in buffers.items()}


class HostTorch:
    """torch for a step function that runs on the host: there is no device to wait for."""

    cuda = types.SimpleNamespace(synchronize=lambda *a: None)

    def __getattr__(self, name):
        return getattr(torch, name)


class Tracer:
    """What a step function takes for its ``Kernels``.  For every kernel method, in order: each pointer argument is
    resolved to ``(buffer name, byte offset)`` through ``step.buffers`` (an address inside no buffer, or an extent past
    a buffer's end, fails); the launch is compared with the stage :func:`stages` has at its place, and one that is not
    the reference's is refused, so that no wrong pointer reaches a device; the call is forwarded and the stream
    synchronised; the launch's outputs are read back; the launch joins the trace.  ``kl`` and ``gs`` are the library
    and its stream, or None: then the twins run every launch on the tensors in host memory.  Everything that is not a
    kernel is the library's own (without one: a workspace size, and a ``sync`` that has nothing to wait for)."""

    def __init__(self, module, c: Config, kl=None, gs=None):
        self.sigs = {n: inspect.signature(getattr(module.Kernels, n)) for n in POINTERS}
        self.kl, self.gs, self.want = kl, gs, stages(c)
        self.buffers, self.spans, self.mem, self.trace = None, [], None, []

    def attach(self, buffers) -> None:
        self.buffers = dict(buffers)
        self.spans = [(t.data_ptr(), t.numel() * t.element_size(), n) for n, t in buffers.items() if t.numel()]
        if self.kl is None:  # the mirror IS the tensors' memory
            self.mem = Memory({})
            self.mem.b = {n: t.reshape(-1).view(torch.uint8).numpy() if t.numel() else np.zeros(0, np.uint8)
                          for n, t in buffers.items()}

    def resolve(self, addr: int):
        if not addr:
            return None
        for base, size, name in self.spans:
            if base <= addr < base + size:
                return name, addr - base
        raise AssertionError(f"the address {addr:#x} lies in none of the workload's buffers")

    def __getattr__(self, name):
        if name not in POINTERS:
            if self.kl is not None:
                return getattr(self.kl, name)
            return {"attn_workspace_bytes": lambda b, hq, page, max_seq_len: b * hq * ac.MAX_SPLITS * ac.PARTIAL_BYTES,
                    "sync": lambda s: None}[name]

        def call(*args, **kw):
            bound = self.sigs[name].bind(None, *args, **kw)
            bound.apply_defaults()
            a = dict(bound.arguments)
            del a["self"]
            assert a.pop("s") is self.gs, "another stream"
            i = len(self.trace)
            st = self.want[i] if i < len(self.want) else None
            try:
                for p in POINTERS[name]:
                    a[p] = self.resolve(a[p])
                same_args(st, name, a, self.buffers["ws"].numel() if "ws" in self.buffers else 0)
                ext = extents(name, a)
                for p in POINTERS[name]:
                    if a[p] is not None:
                        room = self.buffers[a[p][0]].numel() * self.buffers[a[p][0]].element_size()
                        assert a[p][1] + ext[p] <= room, f"{p}: {ext[p]} bytes at {a[p][0]} + {a[p][1]} run past {room}"
            except AssertionError as e:
                raise StageError(i, st, str(e)) from e
            if self.kl is not None:
                getattr(self.kl, name)(*args, **kw)
                self.kl.sync(self.gs)
                out = {p: tensor_bytes(self.buffers[a[p][0]])[a[p][1]:a[p][1] + ext[p]]
                       for p in OUTPUTS[name] if a[p] is not None}
            else:
                out = {p: np.ascontiguousarray(v).reshape(-1).view(np.uint8)[:ext[p]].copy()
                       for p, v in run_twin(name, a, self.mem).items()}
                for p, data in out.items():
                    self.mem.write(a[p], data)
            self.trace.append(Launch(name, a, out))

        return call


def build_steps(module, c: Config, kl, gs, seed: int, torch_=torch, dev=None):
    """``(step, sync, finite)`` of the configuration from the workload's own step function, seeded, with the buffers
    it leaves uninitialised filled with :data:`POISON` (so that two runs start from the same bytes)."""
    torch.manual_seed(seed)
    dev = torch.device("cuda", 0) if dev is None else dev
    shape = (c.kv_dtype, c.batch, c.context, c.heads, c.kv_heads, c.page)
    if c.workload == "server":
        r = module.server_steps(torch_, kl, gs, dev, *shape, c.w_layers, c.kv_layers)
    elif c.workload == "layer":
        r = module.layer_steps(torch_, kl, gs, dev, *shape, c.ffn, c.w_layers, c.kv_layers, c.experts, c.active)
    elif c.workload == "generate":
        r = module.generate_steps(torch_, kl, gs, dev, *shape, c.ffn, c.w_layers, c.kv_layers, c.vocab, c.temperature,
                                  c.top_k, c.top_p, c.seed, c.experts, c.active)
    else:
        r = module.prefill_steps(torch_, kl, gs, dev, c.kv_dtype, c.batch, c.chunk, c.context, c.heads, c.kv_heads,
                                 c.page, c.ffn, c.w_layers, c.kv_layers)
    step, sync, finite = r[:3]
    assert set(step.buffers) == set(buffer_shapes(c)), sorted(set(step.buffers) ^ set(buffer_shapes(c)))
    for n in UNINITIALISED[c.workload]:
        if step.buffers[n].numel():
            step.buffers[n].view(torch.uint8).fill_(POISON)
    torch_.cuda.synchronize()  # the library's stream does not wait for torch's
    return step, sync, finite


def run_traced(module, c: Config, kl=None, gs=None, seed: int = 0):
    """``(initial buffers, trace, buffers after every step, finite())`` of ``c.steps`` traced steps of the workload's
    step function: on the GPU through the library ``kl`` and its stream, or on the host by the twins."""
    tracer = Tracer(module, c, kl, gs)
    host = kl is None
    step, sync, finite = build_steps(module, c, tracer, gs, seed, HostTorch() if host else torch,
                                     torch.device("cpu") if host else None)
    tracer.attach(step.buffers)
    initial, ends = download(step.buffers), []
    for _ in range(c.steps):
        step()
        sync()
        ends.append(download(step.buffers))
    return initial, tracer.trace, ends, finite()
