"""The sample pod workload: a PyTorch-ROCm / HIP GEMM loop that stays inside its GPU share.

Self-contained (the container image holds this file, ``run.sh`` and the ``libgsx_kernels.so`` its Dockerfile
builds; nothing else of this repository): counterpart of the reference's sample container
(``samples/docker/main.py``: TF1 with ``per_process_gpu_memory_fraction`` from ``SHARED_GPU_MEM_DEV`` /
``_CONTAINER``, a tiny matmul forever).  Here:

* the memory share becomes ``torch.cuda.set_per_process_memory_fraction`` (allocated / device total), so the
  caching allocator refuses to grow past the pod's gpu-mem;
* a CU partition handed out by the device plugin (``GSX_CU_MASK`` words) is applied by running the work on a
  ``hipExtStreamCreateWithCUMask`` stream; ``HSA_CU_MASK`` (set by the plugin too) restricts every queue of the
  process, including torch's own;
* the compute is the bf16 MFMA GEMM of ``libgsx_kernels.so`` (``--kernel gsx``, found next to this file, at
  ``$GSX_KERNELS_LIB``, or in the repository's build tree) or ``torch.matmul`` / hipBLASLt (``--kernel torch``);
  ``auto`` (default) takes the MFMA kernel when the library is there and says so when it falls back;
* ``--dtype fp8`` runs the same loop on OCP e4m3 operands: the library's fp8 GEMM, or ``torch._scaled_mm``;
* ``--dtype mxfp4`` runs it on MXFP4 operands (e2m1 with e8m0 block scales), made by quantising the random bf16
  matrices with the library's ``gsx_quant_mxfp4``: the library's mxfp4 GEMM only, ``--kernel torch`` has none;
* ``--workload decode`` is an inference server's decode phase instead of the large GEMM: ``--batch`` (1..16)
  activation rows against a ring of ``--size`` x ``--size`` weight matrices, one launch per matrix and step.  The
  ring (``--weights-gib``; 4 GiB or a quarter of the share) is larger than the 256 MiB Infinity Cache, so the weights
  come from HBM every time: the work is bound by memory bandwidth, and the result reports ``tbps``, the weight and
  weight-scale bytes streamed per second, next to ``tflops``.  The library's decode GEMM, or ``torch.matmul`` /
  ``torch._scaled_mm`` on the same ring;
* ``--workload attn`` is the other half of a decode step: attention of one new token per sequence over a paged KV
  cache.  ``--batch`` sequences (1..256) of ``--context`` tokens each, ``--heads`` query heads sharing ``--kv-heads``
  KV heads at D = 128, pages of ``--page`` tokens handed out through a random permutation, as an allocator leaves
  them after churn, in bf16 or e4m3 (``--kv-dtype``).  A server has one KV cache per layer: the workload keeps a ring
  of per-layer caches (``--kv-gib``; 4 GiB or a quarter of the share, never fewer than two layers) and runs one
  attention per layer and step, so a step streams more than the Infinity Cache.  It reports ``tbps`` (KV bytes read
  per second) and ``tokens_per_s``.  The library's decode attention, or (``--kernel torch``, bf16 only)
  ``scaled_dot_product_attention(enable_gqa=True)`` on a contiguous copy of the same data;
* ``--workload server`` is a whole decode layer per ring layer and step, on the library's kernels only: the fused QKV
  projection of ``--batch`` rows (1..16; hidden = ``--heads`` x 128, bf16 weights) through the decode GEMM, RoPE and
  the append of the new token's K and V to the layer's paged cache (``gsx_kv_append``; ``--kv-dtype`` selects the
  cache), the decode attention over the cache that has just grown, and the output projection, which gives the next
  layer's activations.  Nothing in a step waits for the host.  The sequence lengths live on the device and grow from
  ``--context`` minus a window to ``--context``, then start again, so the run can go on forever.  The weight ring is
  sized by ``--weights-gib`` and the KV ring by ``--kv-gib``; it reports ``tokens_per_s`` and ``tbps`` (weight plus KV
  bytes read per second);
* ``--workload layer`` is a whole decoder layer per ring layer and step, again on the library's kernels only: the
  server workload's attention half between a residual stream and its normalisations, and the MLP, which holds two
  thirds of a layer's weights.  Per layer: ``gsx_add_rmsnorm`` (the residual add fused with the RMSNorm), the QKV
  projection, RoPE and KV append, the attention, the output projection, ``gsx_add_rmsnorm`` again, the fused gate / up
  projection to ``2 x --ffn`` columns, ``gsx_silu_mul`` and the down projection.  ``--ffn`` is the MLP's width (default
  3.5 x hidden, rounded to a multiple of 64).  Layer 0 of every step starts the residual stream afresh from a constant
  input, so an endless run stays finite.  The weights are bf16; it takes the server workload's other options and
  reports the same fields and ``ffn``;
* ``--workload generate`` closes the layer workload into generation, as a server runs it.  Per step:
  ``gsx_embed_gather`` of the previous step's token ids (the input of layer 0), the layers, a final ``gsx_add_rmsnorm``,
  the LM head, which is the bf16 decode GEMM with N = ``--vocab`` (default 128256), and ``gsx_sample`` with
  ``--temperature`` (0.8), ``--top-k`` (50), ``--top-p`` (0.95) and ``--seed`` into the other of two token buffers.  A
  step's token feeds the next step through device memory: nothing waits for the host, which passes only the step
  number.  ``--batch`` is 1..16.  It reports the layer workload's fields, ``vocab``, ``tokens_per_s``,
  ``bytes_per_step`` (LM head and embedding rows included), ``tbps`` from it, and ``tokens_in_range``: every id of the
  last step lies in ``[0, vocab)``;
* ``--workload prefill`` is the same decoder layer in the prefill phase, the compute-bound half of a server:
  ``--batch`` sequences (1..256) of ``--chunk`` new tokens each (default 2048; ``batch * chunk`` a multiple of 128),
  which land at positions ``[--context - chunk, --context)``: ``--context`` is the length after the chunk, and has
  to be given (the other workloads' default means something else).  The
  projections run on the large bf16 GEMM, ``gsx_kv_append`` writes the whole chunk and ``gsx_prefill_attn``, causal
  over the paged cache, attends over it.  The lengths are a constant device buffer, so an endless run rewrites the same
  slots.  It reports ``tokens_per_s`` (prompt tokens), ``tflops`` (the projections, and the attention over visible
  pairs only), ``tbps``, ``chunk`` and the layer workload's fields.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import os
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent


def parse_mask(s: str) -> list[int]:
    return [int(x, 16) for x in s.split(",") if x]


def kernels_lib_path() -> Path | None:
    """libgsx_kernels.so: $GSX_KERNELS_LIB, next to this file (the image), or the repository's build tree."""
    cands = [os.environ.get("GSX_KERNELS_LIB", ""), str(HERE / "libgsx_kernels.so"),
             str(HERE.parents[1] / "gpushare_scheduler_extender_amd" / "_native" / "libgsx_kernels.so")
             if len(HERE.parents) > 1 else ""]
    for c in cands:
        if c and Path(c).is_file():
            return Path(c)
    return None


DECODE_KINDS = {"bf16": 0, "fp8": 1, "mxfp4": 2}  # gsx_kernels.h: GSX_DECODE_*
GIB = 1 << 30


def matrix_bytes(dtype: str, n: int, k: int) -> int:
    """Bytes of one ``n`` x ``k`` weight matrix with its scales: what one decode launch streams."""
    if dtype == "mxfp4":
        return n * k // 2 + n * k // 32
    return n * k * (2 if dtype == "bf16" else 1)


def default_weights_bytes(allocated_gib: float) -> int:
    """The ring's size when ``--weights-gib`` is not given: 4 GiB, or a quarter of the pod's share if that is
    smaller (no share: 4 GiB)."""
    return min(4 * GIB, int(allocated_gib * GIB) // 4) if allocated_gib else 4 * GIB


ATTN_KV_KINDS = {"bf16": 0, "fp8": 1}  # gsx_kernels.h: GSX_ATTN_KV_*
ATTN_D = 128


def kv_layer_bytes(kv_dtype: str, batch: int, context: int, kv_heads: int) -> int:
    """Bytes of K and V one attention launch reads: ``batch`` sequences of ``context`` tokens, D = 128."""
    return 2 * batch * context * kv_heads * ATTN_D * (2 if kv_dtype == "bf16" else 1)


def kv_pages(batch: int, context: int, page: int) -> tuple[int, int]:
    """``(pages per sequence, pages of one layer's cache)``: every sequence owns whole pages."""
    per_seq = math.ceil(context / page)
    return per_seq, batch * per_seq


def default_kv_bytes(allocated_gib: float) -> int:
    """The KV ring's size when ``--kv-gib`` is not given: as :func:`default_weights_bytes`."""
    return default_weights_bytes(allocated_gib)


def kv_ring_layers(kv_bytes: int, one_layer_bytes: int) -> int:
    """Per-layer caches in the ring: enough to cover ``kv_bytes``, never fewer than two."""
    return ring_layers(kv_bytes, one_layer_bytes)


SERVER_WINDOW = 64


def server_layer_weight_bytes(heads: int, kv_heads: int) -> int:
    """Bytes of one decode layer's bf16 weights: the QKV projection ``[(heads + 2 kv_heads) * 128][hidden]`` and the
    output projection ``[hidden][hidden]``, hidden = ``heads * 128``."""
    hidden = heads * ATTN_D
    return ((heads + 2 * kv_heads) * ATTN_D * hidden + hidden * hidden) * 2


def server_window(context: int) -> int:
    """Steps after which the server workload's sequences start again: they grow from ``context - window`` to
    ``context`` tokens, inside the pages the block table has for ``context``."""
    return min(SERVER_WINDOW, context)


def default_ffn(hidden: int) -> int:
    """The MLP's width when ``--ffn`` is not given: 3.5 x ``hidden``, rounded to a multiple of 64."""
    return max(64, round(3.5 * hidden / 64) * 64)


def layer_weight_bytes(heads: int, kv_heads: int, ffn: int) -> int:
    """Bytes of one decoder layer's bf16 weights: the server layer's two projections, the fused gate / up projection
    ``[2 ffn][hidden]`` and the down projection ``[hidden][ffn]`` (the norm weights, 4 x hidden bytes, are not
    counted)."""
    return server_layer_weight_bytes(heads, kv_heads) + 3 * ffn * heads * ATTN_D * 2


MOE_MAX_EXPERTS = 1024
MOE_MAX_ACTIVE = 8
MOE_PLAN_INTS = 516  # GSX_MOE_PLAN_INTS


def moe_expert_bytes(heads: int, ffn: int) -> int:
    """Bytes of one expert's bf16 weights: its gate / up projection ``[2 ffn][hidden]`` and its down projection
    ``[hidden][ffn]``."""
    return 3 * ffn * heads * ATTN_D * 2


def moe_layer_weight_bytes(heads: int, kv_heads: int, ffn: int, experts: int) -> int:
    """Bytes of one MoE decoder layer's bf16 weights as they are resident: the server layer's two projections, the
    router ``[experts][hidden]`` and ``experts`` experts of width ``ffn``.  A step reads only the experts it hits
    (:func:`moe_layer_read_bytes`)."""
    return (server_layer_weight_bytes(heads, kv_heads) + experts * heads * ATTN_D * 2
            + experts * moe_expert_bytes(heads, ffn))


def moe_layer_read_bytes(heads: int, kv_heads: int, ffn: int, experts: int, hit: float) -> float:
    """Bytes of weights one MoE layer reads in a step that hits ``hit`` of its experts: the dense part and the router
    whole, and the hit experts."""
    return (server_layer_weight_bytes(heads, kv_heads) + experts * heads * ATTN_D * 2
            + hit * moe_expert_bytes(heads, ffn))


def moe_active(experts: int, experts_active: int) -> int:
    """The experts a token picks: ``--experts-active``, capped at ``--experts``."""
    return min(experts_active, experts)


def moe_refusal(workload: str, experts: int, experts_active: int) -> str | None:
    """Why ``--experts`` cannot run with these options, or None: known before anything touches the device."""
    if experts == 0:
        return None
    if workload == "prefill":
        return "--workload prefill --experts: more than 16 rows needs a grouped large GEMM, which there is none of"
    if workload not in ("layer", "generate"):
        return f"--experts {experts}: --workload layer and generate only"
    if not 16 <= experts <= MOE_MAX_EXPERTS or experts % 16:
        return f"--experts {experts}: 0, or a multiple of 16 in 16..{MOE_MAX_EXPERTS} (the router is the decode GEMM)"
    if not 1 <= experts_active <= MOE_MAX_ACTIVE:
        return f"--experts-active {experts_active}: 1..{MOE_MAX_ACTIVE}"
    return None


def prefill_refusal(batch: int, chunk: int, context: int) -> str | None:
    """Why ``--workload prefill`` cannot run these sizes, or None: known before anything touches the device."""
    if chunk < 1:
        return f"--chunk {chunk}: at least 1"
    if not 1 <= batch <= 256:
        return f"--batch {batch}: 1..256 sequences"
    if (batch * chunk) % 128:
        return f"--batch {batch} x --chunk {chunk} = {batch * chunk} rows: the GEMM takes a multiple of 128"
    if chunk > context:
        return f"--chunk {chunk} is more than --context {context}: the context is the length after the chunk"
    return None


def prefill_visible_pairs(batch: int, chunk: int, context: int) -> int:
    """(query row, token) pairs a causal chunk at positions ``[context - chunk, context)`` sees, the row's own token
    included: the sum over rows of ``pos + 1``."""
    return batch * (chunk * (context - chunk) + chunk * (chunk + 1) // 2)


def ring_layers(weights_bytes: int, one_matrix_bytes: int) -> int:
    """Matrices in the weight ring: enough to cover ``weights_bytes``, and never fewer than two, so that no launch
    finds its matrix where the last launch left it."""
    return max(2, math.ceil(weights_bytes / one_matrix_bytes))


class Kernels:
    """The slice of libgsx_kernels.so (native/kernels/gsx_kernels.hip) the workload uses."""

    def __init__(self, path: Path):
        L = ctypes.CDLL(str(path))
        vp, u32p, i32 = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_int
        for name, args in {"gsx_stream_create": [i32, u32p, i32, ctypes.POINTER(vp)], "gsx_stream_destroy": [vp],
                           "gsx_stream_sync": [vp], "gsx_gemm_bf16_nt": [vp, vp, vp, vp, i32, i32, i32]}.items():
            f = getattr(L, name)
            f.argtypes, f.restype = args, i32
        if hasattr(L, "gsx_gemm_fp8_nt"):  # an image built before the fp8 kernels has none; --dtype fp8 says so
            L.gsx_gemm_fp8_nt.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp, i32]
            L.gsx_gemm_fp8_nt.restype = i32
        if hasattr(L, "gsx_gemm_mxfp4_nt"):  # likewise: an image built before the mxfp4 kernels
            L.gsx_gemm_mxfp4_nt.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp]
            L.gsx_quant_mxfp4.argtypes = [vp, vp, vp, vp, i32, i32]
            L.gsx_gemm_mxfp4_nt.restype = L.gsx_quant_mxfp4.restype = i32
        if hasattr(L, "gsx_decode_gemm_nt"):  # likewise: an image built before the decode kernels
            L.gsx_decode_gemm_nt.argtypes = [vp, i32, vp, vp, vp, i32, i32, i32, vp, vp, i32]
            L.gsx_decode_gemm_nt.restype = i32
        if hasattr(L, "gsx_decode_attn"):  # likewise: an image built before the attention kernel
            L.gsx_decode_attn.argtypes = ([vp, i32] + [vp] * 6 + [i32] * 8 + [ctypes.c_float] * 3
                                          + [vp, ctypes.c_uint64])
            L.gsx_decode_attn_workspace_bytes.argtypes = [i32] * 5 + [ctypes.POINTER(ctypes.c_uint64)]
            L.gsx_decode_attn.restype = L.gsx_decode_attn_workspace_bytes.restype = i32
        if hasattr(L, "gsx_kv_append"):  # likewise: an image built before the append kernel
            L.gsx_kv_append.argtypes = ([vp, i32, vp, ctypes.c_int64] + [vp] * 8 + [i32] * 10
                                        + [ctypes.c_float] * 2)
            L.gsx_kv_append.restype = i32
        if hasattr(L, "gsx_prefill_attn"):  # likewise: an image built before the prefill attention
            L.gsx_prefill_attn.argtypes = [vp, i32] + [vp] * 6 + [i32] * 9 + [ctypes.c_float] * 3
            L.gsx_prefill_attn.restype = i32
        if hasattr(L, "gsx_add_rmsnorm"):  # likewise: an image built before the norm and activation kernels
            i64 = ctypes.c_int64
            L.gsx_add_rmsnorm.argtypes = [vp, i32, vp, i64, vp, vp, i64, vp, vp, i64, vp, i32, i32, ctypes.c_float]
            L.gsx_silu_mul.argtypes = [vp, i32, vp, i64, vp, i64, vp, i32, i32]
            L.gsx_add_rmsnorm.restype = L.gsx_silu_mul.restype = i32
        if hasattr(L, "gsx_sample"):  # likewise: an image built before the sampler and the embedding gather
            i64, u64, fp = ctypes.c_int64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_float)
            L.gsx_sample.argtypes = [vp, vp, i64, vp, vp, vp, vp, u64, vp, i32, i32]
            L.gsx_embed_gather.argtypes = [vp, vp, i64, vp, vp, i64, i32, i32, i32]
            L.gsx_event_time_sample.argtypes = [*L.gsx_sample.argtypes, i32, fp]
            L.gsx_event_time_embed_gather.argtypes = [*L.gsx_embed_gather.argtypes, i32, fp]
            L.gsx_sample.restype = L.gsx_embed_gather.restype = i32
            L.gsx_event_time_sample.restype = L.gsx_event_time_embed_gather.restype = i32
        if hasattr(L, "gsx_moe_route"):  # likewise: an image built before the MoE kernels
            i64, fp, ip = ctypes.c_int64, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(i32)
            L.gsx_moe_route.argtypes = [vp, vp, i64, vp, vp, vp, i32, i32, i32]
            L.gsx_moe_gemm_nt.argtypes = [vp, i32, vp, i32, vp, vp, vp] + [i32] * 5 + [vp, vp, i32]
            L.gsx_moe_gemm_nt_launch_cfg.argtypes = [*L.gsx_moe_gemm_nt.argtypes, i32]
            L.gsx_moe_combine.argtypes = [vp, vp, i64, vp, vp, i64, i32, i32, i32]
            L.gsx_moe_gemm_cfg_name.argtypes, L.gsx_moe_gemm_cfg_name.restype = [i32], ctypes.c_char_p
            L.gsx_moe_gemm_cfg_shape.argtypes = [i32, ip, ip, ip, ip]
            L.gsx_event_time_moe_route.argtypes = [*L.gsx_moe_route.argtypes, i32, fp]
            L.gsx_event_time_moe_gemm.argtypes = [*L.gsx_moe_gemm_nt.argtypes, i32, fp]
            L.gsx_event_time_moe_combine.argtypes = [*L.gsx_moe_combine.argtypes, i32, fp]
            for f in (L.gsx_moe_route, L.gsx_moe_gemm_nt, L.gsx_moe_gemm_nt_launch_cfg, L.gsx_moe_combine,
                      L.gsx_moe_gemm_cfg_shape, L.gsx_event_time_moe_route, L.gsx_event_time_moe_gemm,
                      L.gsx_event_time_moe_combine):
                f.restype = i32
        L.gsx_last_error.argtypes, L.gsx_last_error.restype = [], ctypes.c_char_p
        self.L, self.path = L, path

    def _ck(self, rc: int, what: str):
        if rc != 0:
            raise RuntimeError(f"{what}: {(self.L.gsx_last_error() or b'').decode()}")

    def stream(self, dev: int, cu_mask: list[int] | None = None) -> ctypes.c_void_p:
        h = ctypes.c_void_p()
        arr = (ctypes.c_uint32 * len(cu_mask))(*cu_mask) if cu_mask else None
        self._ck(self.L.gsx_stream_create(dev, arr, len(cu_mask or []), ctypes.byref(h)), "stream_create")
        return h

    def gemm(self, s, a: int, b: int, c: int, m: int, n: int, k: int):
        self._ck(self.L.gsx_gemm_bf16_nt(s, ctypes.c_void_p(a), ctypes.c_void_p(b), ctypes.c_void_p(c), m, n, k),
                 "gemm_bf16_nt")

    def gemm_fp8(self, s, a: int, b: int, c: int, m: int, n: int, k: int):
        """e4m3 operands, no scales (scale_mode 0)."""
        if not hasattr(self.L, "gsx_gemm_fp8_nt"):
            raise RuntimeError(f"{self.path} has no gsx_gemm_fp8_nt: rebuild it")
        self._ck(self.L.gsx_gemm_fp8_nt(s, ctypes.c_void_p(a), ctypes.c_void_p(b), ctypes.c_void_p(c), m, n, k,
                                        None, None, 0), "gemm_fp8_nt")

    def has_mxfp4(self) -> bool:
        return hasattr(self.L, "gsx_gemm_mxfp4_nt")

    def quant_mxfp4(self, s, x: int, q: int, sc: int, rows: int, k: int):
        """bf16 ``x[rows][k]`` -> e2m1 pairs ``q[rows][k / 2]`` and e8m0 block scales ``sc[rows][k / 32]``."""
        if not self.has_mxfp4():
            raise RuntimeError(f"{self.path} has no gsx_quant_mxfp4: rebuild it")
        self._ck(self.L.gsx_quant_mxfp4(s, ctypes.c_void_p(x), ctypes.c_void_p(q), ctypes.c_void_p(sc), rows, k),
                 "quant_mxfp4")

    def gemm_mxfp4(self, s, a: int, b: int, c: int, m: int, n: int, k: int, sa: int, sb: int):
        if not self.has_mxfp4():
            raise RuntimeError(f"{self.path} has no gsx_gemm_mxfp4_nt: rebuild it")
        self._ck(self.L.gsx_gemm_mxfp4_nt(s, ctypes.c_void_p(a), ctypes.c_void_p(b), ctypes.c_void_p(c), m, n, k,
                                          ctypes.c_void_p(sa), ctypes.c_void_p(sb)), "gemm_mxfp4_nt")

    def decode_gemm(self, s, dtype: str, a: int, b: int, c: int, m: int, n: int, k: int, sa: int = 0, sb: int = 0):
        """``c[m][n] = a[m][k] * b[n][k]^T`` for m <= 16; mxfp4 takes the e8m0 block scales, the others none."""
        if not hasattr(self.L, "gsx_decode_gemm_nt"):
            raise RuntimeError(f"{self.path} has no gsx_decode_gemm_nt: rebuild it")
        self._ck(self.L.gsx_decode_gemm_nt(s, DECODE_KINDS[dtype], ctypes.c_void_p(a), ctypes.c_void_p(b),
                                           ctypes.c_void_p(c), m, n, k, ctypes.c_void_p(sa), ctypes.c_void_p(sb), 0),
                 "decode_gemm_nt")

    def attn_workspace_bytes(self, b: int, hq: int, page: int, max_seq_len: int) -> int:
        if not hasattr(self.L, "gsx_decode_attn"):
            raise RuntimeError(f"{self.path} has no gsx_decode_attn: rebuild it")
        n = ctypes.c_uint64(0)
        self._ck(self.L.gsx_decode_attn_workspace_bytes(b, hq, ATTN_D, page, max_seq_len, ctypes.byref(n)),
                 "decode_attn_workspace_bytes")
        return n.value

    def decode_attn(self, s, kv_dtype: str, q: int, kc: int, vc: int, table: int, lens: int, o: int, b: int, hq: int,
                    hkv: int, page: int, num_pages: int, table_stride: int, max_seq_len: int, scale: float, ws: int,
                    ws_bytes: int):
        """One decode step of attention over a paged KV cache (unit cache scales)."""
        self._ck(self.L.gsx_decode_attn(s, ATTN_KV_KINDS[kv_dtype], *(ctypes.c_void_p(x) for x in
                                                                      (q, kc, vc, table, lens, o)),
                                        b, hq, hkv, ATTN_D, page, num_pages, table_stride, max_seq_len, scale, 1.0, 1.0,
                                        ctypes.c_void_p(ws), ws_bytes), "decode_attn")

    def kv_append(self, s, kv_dtype: str, qkv: int, qkv_stride: int, q_out: int, kc: int, vc: int, table: int,
                  lens: int, lens_out: int, cos: int, sin: int, rope_len: int, b: int, t: int, hq: int, hkv: int,
                  page: int, num_pages: int, table_stride: int, max_seq_len: int):
        """RoPE on Q and K and the new tokens' K and V into their page slots (unit cache scales)."""
        if not hasattr(self.L, "gsx_kv_append"):
            raise RuntimeError(f"{self.path} has no gsx_kv_append: rebuild it")
        self._ck(self.L.gsx_kv_append(s, ATTN_KV_KINDS[kv_dtype], ctypes.c_void_p(qkv), qkv_stride,
                                      *(ctypes.c_void_p(x) for x in (q_out, kc, vc, table, lens, lens_out, cos, sin)),
                                      rope_len, b, t, hq, hkv, ATTN_D, page, num_pages, table_stride, max_seq_len,
                                      1.0, 1.0), "kv_append")

    def prefill_attn(self, s, kv_dtype: str, q: int, kc: int, vc: int, table: int, lens: int, o: int, b: int, t: int,
                     hq: int, hkv: int, page: int, num_pages: int, table_stride: int, max_seq_len: int, scale: float):
        """Causal attention of ``t`` new tokens per sequence over the paged cache (unit cache scales); ``lens`` are the
        lengths before the chunk."""
        if not hasattr(self.L, "gsx_prefill_attn"):
            raise RuntimeError(f"{self.path} has no gsx_prefill_attn: rebuild it")
        self._ck(self.L.gsx_prefill_attn(s, ATTN_KV_KINDS[kv_dtype], *(ctypes.c_void_p(x) for x in
                                                                       (q, kc, vc, table, lens, o)),
                                         b, t, hq, hkv, ATTN_D, page, num_pages, table_stride, max_seq_len, scale, 1.0,
                                         1.0), "prefill_attn")

    def add_rmsnorm(self, s, x: int, r_in: int, r_out: int, w: int, y: int, m: int, h: int, eps: float):
        """``hid = bf16(x + r_in)`` (``x`` with ``r_in`` 0) to ``r_out``, and its RMSNorm times ``w`` to ``y``: bf16,
        contiguous rows."""
        if not hasattr(self.L, "gsx_add_rmsnorm"):
            raise RuntimeError(f"{self.path} has no gsx_add_rmsnorm: rebuild it")
        self._ck(self.L.gsx_add_rmsnorm(s, 0, ctypes.c_void_p(x), h, ctypes.c_void_p(r_in), ctypes.c_void_p(r_out), h,
                                        ctypes.c_void_p(w), ctypes.c_void_p(y), h, None, m, h, eps), "add_rmsnorm")

    def silu_mul(self, s, gu: int, y: int, m: int, i: int):
        """``y[m][i] = silu(gu[:, :i]) * gu[:, i:]``: bf16, contiguous rows."""
        self._ck(self.L.gsx_silu_mul(s, 0, ctypes.c_void_p(gu), 2 * i, ctypes.c_void_p(y), i, None, m, i), "silu_mul")

    def _sample_args(self, s, logits: int, temperature: int, top_k: int, top_p: int, seeds: int, counter: int,
                     tokens_out: int, m: int, v: int) -> tuple:
        if not hasattr(self.L, "gsx_sample"):
            raise RuntimeError(f"{self.path} has no gsx_sample: rebuild it")
        return (s, ctypes.c_void_p(logits), v, *(ctypes.c_void_p(x) for x in (temperature, top_k, top_p, seeds)),
                counter & 0xFFFFFFFFFFFFFFFF, ctypes.c_void_p(tokens_out), m, v)

    def sample(self, s, logits: int, temperature: int, top_k: int, top_p: int, seeds: int, counter: int,
               tokens_out: int, m: int, v: int):
        """One int32 token id per row of ``logits[m][v]`` (bf16, contiguous rows); the per-row parameter arrays are
        device addresses (0: NULL), ``counter`` is the step number."""
        self._ck(self.L.gsx_sample(*self._sample_args(s, logits, temperature, top_k, top_p, seeds, counter, tokens_out,
                                                      m, v)), "sample")

    def time_sample(self, s, logits: int, temperature: int, top_k: int, top_p: int, seeds: int, counter: int,
                    tokens_out: int, m: int, v: int, iters: int) -> float:
        ms = ctypes.c_float(0)
        self._ck(self.L.gsx_event_time_sample(*self._sample_args(s, logits, temperature, top_k, top_p, seeds, counter,
                                                                 tokens_out, m, v), iters, ctypes.byref(ms)),
                 "time_sample")
        return ms.value

    def _embed_args(self, s, table: int, tokens: int, out: int, m: int, h: int, v: int) -> tuple:
        if not hasattr(self.L, "gsx_embed_gather"):
            raise RuntimeError(f"{self.path} has no gsx_embed_gather: rebuild it")
        return (s, ctypes.c_void_p(table), h, ctypes.c_void_p(tokens), ctypes.c_void_p(out), h, m, h, v)

    def embed_gather(self, s, table: int, tokens: int, out: int, m: int, h: int, v: int):
        """``out[m][h]`` = rows ``tokens[m]`` (int32, device memory) of ``table[v][h]``: bf16, contiguous rows."""
        self._ck(self.L.gsx_embed_gather(*self._embed_args(s, table, tokens, out, m, h, v)), "embed_gather")

    def time_embed_gather(self, s, table: int, tokens: int, out: int, m: int, h: int, v: int, iters: int) -> float:
        ms = ctypes.c_float(0)
        self._ck(self.L.gsx_event_time_embed_gather(*self._embed_args(s, table, tokens, out, m, h, v), iters,
                                                    ctypes.byref(ms)), "time_embed_gather")
        return ms.value

    def _moe_route_args(self, s, logits: int, ids: int, w: int, plan: int, m: int, e: int, topk: int) -> tuple:
        if not hasattr(self.L, "gsx_moe_route"):
            raise RuntimeError(f"{self.path} has no gsx_moe_route: rebuild it")
        return (s, ctypes.c_void_p(logits), e, *(ctypes.c_void_p(x) for x in (ids, w, plan)), m, e, topk)

    def moe_route(self, s, logits: int, ids: int, w: int, plan: int, m: int, e: int, topk: int):
        """From ``logits[m][e]`` (bf16, contiguous rows): ``ids[m][topk]`` int32, ``w[m][topk]`` fp32 and the plan of
        ``MOE_PLAN_INTS`` int32 that groups the pairs by expert, all in device memory."""
        self._ck(self.L.gsx_moe_route(*self._moe_route_args(s, logits, ids, w, plan, m, e, topk)), "moe_route")

    def time_moe_route(self, s, logits: int, ids: int, w: int, plan: int, m: int, e: int, topk: int,
                       iters: int) -> float:
        ms = ctypes.c_float(0)
        self._ck(self.L.gsx_event_time_moe_route(*self._moe_route_args(s, logits, ids, w, plan, m, e, topk), iters,
                                                 ctypes.byref(ms)), "time_moe_route")
        return ms.value

    def _moe_gemm_args(self, s, dtype: str, a: int, a_div: int, b: int, c: int, plan: int, m: int, topk: int, e: int,
                       n: int, k: int, sa: int, sb: int, mode: int) -> tuple:
        if not hasattr(self.L, "gsx_moe_gemm_nt"):
            raise RuntimeError(f"{self.path} has no gsx_moe_gemm_nt: rebuild it")
        return (s, DECODE_KINDS[dtype], ctypes.c_void_p(a), a_div, ctypes.c_void_p(b), ctypes.c_void_p(c),
                ctypes.c_void_p(plan), m, topk, e, n, k, ctypes.c_void_p(sa), ctypes.c_void_p(sb), mode)

    def moe_gemm_nt(self, s, dtype: str, a: int, a_div: int, b: int, c: int, plan: int, m: int, topk: int, e: int,
                    n: int, k: int, sa: int = 0, sb: int = 0, mode: int = 0):
        """``c[p][n] = a[p // a_div][k] * b[expert of p][n][k]^T`` for every pair ``p`` of the plan."""
        self._ck(self.L.gsx_moe_gemm_nt(*self._moe_gemm_args(s, dtype, a, a_div, b, c, plan, m, topk, e, n, k, sa, sb,
                                                             mode)), "moe_gemm_nt")

    def moe_gemm_cfgs(self) -> dict[int, tuple[str, int, int, int, int]]:
        """``{index: (name, bn, waves, inflight, decode_cfg)}`` of the grouped GEMM's table."""
        out: dict[int, tuple[str, int, int, int, int]] = {}
        while (name := self.L.gsx_moe_gemm_cfg_name(len(out))) is not None:
            v = [ctypes.c_int(0) for _ in range(4)]
            self._ck(self.L.gsx_moe_gemm_cfg_shape(len(out), *map(ctypes.byref, v)), "moe_gemm_cfg_shape")
            out[len(out)] = (name.decode(), *(x.value for x in v))
        return out

    def moe_gemm_nt_cfg(self, s, dtype: str, a: int, a_div: int, b: int, c: int, plan: int, m: int, topk: int, e: int,
                        n: int, k: int, cfg: int, sa: int = 0, sb: int = 0, mode: int = 0):
        self._ck(self.L.gsx_moe_gemm_nt_launch_cfg(*self._moe_gemm_args(s, dtype, a, a_div, b, c, plan, m, topk, e, n,
                                                                        k, sa, sb, mode), cfg), f"moe gemm cfg {cfg}")

    def time_moe_gemm(self, s, dtype: str, a: int, a_div: int, b: int, c: int, plan: int, m: int, topk: int, e: int,
                      n: int, k: int, iters: int, sa: int = 0, sb: int = 0, mode: int = 0) -> float:
        ms = ctypes.c_float(0)
        self._ck(self.L.gsx_event_time_moe_gemm(*self._moe_gemm_args(s, dtype, a, a_div, b, c, plan, m, topk, e, n, k,
                                                                     sa, sb, mode), iters, ctypes.byref(ms)),
                 "time_moe_gemm")
        return ms.value

    def _moe_combine_args(self, s, y: int, w: int, out: int, m: int, topk: int, h: int) -> tuple:
        if not hasattr(self.L, "gsx_moe_combine"):
            raise RuntimeError(f"{self.path} has no gsx_moe_combine: rebuild it")
        return (s, ctypes.c_void_p(y), h, ctypes.c_void_p(w), ctypes.c_void_p(out), h, m, topk, h)

    def moe_combine(self, s, y: int, w: int, out: int, m: int, topk: int, h: int):
        """``out[m][h]`` = the sum over ``j`` of ``w[m][j] * y[m topk + j][h]``: bf16, contiguous rows."""
        self._ck(self.L.gsx_moe_combine(*self._moe_combine_args(s, y, w, out, m, topk, h)), "moe_combine")

    def time_moe_combine(self, s, y: int, w: int, out: int, m: int, topk: int, h: int, iters: int) -> float:
        ms = ctypes.c_float(0)
        self._ck(self.L.gsx_event_time_moe_combine(*self._moe_combine_args(s, y, w, out, m, topk, h), iters,
                                                   ctypes.byref(ms)), "time_moe_combine")
        return ms.value

    def sync(self, s):
        self._ck(self.L.gsx_stream_sync(s), "stream_sync")

    def destroy(self, s):
        self.L.gsx_stream_destroy(s)


def decode_steps(torch, kl, gs, stream, dev, dtype: str, a, c, layers: int):
    """``(step, sync)`` of the decode workload: the ring of ``layers`` weight matrices ``[n][k]`` (random normal, made
    one at a time so that nothing larger than one matrix is ever held in bf16), and a step that multiplies the ``m``
    activation rows ``a`` by each of them in turn into ``c``.  ``kl`` and ``gs`` are the library and its stream, or
    None for torch's own GEMMs (on ``stream`` if there is one)."""
    m, k = a.shape
    n = c.shape[1]
    wdt = {"bf16": torch.bfloat16, "fp8": torch.float8_e4m3fn, "mxfp4": torch.uint8}[dtype]
    w = torch.empty(layers, n, k // 2 if dtype == "mxfp4" else k, device=dev, dtype=wdt)
    if dtype == "mxfp4":  # the library's quantiser makes weights and activations; it takes any row count
        ws = torch.empty(layers, n, k // 32, device=dev, dtype=torch.uint8)
        qa = torch.empty(m, k // 2, device=dev, dtype=torch.uint8)
        sa = torch.empty(m, k // 32, device=dev, dtype=torch.uint8)
        torch.cuda.synchronize()
        kl.quant_mxfp4(gs, a.data_ptr(), qa.data_ptr(), sa.data_ptr(), m, k)
    for i in range(layers):
        x = torch.randn(n, k, device=dev, dtype=torch.bfloat16)
        if dtype == "mxfp4":
            torch.cuda.synchronize()
            kl.quant_mxfp4(gs, x.data_ptr(), w[i].data_ptr(), ws[i].data_ptr(), n, k)
            kl.sync(gs)
        else:
            w[i].copy_(x.to(wdt))
        del x
    if kl is not None:
        w_bytes = w[0].numel() * w.element_size()
        if dtype == "mxfp4":
            a_ptr, sa_ptr, s_bytes = qa.data_ptr(), sa.data_ptr(), ws[0].numel()
        else:
            a_ptr, sa_ptr, s_bytes, ws = a.data_ptr(), 0, 0, None

        def step():
            for i in range(layers):
                kl.decode_gemm(gs, dtype, a_ptr, w.data_ptr() + i * w_bytes, c.data_ptr(), m, n, k, sa_ptr,
                               ws.data_ptr() + i * s_bytes if ws is not None else 0)

        def sync():
            kl.sync(gs)

        step.keep = (w, ws, a)  # the closures hold addresses, not tensors
        return step, sync
    one = torch.ones((), device=dev, dtype=torch.float32)

    def matmul(i):
        if dtype == "fp8":  # hipBLASLt's fp8 GEMM, unit per-tensor scales
            torch._scaled_mm(a, w[i].t(), scale_a=one, scale_b=one, out_dtype=torch.bfloat16, out=c)
        else:
            torch.matmul(a, w[i].t(), out=c)

    try:  # torch may refuse so skinny a shape: its message is the answer then
        matmul(0)
    except RuntimeError as e:
        raise SystemExit(f"--kernel torch --workload decode --dtype {dtype} --batch {m}: {e}") from None

    def step():
        if stream is not None:
            with torch.cuda.stream(stream):
                for i in range(layers):
                    matmul(i)
        else:
            for i in range(layers):
                matmul(i)

    def sync():
        (stream or torch.cuda.current_stream()).synchronize()

    return step, sync


def attn_steps(torch, kl, gs, stream, dev, kv_dtype: str, batch: int, context: int, heads: int, kv_heads: int,
               page: int, layers: int):
    """``(step, sync)`` of the attention workload: a ring of ``layers`` paged KV caches (random normal), one block
    table (a random permutation of a layer's pages: every layer has the same map and its own memory), and a step that
    runs one attention per layer.  ``kl`` and ``gs`` are the library and its stream, or None for torch's SDPA on a
    contiguous bf16 copy (on ``stream`` if there is one)."""
    per_seq, pages = kv_pages(batch, context, page)
    q = torch.randn(batch, heads, ATTN_D, device=dev, dtype=torch.bfloat16)
    o = torch.empty_like(q)
    scale = 1.0 / math.sqrt(ATTN_D)
    if kl is None:
        kc = torch.randn(layers, batch, kv_heads, context, ATTN_D, device=dev, dtype=torch.bfloat16)
        vc = torch.randn(layers, batch, kv_heads, context, ATTN_D, device=dev, dtype=torch.bfloat16)
        q4 = q.unsqueeze(2)  # [B][Hq][1][D]
        sdpa = torch.nn.functional.scaled_dot_product_attention

        def attend():
            for i in range(layers):
                o.copy_(sdpa(q4, kc[i], vc[i], scale=scale, enable_gqa=True).squeeze(2))

        def step():
            if stream is not None:
                with torch.cuda.stream(stream):
                    attend()
            else:
                attend()

        def sync():
            (stream or torch.cuda.current_stream()).synchronize()

        return step, sync
    kdt = torch.bfloat16 if kv_dtype == "bf16" else torch.float8_e4m3fn
    kc = torch.empty(layers, pages, kv_heads, page, ATTN_D, device=dev, dtype=kdt)
    vc = torch.empty_like(kc)
    for i in range(layers):  # one layer at a time: nothing larger is ever held in bf16
        for c in (kc, vc):
            c[i].copy_(torch.randn(pages, kv_heads, page, ATTN_D, device=dev, dtype=torch.bfloat16).to(kdt))
    table = torch.randperm(pages, device=dev).to(torch.int32).view(batch, per_seq).contiguous()
    lens = torch.full((batch,), context, device=dev, dtype=torch.int32)
    ws_bytes = kl.attn_workspace_bytes(batch, heads, page, context)
    ws = torch.empty(max(ws_bytes, 16), device=dev, dtype=torch.uint8)
    layer_bytes = kc[0].numel() * kc.element_size()
    torch.cuda.synchronize()

    def step():
        for i in range(layers):
            kl.decode_attn(gs, kv_dtype, q.data_ptr(), kc.data_ptr() + i * layer_bytes,
                           vc.data_ptr() + i * layer_bytes, table.data_ptr(), lens.data_ptr(), o.data_ptr(), batch,
                           heads, kv_heads, page, pages, per_seq, context, scale, ws.data_ptr(), ws_bytes)

    def sync():
        kl.sync(gs)

    step.keep = (q, o, kc, vc, table, lens, ws)  # the closures hold addresses, not tensors
    return step, sync


def server_steps(torch, kl, gs, dev, kv_dtype: str, batch: int, context: int, heads: int, kv_heads: int, page: int,
                 w_layers: int, kv_layers: int):
    """``(step, sync, finite)`` of the server workload: a ring of ``w_layers`` decode layers' bf16 weights (random
    normal over sqrt(hidden), so activations keep their size), a ring of ``kv_layers`` paged KV caches behind one block
    table, and a step that runs ``max(w_layers, kv_layers)`` decode layers back to back on the library's stream: QKV
    projection, RoPE and append, attention, output projection.  Layer 0 always reads the same activations.  The
    lengths ping-pong between two device buffers through ``lens_out``; every :func:`server_window` steps the constant
    start buffer is the input again.  ``finite()`` says whether the last activations are finite."""
    hidden, nqkv = heads * ATTN_D, (heads + 2 * kv_heads) * ATTN_D
    per_seq, pages = kv_pages(batch, context, page)
    window = server_window(context)
    layers = max(w_layers, kv_layers)
    wqkv = torch.empty(w_layers, nqkv, hidden, device=dev, dtype=torch.bfloat16)
    wo = torch.empty(w_layers, hidden, hidden, device=dev, dtype=torch.bfloat16)
    for i in range(w_layers):  # one matrix at a time: nothing larger is ever held in fp32
        wqkv[i].copy_(torch.randn(nqkv, hidden, device=dev) / math.sqrt(hidden))
        wo[i].copy_(torch.randn(hidden, hidden, device=dev) / math.sqrt(hidden))
    kdt = torch.bfloat16 if kv_dtype == "bf16" else torch.float8_e4m3fn
    kc = torch.empty(kv_layers, pages, kv_heads, page, ATTN_D, device=dev, dtype=kdt)
    vc = torch.empty_like(kc)
    for i in range(kv_layers):
        for c in (kc, vc):
            c[i].copy_(torch.randn(pages, kv_heads, page, ATTN_D, device=dev, dtype=torch.bfloat16).to(kdt))
    table = torch.randperm(pages, device=dev).to(torch.int32).view(batch, per_seq).contiguous()
    start = torch.full((batch,), context - window, device=dev, dtype=torch.int32)
    lens = [torch.zeros(batch, device=dev, dtype=torch.int32) for _ in range(2)]
    ang = (torch.arange(context, device=dev, dtype=torch.float64)[:, None]
           * 10000.0 ** (-torch.arange(ATTN_D // 2, device=dev, dtype=torch.float64) / (ATTN_D // 2))[None])
    cos, sin = ang.cos().float().contiguous(), ang.sin().float().contiguous()
    x = [torch.randn(batch, hidden, device=dev, dtype=torch.bfloat16) for _ in range(3)]  # x[0]: layer 0's, constant
    qkv = torch.empty(batch, nqkv, device=dev, dtype=torch.bfloat16)
    q = torch.empty(batch, heads, ATTN_D, device=dev, dtype=torch.bfloat16)
    o = torch.empty_like(q)
    ws_bytes = kl.attn_workspace_bytes(batch, heads, page, context)
    ws = torch.empty(max(ws_bytes, 16), device=dev, dtype=torch.uint8)
    wqkv_bytes, wo_bytes = wqkv[0].numel() * 2, wo[0].numel() * 2
    cache_bytes = kc[0].numel() * kc.element_size()
    scale = 1.0 / math.sqrt(ATTN_D)
    torch.cuda.synchronize()
    count = [0]

    def step():
        k = count[0] % window
        count[0] += 1
        lens_in = start if k == 0 else lens[(k - 1) % 2]
        lens_out = lens[k % 2]
        for i in range(layers):
            xin = x[0] if i == 0 else x[1 + i % 2]
            xout = x[1 + (i + 1) % 2]
            kci, vci = kc.data_ptr() + (i % kv_layers) * cache_bytes, vc.data_ptr() + (i % kv_layers) * cache_bytes
            kl.decode_gemm(gs, "bf16", xin.data_ptr(), wqkv.data_ptr() + (i % w_layers) * wqkv_bytes, qkv.data_ptr(),
                           batch, nqkv, hidden)
            kl.kv_append(gs, kv_dtype, qkv.data_ptr(), nqkv, q.data_ptr(), kci, vci, table.data_ptr(),
                         lens_in.data_ptr(), lens_out.data_ptr(), cos.data_ptr(), sin.data_ptr(), context, batch, 1,
                         heads, kv_heads, page, pages, per_seq, context)
            kl.decode_attn(gs, kv_dtype, q.data_ptr(), kci, vci, table.data_ptr(), lens_out.data_ptr(), o.data_ptr(),
                           batch, heads, kv_heads, page, pages, per_seq, context, scale, ws.data_ptr(), ws_bytes)
            kl.decode_gemm(gs, "bf16", o.data_ptr(), wo.data_ptr() + (i % w_layers) * wo_bytes, xout.data_ptr(), batch,
                           hidden, hidden)

    def sync():
        kl.sync(gs)

    def finite():
        kl.sync(gs)
        return all(bool(torch.isfinite(t.float()).all()) for t in (*x, qkv, q, o))

    step.keep = (wqkv, wo, kc, vc, table, start, lens, cos, sin, x, qkv, q, o, ws)  # the closures hold addresses
    step.buffers = {"wqkv": wqkv, "wo": wo, "kc": kc, "vc": vc, "table": table, "start": start, "lens0": lens[0],
                    "lens1": lens[1], "cos": cos, "sin": sin, "x0": x[0], "x1": x[1], "x2": x[2], "qkv": qkv, "q": q,
                    "o": o, "ws": ws}  # every tensor the step addresses, by name: what a test resolves a launch against
    return step, sync, finite


LAYER_EPS = 1e-5


def layer_steps(torch, kl, gs, dev, kv_dtype: str, batch: int, context: int, heads: int, kv_heads: int, page: int,
                ffn: int, w_layers: int, kv_layers: int, experts: int = 0, active: int = 0):
    """``(step, sync, finite)`` of the layer workload: :func:`server_steps` with a residual stream, the two
    normalisations and the MLP.  A ring of ``w_layers`` decoder layers' bf16 weights (random normal over the square
    root of the input width; norm weights of 1), a ring of ``kv_layers`` paged KV caches, and a step that runs
    ``max(w_layers, kv_layers)`` layers back to back on the library's stream.  Layer 0 takes the constant input with
    no residual and writes the residual buffer; every later add updates it in place.

    With ``experts`` > 0 the MLP is a mixture of experts of width ``ffn``, of which a token picks ``active``: the
    router (the decode GEMM with N = ``experts``), ``moe_route``, the grouped up projection, SwiGLU on the
    ``batch * active`` pairs, the grouped down projection and ``moe_combine``, with ids, weights and plan in device
    memory and one plan buffer per layer of the step.  ``step.hits()`` synchronises and returns every layer's
    ``n_active`` of the last step."""
    hidden, nqkv = heads * ATTN_D, (heads + 2 * kv_heads) * ATTN_D
    per_seq, pages = kv_pages(batch, context, page)
    window = server_window(context)
    layers = max(w_layers, kv_layers)
    bf = torch.bfloat16
    wqkv = torch.empty(w_layers, nqkv, hidden, device=dev, dtype=bf)
    wo = torch.empty(w_layers, hidden, hidden, device=dev, dtype=bf)
    nexp, pairs = max(experts, 1), batch * max(active, 1)  # a dense MLP is one expert that every row takes once
    wgu = torch.empty(w_layers, nexp * 2 * ffn, hidden, device=dev, dtype=bf)
    wdown = torch.empty(w_layers, nexp * hidden, ffn, device=dev, dtype=bf)
    router = torch.empty(w_layers, experts, hidden, device=dev, dtype=bf)
    for i in range(w_layers):  # one matrix at a time: nothing larger is ever held in fp32
        for w, k in ((wqkv, hidden), (wo, hidden), (router, hidden)):
            w[i].copy_(torch.randn(w.shape[1], k, device=dev) / math.sqrt(k))
        for w, rows, k in ((wgu, 2 * ffn, hidden), (wdown, hidden, ffn)):
            for e in range(nexp):
                w[i, e * rows:(e + 1) * rows].copy_(torch.randn(rows, k, device=dev) / math.sqrt(k))
    ln = torch.ones(w_layers, 2, hidden, device=dev, dtype=bf)
    kdt = bf if kv_dtype == "bf16" else torch.float8_e4m3fn
    kc = torch.empty(kv_layers, pages, kv_heads, page, ATTN_D, device=dev, dtype=kdt)
    vc = torch.empty_like(kc)
    for i in range(kv_layers):
        for c in (kc, vc):
            c[i].copy_(torch.randn(pages, kv_heads, page, ATTN_D, device=dev, dtype=bf).to(kdt))
    table = torch.randperm(pages, device=dev).to(torch.int32).view(batch, per_seq).contiguous()
    start = torch.full((batch,), context - window, device=dev, dtype=torch.int32)
    lens = [torch.zeros(batch, device=dev, dtype=torch.int32) for _ in range(2)]
    ang = (torch.arange(context, device=dev, dtype=torch.float64)[:, None]
           * 10000.0 ** (-torch.arange(ATTN_D // 2, device=dev, dtype=torch.float64) / (ATTN_D // 2))[None])
    cos, sin = ang.cos().float().contiguous(), ang.sin().float().contiguous()
    x0 = torch.randn(batch, hidden, device=dev, dtype=bf)  # layer 0's input, constant
    resid, xn, sub = (torch.zeros(batch, hidden, device=dev, dtype=bf) for _ in range(3))
    qkv = torch.empty(batch, nqkv, device=dev, dtype=bf)
    q = torch.empty(batch, heads, ATTN_D, device=dev, dtype=bf)
    o = torch.empty_like(q)
    gu = torch.empty(pairs, 2 * ffn, device=dev, dtype=bf)
    act = torch.empty(pairs, ffn, device=dev, dtype=bf)
    rlogits = torch.empty(batch, experts, device=dev, dtype=bf)
    ids = torch.empty(pairs, device=dev, dtype=torch.int32)
    tw = torch.empty(pairs, device=dev, dtype=torch.float32)
    yexp = torch.empty(pairs, hidden, device=dev, dtype=bf)
    plans = torch.zeros(layers if experts else 0, MOE_PLAN_INTS, device=dev, dtype=torch.int32)
    ws_bytes = kl.attn_workspace_bytes(batch, heads, page, context)
    ws = torch.empty(max(ws_bytes, 16), device=dev, dtype=torch.uint8)
    wqkv_b, wo_b, wgu_b, wdown_b, router_b = (w[0].numel() * 2 for w in (wqkv, wo, wgu, wdown, router))
    cache_bytes = kc[0].numel() * kc.element_size()
    scale = 1.0 / math.sqrt(ATTN_D)
    torch.cuda.synchronize()
    count = [0]

    def step():
        k = count[0] % window
        count[0] += 1
        lens_in = start if k == 0 else lens[(k - 1) % 2]
        lens_out = lens[k % 2]
        for i in range(layers):
            wi = i % w_layers
            kci, vci = kc.data_ptr() + (i % kv_layers) * cache_bytes, vc.data_ptr() + (i % kv_layers) * cache_bytes
            ln1 = ln.data_ptr() + wi * 2 * hidden * 2
            if i == 0:  # the residual stream starts afresh
                kl.add_rmsnorm(gs, x0.data_ptr(), 0, resid.data_ptr(), ln1, xn.data_ptr(), batch, hidden, LAYER_EPS)
            else:
                kl.add_rmsnorm(gs, sub.data_ptr(), resid.data_ptr(), resid.data_ptr(), ln1, xn.data_ptr(), batch,
                               hidden, LAYER_EPS)
            kl.decode_gemm(gs, "bf16", xn.data_ptr(), wqkv.data_ptr() + wi * wqkv_b, qkv.data_ptr(), batch, nqkv,
                           hidden)
            kl.kv_append(gs, kv_dtype, qkv.data_ptr(), nqkv, q.data_ptr(), kci, vci, table.data_ptr(),
                         lens_in.data_ptr(), lens_out.data_ptr(), cos.data_ptr(), sin.data_ptr(), context, batch, 1,
                         heads, kv_heads, page, pages, per_seq, context)
            kl.decode_attn(gs, kv_dtype, q.data_ptr(), kci, vci, table.data_ptr(), lens_out.data_ptr(), o.data_ptr(),
                           batch, heads, kv_heads, page, pages, per_seq, context, scale, ws.data_ptr(), ws_bytes)
            kl.decode_gemm(gs, "bf16", o.data_ptr(), wo.data_ptr() + wi * wo_b, sub.data_ptr(), batch, hidden, hidden)
            kl.add_rmsnorm(gs, sub.data_ptr(), resid.data_ptr(), resid.data_ptr(), ln1 + hidden * 2, xn.data_ptr(),
                           batch, hidden, LAYER_EPS)
            if not experts:
                kl.decode_gemm(gs, "bf16", xn.data_ptr(), wgu.data_ptr() + wi * wgu_b, gu.data_ptr(), batch, 2 * ffn,
                               hidden)
                kl.silu_mul(gs, gu.data_ptr(), act.data_ptr(), batch, ffn)
                kl.decode_gemm(gs, "bf16", act.data_ptr(), wdown.data_ptr() + wi * wdown_b, sub.data_ptr(), batch,
                               hidden, ffn)
                continue
            plan = plans.data_ptr() + i * MOE_PLAN_INTS * 4
            kl.decode_gemm(gs, "bf16", xn.data_ptr(), router.data_ptr() + wi * router_b, rlogits.data_ptr(), batch,
                           experts, hidden)
            kl.moe_route(gs, rlogits.data_ptr(), ids.data_ptr(), tw.data_ptr(), plan, batch, experts, active)
            kl.moe_gemm_nt(gs, "bf16", xn.data_ptr(), active, wgu.data_ptr() + wi * wgu_b, gu.data_ptr(), plan, batch,
                           active, experts, 2 * ffn, hidden)
            kl.silu_mul(gs, gu.data_ptr(), act.data_ptr(), pairs, ffn)
            kl.moe_gemm_nt(gs, "bf16", act.data_ptr(), 1, wdown.data_ptr() + wi * wdown_b, yexp.data_ptr(), plan,
                           batch, active, experts, hidden, ffn)
            kl.moe_combine(gs, yexp.data_ptr(), tw.data_ptr(), sub.data_ptr(), batch, active, hidden)

    def sync():
        kl.sync(gs)

    def finite():
        kl.sync(gs)
        moe = (rlogits, tw, yexp) if experts else ()
        return all(bool(torch.isfinite(t.float()).all()) for t in (resid, xn, sub, qkv, q, o, gu, act, *moe))

    def hits():
        kl.sync(gs)
        return plans[:, 0].tolist()

    step.hits = hits
    # the closures hold addresses, not tensors
    step.keep = (wqkv, wo, wgu, wdown, router, ln, kc, vc, table, start, lens, cos, sin, x0, resid, xn, sub, qkv, q, o,
                 gu, act, ws, rlogits, ids, tw, yexp, plans)
    step.io = {"x0": x0, "resid": resid, "sub": sub, "xn": xn}  # what the generate workload puts around the layers
    step.buffers = {"wqkv": wqkv, "wo": wo, "wgu": wgu, "wdown": wdown, "router": router, "ln": ln, "kc": kc, "vc": vc,
                    "table": table, "start": start, "lens0": lens[0], "lens1": lens[1], "cos": cos, "sin": sin,
                    "x0": x0, "resid": resid, "xn": xn, "sub": sub, "qkv": qkv, "q": q, "o": o, "gu": gu, "act": act,
                    "ws": ws, "rlogits": rlogits, "ids": ids, "tw": tw, "yexp": yexp, "plans": plans}  # as server_steps'
    return step, sync, finite


GENERATE_MAX_VOCAB = 262144


def generate_refusal(batch: int, vocab: int) -> str | None:
    """Why ``--workload generate`` cannot run these sizes, or None: known before anything touches the device."""
    if not 1 <= batch <= 16:
        return f"--batch {batch}: 1..16 rows (the LM head is the decode GEMM)"
    if not 16 <= vocab <= GENERATE_MAX_VOCAB or vocab % 16:
        return f"--vocab {vocab}: a multiple of 16 in 16..{GENERATE_MAX_VOCAB}"
    return None


def generate_step_bytes(layers: int, one_layer_bytes: int, kv_bytes: int, batch: int, hidden: int, vocab: int) -> int:
    """Bytes one generation step reads: the layers' weights and KV, the LM head ``[vocab][hidden]`` and the ``batch``
    embedding rows (bf16)."""
    return layers * (one_layer_bytes + kv_bytes) + vocab * hidden * 2 + batch * hidden * 2


def generate_steps(torch, kl, gs, dev, kv_dtype: str, batch: int, context: int, heads: int, kv_heads: int, page: int,
                   ffn: int, w_layers: int, kv_layers: int, vocab: int, temperature: float, top_k: int, top_p: float,
                   seed: int, experts: int = 0, active: int = 0):
    """``(step, sync, finite, tokens)`` of the generate workload: a step of :func:`layer_steps` between the embedding
    lookup of the previous step's tokens and the final norm, the LM head (the decode GEMM with N = ``vocab``) and the
    sampler, which writes the other of two token buffers.  The tokens go from step to step through device memory;
    the host passes only the step number.  ``tokens()`` synchronises and returns the last step's token ids."""
    hidden = heads * ATTN_D
    bf = torch.bfloat16
    layers, sync, layers_finite = layer_steps(torch, kl, gs, dev, kv_dtype, batch, context, heads, kv_heads, page, ffn,
                                              w_layers, kv_layers, experts, active)
    io = layers.io
    embed = torch.randn(vocab, hidden, device=dev, dtype=bf)
    head = torch.empty(vocab, hidden, device=dev, dtype=bf)
    for lo in range(0, vocab, 16384):  # in slices: nothing large is ever held in fp32
        head[lo:lo + 16384].copy_(torch.randn(min(16384, vocab - lo), hidden, device=dev) / math.sqrt(hidden))
    lnf = torch.ones(hidden, device=dev, dtype=bf)
    logits = torch.empty(batch, vocab, device=dev, dtype=bf)
    tokens = [torch.randint(0, vocab, (batch,), device=dev, dtype=torch.int32) for _ in range(2)]
    temp = torch.full((batch,), temperature, device=dev, dtype=torch.float32)
    topk = torch.full((batch,), top_k, device=dev, dtype=torch.int32)
    topp = torch.full((batch,), top_p, device=dev, dtype=torch.float32)
    seeds = (torch.arange(batch, device=dev, dtype=torch.int64) + (seed & 0x7FFFFFFFFFFFFFFF)).contiguous()
    torch.cuda.synchronize()
    count = [0]

    def step():
        n = count[0]
        count[0] += 1
        kl.embed_gather(gs, embed.data_ptr(), tokens[n % 2].data_ptr(), io["x0"].data_ptr(), batch, hidden, vocab)
        layers()
        kl.add_rmsnorm(gs, io["sub"].data_ptr(), io["resid"].data_ptr(), 0, lnf.data_ptr(), io["xn"].data_ptr(), batch,
                       hidden, LAYER_EPS)
        kl.decode_gemm(gs, "bf16", io["xn"].data_ptr(), head.data_ptr(), logits.data_ptr(), batch, vocab, hidden)
        kl.sample(gs, logits.data_ptr(), temp.data_ptr(), topk.data_ptr(), topp.data_ptr(), seeds.data_ptr(), n,
                  tokens[(n + 1) % 2].data_ptr(), batch, vocab)

    def finite():
        return layers_finite() and bool(torch.isfinite(logits.float()).all())

    def last_tokens():
        kl.sync(gs)
        return tokens[count[0] % 2].tolist()

    step.hits = layers.hits
    step.keep = (layers, embed, head, lnf, logits, tokens, temp, topk, topp, seeds)
    step.buffers = {**layers.buffers, "embed": embed, "head": head, "lnf": lnf, "logits": logits, "tokens0": tokens[0],
                    "tokens1": tokens[1], "temp": temp, "topk": topk, "topp": topp, "seeds": seeds}
    return step, sync, finite, last_tokens


def prefill_steps(torch, kl, gs, dev, kv_dtype: str, batch: int, chunk: int, context: int, heads: int, kv_heads: int,
                  page: int, ffn: int, w_layers: int, kv_layers: int):
    """``(step, sync, finite)`` of the prefill workload: :func:`layer_steps` on ``batch * chunk`` rows.  The
    projections go through the large GEMM, the append writes ``chunk`` tokens per sequence at positions
    ``[context - chunk, context)`` and the causal attention reads the lengths the append read: one constant buffer."""
    hidden, nqkv = heads * ATTN_D, (heads + 2 * kv_heads) * ATTN_D
    rows = batch * chunk
    per_seq, pages = kv_pages(batch, context, page)
    layers = max(w_layers, kv_layers)
    bf = torch.bfloat16
    wqkv = torch.empty(w_layers, nqkv, hidden, device=dev, dtype=bf)
    wo = torch.empty(w_layers, hidden, hidden, device=dev, dtype=bf)
    wgu = torch.empty(w_layers, 2 * ffn, hidden, device=dev, dtype=bf)
    wdown = torch.empty(w_layers, hidden, ffn, device=dev, dtype=bf)
    for i in range(w_layers):  # one matrix at a time: nothing larger is ever held in fp32
        for w, k in ((wqkv, hidden), (wo, hidden), (wgu, hidden), (wdown, ffn)):
            w[i].copy_(torch.randn(w.shape[1], k, device=dev) / math.sqrt(k))
    ln = torch.ones(w_layers, 2, hidden, device=dev, dtype=bf)
    kdt = bf if kv_dtype == "bf16" else torch.float8_e4m3fn
    kc = torch.empty(kv_layers, pages, kv_heads, page, ATTN_D, device=dev, dtype=kdt)
    vc = torch.empty_like(kc)
    for i in range(kv_layers):
        for c in (kc, vc):
            c[i].copy_(torch.randn(pages, kv_heads, page, ATTN_D, device=dev, dtype=bf).to(kdt))
    table = torch.randperm(pages, device=dev).to(torch.int32).view(batch, per_seq).contiguous()
    lens = torch.full((batch,), context - chunk, device=dev, dtype=torch.int32)  # before the chunk; never written
    ang = (torch.arange(context, device=dev, dtype=torch.float64)[:, None]
           * 10000.0 ** (-torch.arange(ATTN_D // 2, device=dev, dtype=torch.float64) / (ATTN_D // 2))[None])
    cos, sin = ang.cos().float().contiguous(), ang.sin().float().contiguous()
    x0 = torch.randn(rows, hidden, device=dev, dtype=bf)  # layer 0's input, constant
    resid, xn, sub = (torch.zeros(rows, hidden, device=dev, dtype=bf) for _ in range(3))
    qkv = torch.empty(rows, nqkv, device=dev, dtype=bf)
    q = torch.empty(rows, heads, ATTN_D, device=dev, dtype=bf)
    o = torch.empty_like(q)
    gu = torch.empty(rows, 2 * ffn, device=dev, dtype=bf)
    act = torch.empty(rows, ffn, device=dev, dtype=bf)
    wqkv_b, wo_b, wgu_b, wdown_b = (w[0].numel() * 2 for w in (wqkv, wo, wgu, wdown))
    cache_bytes = kc[0].numel() * kc.element_size()
    scale = 1.0 / math.sqrt(ATTN_D)
    torch.cuda.synchronize()

    def step():
        for i in range(layers):
            wi = i % w_layers
            kci, vci = kc.data_ptr() + (i % kv_layers) * cache_bytes, vc.data_ptr() + (i % kv_layers) * cache_bytes
            ln1 = ln.data_ptr() + wi * 2 * hidden * 2
            if i == 0:  # the residual stream starts afresh
                kl.add_rmsnorm(gs, x0.data_ptr(), 0, resid.data_ptr(), ln1, xn.data_ptr(), rows, hidden, LAYER_EPS)
            else:
                kl.add_rmsnorm(gs, sub.data_ptr(), resid.data_ptr(), resid.data_ptr(), ln1, xn.data_ptr(), rows,
                               hidden, LAYER_EPS)
            kl.gemm(gs, xn.data_ptr(), wqkv.data_ptr() + wi * wqkv_b, qkv.data_ptr(), rows, nqkv, hidden)
            kl.kv_append(gs, kv_dtype, qkv.data_ptr(), nqkv, q.data_ptr(), kci, vci, table.data_ptr(),
                         lens.data_ptr(), 0, cos.data_ptr(), sin.data_ptr(), context, batch, chunk, heads, kv_heads,
                         page, pages, per_seq, context)
            kl.prefill_attn(gs, kv_dtype, q.data_ptr(), kci, vci, table.data_ptr(), lens.data_ptr(), o.data_ptr(),
                            batch, chunk, heads, kv_heads, page, pages, per_seq, context, scale)
            kl.gemm(gs, o.data_ptr(), wo.data_ptr() + wi * wo_b, sub.data_ptr(), rows, hidden, hidden)
            kl.add_rmsnorm(gs, sub.data_ptr(), resid.data_ptr(), resid.data_ptr(), ln1 + hidden * 2, xn.data_ptr(),
                           rows, hidden, LAYER_EPS)
            kl.gemm(gs, xn.data_ptr(), wgu.data_ptr() + wi * wgu_b, gu.data_ptr(), rows, 2 * ffn, hidden)
            kl.silu_mul(gs, gu.data_ptr(), act.data_ptr(), rows, ffn)
            kl.gemm(gs, act.data_ptr(), wdown.data_ptr() + wi * wdown_b, sub.data_ptr(), rows, hidden, ffn)

    def sync():
        kl.sync(gs)

    def finite():
        kl.sync(gs)
        return all(bool(torch.isfinite(t.float()).all()) for t in (resid, xn, sub, qkv, q, o, gu, act))

    # the closures hold addresses, not tensors
    step.keep = (wqkv, wo, wgu, wdown, ln, kc, vc, table, lens, cos, sin, x0, resid, xn, sub, qkv, q, o, gu, act)
    step.buffers = {"wqkv": wqkv, "wo": wo, "wgu": wgu, "wdown": wdown, "ln": ln, "kc": kc, "vc": vc, "table": table,
                    "lens": lens, "cos": cos, "sin": sin, "x0": x0, "resid": resid, "xn": xn, "sub": sub, "qkv": qkv,
                    "q": q, "o": o, "gu": gu, "act": act}  # as server_steps'
    return step, sync, finite


def run(total: float, allocated: float, *, kernel: str = "auto", size: int = 8192, seconds: float = 0.0,
        iters: int = 0, report_every: float = 5.0, touch: bool = False, quiet: bool = False,
        probe_limit: bool = False, dtype: str = "bf16", workload: str = "gemm", batch: int = 8,
        weights_gib: float | None = None, context: int = 8192, heads: int = 64, kv_heads: int = 8,
        kv_dtype: str = "bf16", kv_gib: float | None = None, page: int = 16, ffn: int | None = None,
        chunk: int = 2048, vocab: int = 128256, temperature: float = 0.8, top_k: int = 50, top_p: float = 0.95,
        seed: int = 0, experts: int = 0, experts_active: int = MOE_MAX_ACTIVE) -> dict:
    if why := moe_refusal(workload, experts, experts_active):
        raise SystemExit(why)
    if workload == "prefill" and (why := prefill_refusal(batch, chunk, context)):
        raise SystemExit(f"--workload prefill: {why}")
    if workload == "generate" and (why := generate_refusal(batch, vocab)):
        raise SystemExit(f"--workload generate: {why}")
    import torch

    lib_path = kernels_lib_path()
    if kernel == "auto":
        kernel = "gsx" if lib_path is not None else "torch"
        if lib_path is None and not quiet:
            print("[workload] libgsx_kernels.so not found: torch.matmul (hipBLASLt) instead", flush=True)
    kl = None
    if kernel == "gsx" or os.environ.get("GSX_CU_MASK"):
        if lib_path is None:
            if kernel == "gsx":
                raise SystemExit("--kernel gsx: libgsx_kernels.so not found (GSX_KERNELS_LIB, next to main.py)")
        else:
            kl = Kernels(lib_path)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    frac = 1.0 if not total else max(0.0, min(1.0, allocated / total))
    torch.cuda.set_per_process_memory_fraction(frac, dev)
    stream = None
    hip_stream = None
    if os.environ.get("GSX_CU_MASK") and kl is not None:
        hip_stream = kl.stream(0, parse_mask(os.environ["GSX_CU_MASK"]))
        stream = torch.cuda.ExternalStream(hip_stream.value, device=dev)
    hold = None
    if touch:
        # claim (most of) the share so co-resident pods really contend for HBM
        hold = torch.empty(int(allocated * (1 << 30) * 0.9) // 2, dtype=torch.bfloat16, device=dev)
        hold.fill_(1)
    m = n = k = size
    if dtype not in ("bf16", "fp8", "mxfp4"):
        raise SystemExit(f"--dtype {dtype}: bf16, fp8 or mxfp4")
    if workload not in ("gemm", "decode", "attn", "server", "layer", "prefill", "generate"):
        raise SystemExit(f"--workload {workload}: gemm, decode, attn, server, layer, prefill or generate")
    decode = workload == "decode"
    prefill = workload == "prefill"
    generate = workload == "generate"
    layer = workload == "layer" or generate  # the generate workload is the layer workload between tokens
    server = workload == "server" or layer  # the layer workload is the server workload with more in a layer
    attn = workload == "attn" or server or prefill  # these have the attention's shape options
    if server or prefill:
        if kernel != "gsx":
            raise SystemExit(f"--workload {workload} runs on the library's kernels only (--kernel gsx)")
        if dtype != "bf16":
            raise SystemExit(f"--workload {workload}: the weights are bf16 only (the KV cache: --kv-dtype)")
        if server and not 1 <= batch <= 16:
            raise SystemExit(f"--batch {batch}: 1..16")
    if layer or prefill:
        ffn = default_ffn(heads * ATTN_D) if ffn is None else ffn
        if ffn < 64 or ffn % 64:
            raise SystemExit(f"--ffn {ffn}: a multiple of 64, at least 64")
    if attn:
        if not 1 <= batch <= 256:
            raise SystemExit(f"--batch {batch}: 1..256 sequences")
        if kv_dtype not in ATTN_KV_KINDS:
            raise SystemExit(f"--kv-dtype {kv_dtype}: bf16 or fp8")
        if kernel != "gsx" and kv_dtype != "bf16":
            raise SystemExit("--kernel torch --workload attn runs scaled_dot_product_attention on bf16 only")
        if context < 1 or heads < 1 or kv_heads < 1 or heads % kv_heads or heads // kv_heads > 16:
            raise SystemExit("--workload attn: --context >= 1, --heads a multiple of --kv-heads, at most 16 times it")
        if page % 16 or not 16 <= page <= 256:
            raise SystemExit(f"--page {page}: a multiple of 16 in 16..256")
        m, n, k = batch, heads, ATTN_D  # nothing of the GEMM's operands is needed: keep them tiny
    if decode:
        if not 1 <= batch <= 16:
            raise SystemExit(f"--batch {batch}: 1..16")
        m = batch
    if dtype == "mxfp4" and kernel != "gsx":
        raise SystemExit("--dtype mxfp4 needs the library's kernels (--kernel gsx): "
                         + ("torch has no such GEMM" if kl is not None else "libgsx_kernels.so was not found"))
    a = torch.randn(m, k, device=dev, dtype=torch.bfloat16)
    if not decode:
        b = torch.randn(n, k, device=dev, dtype=torch.bfloat16)
    c = torch.empty(m, n, device=dev, dtype=torch.bfloat16)
    if dtype == "fp8":  # OCP e4m3, the MI355X's format; the output stays bf16
        a = a.to(torch.float8_e4m3fn)
        if not decode:
            b = b.to(torch.float8_e4m3fn)
        one = torch.ones((), device=dev, dtype=torch.float32)
    own = None
    if kernel == "gsx":
        gs = hip_stream if hip_stream is not None else kl.stream(0)
        own = None if hip_stream is not None else gs
    layers = 1
    finite = None
    if prefill:
        weights_bytes = default_weights_bytes(allocated) if weights_gib is None else int(weights_gib * GIB)
        one_layer_bytes = layer_weight_bytes(heads, kv_heads, ffn)
        w_layers = ring_layers(weights_bytes, one_layer_bytes)
        kv_layers = kv_ring_layers(default_kv_bytes(allocated) if kv_gib is None else int(kv_gib * GIB),
                                   kv_layer_bytes(kv_dtype, batch, context, kv_heads))
        layers = max(w_layers, kv_layers)
        step, sync, finite = prefill_steps(torch, kl, gs, dev, kv_dtype, batch, chunk, context, heads, kv_heads, page,
                                           ffn, w_layers, kv_layers)
        # the projections (2 flops per weight and row: a weight is 2 bytes), and QK^T and PV over the visible pairs
        flops_attn = layers * (batch * chunk * one_layer_bytes
                               + 4.0 * ATTN_D * heads * prefill_visible_pairs(batch, chunk, context))
    elif server:
        weights_bytes = default_weights_bytes(allocated) if weights_gib is None else int(weights_gib * GIB)
        active = moe_active(experts, experts_active)
        one_layer_bytes = (moe_layer_weight_bytes(heads, kv_heads, ffn, experts) if experts
                           else layer_weight_bytes(heads, kv_heads, ffn) if layer
                           else server_layer_weight_bytes(heads, kv_heads))
        w_layers = ring_layers(weights_bytes, one_layer_bytes)
        kv_layers = kv_ring_layers(default_kv_bytes(allocated) if kv_gib is None else int(kv_gib * GIB),
                                   kv_layer_bytes(kv_dtype, batch, context, kv_heads))
        layers = max(w_layers, kv_layers)
        if generate:
            step, sync, finite, last_tokens = generate_steps(torch, kl, gs, dev, kv_dtype, batch, context, heads,
                                                             kv_heads, page, ffn, w_layers, kv_layers, vocab,
                                                             temperature, top_k, top_p, seed, experts, active)
        elif layer:
            step, sync, finite = layer_steps(torch, kl, gs, dev, kv_dtype, batch, context, heads, kv_heads, page, ffn,
                                             w_layers, kv_layers, experts, active)
        else:
            step, sync, finite = server_steps(torch, kl, gs, dev, kv_dtype, batch, context, heads, kv_heads, page,
                                              w_layers, kv_layers)
        # the projections (2 flops per weight and row: a weight is 2 bytes), and QK^T and PV over the context
        flops_attn = layers * (batch * one_layer_bytes + 4.0 * batch * heads * context * ATTN_D)
        if experts:  # a row meets the dense part, the router and its `active` experts
            flops_attn = layers * (batch * moe_layer_read_bytes(heads, kv_heads, ffn, experts, active)
                                   + 4.0 * batch * heads * context * ATTN_D)
        if generate:  # the LM head
            flops_attn += 2.0 * batch * vocab * heads * ATTN_D
    elif attn:
        layer_bytes = kv_layer_bytes(kv_dtype, batch, context, kv_heads)
        layers = kv_ring_layers(default_kv_bytes(allocated) if kv_gib is None else int(kv_gib * GIB), layer_bytes)
        step, sync = attn_steps(torch, kl if kernel == "gsx" else None, gs if kernel == "gsx" else None, stream, dev,
                                kv_dtype, batch, context, heads, kv_heads, page, layers)
        # QK^T and PV: 2 * 2 * D flops per (sequence, query head, token)
        flops_attn = 4.0 * batch * heads * context * ATTN_D * layers
    elif decode:
        weights_bytes = default_weights_bytes(allocated) if weights_gib is None else int(weights_gib * GIB)
        layers = ring_layers(weights_bytes, matrix_bytes(dtype, n, k))
        step, sync = decode_steps(torch, kl if kernel == "gsx" else None, gs if kernel == "gsx" else None, stream, dev,
                                  dtype, a, c, layers)
    elif kernel == "gsx":
        gemm = kl.gemm_fp8 if dtype == "fp8" else kl.gemm
        if dtype == "mxfp4":  # quantise the random bf16 operands once; the loop runs on the result
            qa, qb = (torch.empty(r, k // 2, device=dev, dtype=torch.uint8) for r in (m, n))
            sa, sb = (torch.empty(r, k // 32, device=dev, dtype=torch.uint8) for r in (m, n))
            torch.cuda.synchronize()
            kl.quant_mxfp4(gs, a.data_ptr(), qa.data_ptr(), sa.data_ptr(), m, k)
            kl.quant_mxfp4(gs, b.data_ptr(), qb.data_ptr(), sb.data_ptr(), n, k)
            kl.sync(gs)
            a, b = qa, qb

            def gemm(s, pa, pb, pc, m, n, k):
                kl.gemm_mxfp4(s, pa, pb, pc, m, n, k, sa.data_ptr(), sb.data_ptr())

        def step():
            gemm(gs, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k)

        def sync():
            kl.sync(gs)
    else:
        def matmul():
            if dtype == "fp8":  # hipBLASLt's fp8 GEMM, unit per-tensor scales
                torch._scaled_mm(a, b.t(), scale_a=one, scale_b=one, out_dtype=torch.bfloat16, out=c)
            else:
                torch.matmul(a, b.t(), out=c)

        def step():
            if stream is not None:
                with torch.cuda.stream(stream):
                    matmul()
            else:
                matmul()

        def sync():
            (stream or torch.cuda.current_stream()).synchronize()
    torch.cuda.synchronize()
    for _ in range(3):
        step()
    sync()
    start_at = float(os.environ.get("GSX_START_AT", "0") or 0)
    if start_at:  # co-resident pods start their timed loops together (isolation bench)
        time.sleep(max(0.0, start_at - time.time()))
    flops = 2.0 * m * n * k * layers  # of one step: decode launches once per matrix of the ring
    if attn:
        flops = flops_attn
    done = 0
    t0 = last = time.perf_counter()
    last_done = 0
    while True:
        for _ in range(10):
            step()
        done += 10
        sync()
        now = time.perf_counter()
        if now - last >= report_every:
            r = (done - last_done) * flops / (now - last) / 1e12
            if not quiet:
                print(f"[workload] {r:.1f} TFLOP/s  share={allocated}/{total} GiB frac={frac:.3f}", flush=True)
            last, last_done = now, done
        if (seconds and now - t0 >= seconds) or (iters and done >= iters):
            break
    el = time.perf_counter() - t0
    out = {"tflops": done * flops / el / 1e12, "iters": done, "seconds": el, "fraction": frac,
           "cu_mask": os.environ.get("GSX_CU_MASK", ""), "kernel": kernel, "dtype": dtype, "size": size,
           "kernels_lib": str(kl.path) if kl is not None else "",
           "visible_devices": os.environ.get("HIP_VISIBLE_DEVICES", ""),
           "device_total_bytes": torch.cuda.get_device_properties(dev).total_memory}
    if decode:
        out.update({"workload": workload, "batch": m, "layers": layers,
                    "tbps": done * layers * matrix_bytes(dtype, n, k) / el / 1e12})
    if prefill:
        step_bytes = layers * (one_layer_bytes + kv_layer_bytes(kv_dtype, batch, context, kv_heads))
        out.update({"workload": workload, "batch": batch, "chunk": chunk, "layers": layers, "weight_layers": w_layers,
                    "kv_layers": kv_layers, "context": context, "heads": heads, "kv_heads": kv_heads,
                    "kv_dtype": kv_dtype, "page": page, "ffn": ffn, "tbps": done * step_bytes / el / 1e12,
                    "tokens_per_s": done * batch * chunk / el, "activations_finite": finite()})
    elif server:
        step_bytes = layers * (one_layer_bytes + kv_layer_bytes(kv_dtype, batch, context, kv_heads))
        out.update({"workload": workload, "batch": batch, "layers": layers, "weight_layers": w_layers,
                    "kv_layers": kv_layers, "context": context, "heads": heads, "kv_heads": kv_heads,
                    "kv_dtype": kv_dtype, "page": page, "window": server_window(context),
                    "tbps": done * step_bytes / el / 1e12, "tokens_per_s": done * batch / el,
                    "activations_finite": finite()})
        if layer:
            out["ffn"] = ffn
        if experts:
            # what a step reads depends on its routing: the weights are counted for the experts the last step hit
            hits = step.hits()
            read_bytes = sum(moe_layer_read_bytes(heads, kv_heads, ffn, experts, h) for h in hits) / len(hits)
            step_bytes = layers * (read_bytes + kv_layer_bytes(kv_dtype, batch, context, kv_heads))
            out.update({"experts": experts, "experts_active": active, "experts_hit_mean": sum(hits) / len(hits),
                        "tbps": done * step_bytes / el / 1e12,
                        "tbps_basis": "the experts hit by the last step's routing, taken for every step"})
        if generate:
            one_read = read_bytes if experts else one_layer_bytes
            step_bytes = generate_step_bytes(layers, one_read, kv_layer_bytes(kv_dtype, batch, context, kv_heads),
                                             batch, heads * ATTN_D, vocab)
            out.update({"vocab": vocab, "temperature": temperature, "top_k": top_k, "top_p": top_p, "seed": seed,
                        "bytes_per_step": step_bytes, "tbps": done * step_bytes / el / 1e12,
                        "tokens_in_range": all(0 <= t < vocab for t in last_tokens())})
    elif attn:
        out.update({"workload": workload, "batch": batch, "layers": layers, "context": context, "heads": heads,
                    "kv_heads": kv_heads, "kv_dtype": kv_dtype, "page": page,
                    "tbps": done * layers * kv_layer_bytes(kv_dtype, batch, context, kv_heads) / el / 1e12,
                    "tokens_per_s": done * batch / el})
    if probe_limit and allocated:
        # the share is a ceiling: one more share-sized tensor must be refused by the caching allocator
        try:
            extra = torch.empty(int(allocated * (1 << 30)) // 2, dtype=torch.bfloat16, device=dev)
            del extra
            out["limit_enforced"] = False
        except torch.cuda.OutOfMemoryError:
            out["limit_enforced"] = True
    del hold
    for s in (hip_stream, own):
        if s is not None:
            kl.destroy(s)
    return out


class _Parser(argparse.ArgumentParser):
    """``--batch`` has a range per workload: 1..16 rows (gemm ignores it, decode uses it), 1..256 sequences for attn
    and prefill, also where only an ``attn-*`` scenario of the isolation harness (its ``--scenarios``) runs an
    attention pod.  The sizes ``--workload prefill`` cannot run are refused here too, before anything loads torch."""

    def parse_args(self, args=None, namespace=None):
        ns = super().parse_args(args, namespace)
        scenarios = getattr(ns, "scenarios", "").split(",")
        wide = ns.workload in ("attn", "prefill") or any(sc.startswith("attn-") for sc in scenarios)
        top = 256 if wide else 16
        if not 1 <= ns.batch <= top:
            self.error(f"argument --batch: {ns.batch} is not in 1..{top} (--workload {ns.workload})")
        if ns.workload == "generate" and (why := generate_refusal(ns.batch, ns.vocab)):
            self.error(f"--workload generate: {why}")
        if why := moe_refusal(ns.workload, getattr(ns, "experts", 0), getattr(ns, "experts_active", MOE_MAX_ACTIVE)):
            self.error(why)
        if ns.workload == "prefill":
            # --context means something else here, the length AFTER the chunk, and the chunk's place follows from it:
            # the other workloads' default is not taken over silently
            given = sys.argv[1:] if args is None else args
            if not any(len(a.split("=")[0]) >= 5 and "--context".startswith(a.split("=")[0]) for a in given):
                self.error("--workload prefill: give --context, the length after the chunk (the chunk lands at "
                           "[context - chunk, context))")
            if why := prefill_refusal(ns.batch, ns.chunk, ns.context):
                self.error(f"--workload prefill: {why}")
        return ns


def add_attn_arguments(ap: argparse.ArgumentParser) -> None:
    """The options of ``--workload attn`` (shared with the isolation harness)."""
    ap.add_argument("--context", type=int, default=8192, help="--workload attn: tokens of every sequence")
    ap.add_argument("--heads", type=int, default=64, help="--workload attn: query heads")
    ap.add_argument("--kv-heads", type=int, default=8, help="--workload attn: KV heads (groups of heads / kv-heads)")
    ap.add_argument("--kv-dtype", default="bf16", choices=["bf16", "fp8"],
                    help="--workload attn: type of the KV cache (fp8: OCP e4m3; --kernel gsx only)")
    ap.add_argument("--kv-gib", type=float, default=None,
                    help="--workload attn: size of the ring of per-layer KV caches (default 4, or a quarter of the "
                         "share if that is smaller; never fewer than two layers)")
    ap.add_argument("--page", type=int, default=16,
                    help="--workload attn: tokens of a KV page (a multiple of 16 in 16..256)")
    ap.add_argument("--chunk", type=int, default=2048,
                    help="--workload prefill: new tokens per sequence, at most --context (which this workload wants "
                         "given: the length after the chunk); batch x chunk a multiple of 128")


def add_generate_arguments(ap: argparse.ArgumentParser) -> None:
    """The options of ``--workload generate`` (shared with the isolation harness)."""
    ap.add_argument("--vocab", type=int, default=128256,
                    help="--workload generate: the vocabulary, a multiple of 16 up to 262144")
    ap.add_argument("--temperature", type=float, default=0.8,
                    help="--workload generate: the sampling temperature of every row (<= 0: greedy)")
    ap.add_argument("--top-k", type=int, default=50, help="--workload generate: top-k of every row (<= 0: no limit)")
    ap.add_argument("--top-p", type=float, default=0.95, help="--workload generate: top-p of every row (>= 1: no cut)")
    ap.add_argument("--seed", type=int, default=0, help="--workload generate: row r draws with seed + r")


def add_moe_arguments(ap: argparse.ArgumentParser) -> None:
    """The options of the MoE form of ``--workload layer`` and ``generate`` (shared with the isolation harness)."""
    ap.add_argument("--experts", type=int, default=0,
                    help="--workload layer and generate: experts of the MLP, each --ffn wide (0: a dense MLP; otherwise "
                         "a multiple of 16 up to 1024)")
    ap.add_argument("--experts-active", type=int, default=MOE_MAX_ACTIVE,
                    help="--experts > 0: experts a token picks, 1..8, capped at --experts")


def build_parser() -> argparse.ArgumentParser:
    p = os.environ.get("GSX_ENV_PREFIX", "SHARED_GPU_MEM")
    ap = _Parser(description="GEMM loop inside the pod's GPU share (the gpushare sample workload)")
    ap.add_argument("--total", type=float, default=float(os.environ.get(f"{p}_DEV", "0") or 0),
                    help="the GPU's gpu-mem (the device plugin's *_DEV env)")
    ap.add_argument("--allocated", type=float, default=float(os.environ.get(f"{p}_CONTAINER", "0") or 0),
                    help="this container's share (the device plugin's *_CONTAINER env)")
    ap.add_argument("--kernel", default="auto", choices=["auto", "gsx", "torch"])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp8", "mxfp4"],
                    help="operand type of the GEMM: bf16, fp8 (OCP e4m3) or mxfp4 (e2m1 with e8m0 block scales, "
                         "quantised from bf16 by the library; --kernel gsx only); the output stays bf16")
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--workload", default="gemm",
                    choices=["gemm", "decode", "attn", "server", "layer", "prefill", "generate"],
                    help="gemm: one large square GEMM per step (compute-bound); decode: --batch activation rows "
                         "against a ring of --size x --size weight matrices, one launch each (HBM-bandwidth-bound); "
                         "attn: one decode step of attention per layer over a ring of paged KV caches; server: a "
                         "whole decode layer per ring layer (QKV projection, RoPE and KV append, attention, output "
                         "projection) over caches that grow; layer: a whole decoder layer per ring layer (the server "
                         "workload's with a residual stream, two RMSNorms and the SwiGLU MLP); prefill: the same layer on "
                         "--batch sequences of --chunk new tokens each, causal attention over the paged cache "
                         "(compute-bound); generate: the layer workload closed into generation: the embedding lookup of "
                         "the last step's tokens, the layers, a final RMSNorm, the LM head (--vocab columns) and the "
                         "sampler, token to token through device memory")
    ap.add_argument("--batch", type=int, default=8, metavar="N",
                    help="--workload decode, server, layer and generate: the activation rows (M), 1..16; --workload attn and "
                         "prefill: the sequences, 1..256")
    add_attn_arguments(ap)
    ap.add_argument("--weights-gib", type=float, default=None,
                    help="--workload decode, server, layer and prefill: size of the weight ring (default 4, or a quarter of the "
                         "share if that is smaller; never fewer than two matrices or layers)")
    ap.add_argument("--ffn", type=int, default=None,
                    help="--workload layer and prefill: width of the MLP (default 3.5 x hidden, rounded to a multiple of 64)")
    add_generate_arguments(ap)
    add_moe_arguments(ap)
    ap.add_argument("--seconds", type=float, default=0.0, help="0 = run forever (like the reference sample)")
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--touch", action="store_true")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--probe-limit", action="store_true", help="check that the memory share is enforced")
    return ap


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    res = run(a.total, a.allocated, kernel=a.kernel, size=a.size, seconds=a.seconds, iters=a.iters, touch=a.touch,
              quiet=a.json, probe_limit=a.probe_limit, dtype=a.dtype, workload=a.workload, batch=a.batch,
              weights_gib=a.weights_gib, context=a.context, heads=a.heads, kv_heads=a.kv_heads, kv_dtype=a.kv_dtype,
              kv_gib=a.kv_gib, page=a.page, ffn=a.ffn, chunk=a.chunk, vocab=a.vocab, temperature=a.temperature,
              top_k=a.top_k, top_p=a.top_p, seed=a.seed, experts=a.experts, experts_active=a.experts_active)
    print(json.dumps(res) if a.json else res, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
