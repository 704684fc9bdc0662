#!/usr/bin/env python3
"""Micro-benchmarks of the HIP kernels on one MI355X: bf16, fp8, block-scaled fp8 and mxfp4 GEMM (ours vs torch/hipBLASLt), the decode
GEMM (every configuration vs torch and a read-bandwidth yardstick), the decode attention over a paged KV cache (every
configuration and split count vs torch SDPA and the same yardstick), RoPE + KV append and the fused add + RMSNorm and
SwiGLU (vs a read-and-rewrite yardstick), the causal prefill attention over the paged cache (vs torch SDPA on a
contiguous copy), the sampler, the MoE router, grouped expert GEMM and combine (vs one plain decode GEMM per active
expert and the read yardstick), the MoE prefill router, tile plan, grouped 128x128 GEMM and combine (vs the dense
128x128 configuration at equal padded rows), HBM fill, stamp/verify."""
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from gpushare_scheduler_extender_amd.ops import hip  # noqa: E402


def gemm(size_list, iters=20):
    out = []
    s = hip.Stream(0)
    for m, n, k in size_list:
        a = torch.rand(m, k, device="cuda", dtype=torch.bfloat16) * 2 - 1
        b = torch.rand(n, k, device="cuda", dtype=torch.bfloat16) * 2 - 1
        c = torch.empty(m, n, device="cuda", dtype=torch.bfloat16)
        torch.cuda.synchronize()
        hip.time_gemm(s, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, 3)
        ms = hip.time_gemm(s, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, iters) / iters
        ours = 2 * m * n * k / ms / 1e9
        for _ in range(3):
            torch.matmul(a, b.t())
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            torch.matmul(a, b.t())
        e1.record()
        torch.cuda.synchronize()
        tms = e0.elapsed_time(e1) / iters
        ref = 2 * m * n * k / tms / 1e9
        err = (c.float() - (a.float() @ b.float().t())).abs().max().item()
        row = {"m": m, "n": n, "k": k, "gsx_tflops": round(ours, 1), "torch_tflops": round(ref, 1),
               "gsx_ms": round(ms, 4), "max_abs_err": round(err, 4)}
        ts = torch.cuda.ExternalStream(s.ptr)
        for cfg, name in hip.gemm_cfgs().items():
            try:
                hip.gemm_bf16_nt_cfg(s, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, cfg)
            except hip.HipError:
                continue
            s.sync()
            e = (c.float() - (a.float() @ b.float().t())).abs().max().item()
            torch.cuda.synchronize()
            with torch.cuda.stream(ts):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(ts)
                for _ in range(iters):
                    hip.gemm_bf16_nt_cfg(s, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, cfg)
                e1.record(ts)
            e1.synchronize()
            cms = e0.elapsed_time(e1) / iters
            row[f"cfg{cfg}_{name}_tflops"] = round(2 * m * n * k / cms / 1e9, 1)
            row[f"cfg{cfg}_err"] = round(e, 4)
        out.append(row)
        del a, b, c
    s.destroy()
    return out


def gemm_fp8(size_list, iters=20, rounds=3):
    """Every fp8 (e4m3) configuration, the bf16 default on operands of the same shape and ``torch._scaled_mm`` with
    unit per-tensor scales, interleaved in one process: median TFLOP/s of ``rounds`` repeats, and each fp8 result's
    max abs error against the fp32 product of the same fp8 operands."""
    out = []
    s = hip.Stream(0)
    ts = torch.cuda.ExternalStream(s.ptr)
    one = torch.ones((), device="cuda", dtype=torch.float32)
    for m, n, k in size_list:
        a16 = torch.rand(m, k, device="cuda", dtype=torch.bfloat16) * 2 - 1
        b16 = torch.rand(n, k, device="cuda", dtype=torch.bfloat16) * 2 - 1
        a, b = a16.to(torch.float8_e4m3fn), b16.to(torch.float8_e4m3fn)
        c = torch.empty(m, n, device="cuda", dtype=torch.bfloat16)
        ref = a.float() @ b.float().t()
        torch.cuda.synchronize()  # operands and reference come from torch's stream; the GEMMs run on ours
        ptrs = (a.data_ptr(), b.data_ptr(), c.data_ptr())
        variants = {f"cfg{cfg}_{name}": (lambda cfg=cfg: hip.gemm_fp8_nt_cfg(s, *ptrs, m, n, k, cfg))
                    for cfg, name in hip.gemm_fp8_cfgs().items()}
        row = {"m": m, "n": n, "k": k}
        for name, fn in variants.items():
            c.zero_()
            torch.cuda.synchronize()
            fn()
            s.sync()
            row[f"{name}_err"] = round((c.float() - ref).abs().max().item(), 4)
        del ref
        variants["gsx"] = lambda: hip.gemm_fp8_nt(s, *ptrs, m, n, k)
        variants["bf16_gsx"] = lambda: hip.gemm_bf16_nt(s, a16.data_ptr(), b16.data_ptr(), c.data_ptr(), m, n, k)
        variants["torch"] = lambda: torch._scaled_mm(a, b.t(), scale_a=one, scale_b=one, out_dtype=torch.bfloat16,
                                                     out=c)

        def timed(fn):
            torch.cuda.synchronize()
            with torch.cuda.stream(ts):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(ts)
                for _ in range(iters):
                    fn()
                e1.record(ts)
            e1.synchronize()
            return 2 * m * n * k / (e0.elapsed_time(e1) / iters) / 1e9

        runs = {name: [] for name in variants}
        for r in range(rounds + 1):  # the first round warms up clocks and code objects
            for name, fn in variants.items():
                t = timed(fn)
                if r:
                    runs[name].append(t)
        for name, r in runs.items():
            row[f"{name}_tflops"] = round(statistics.median(r), 1)
        out.append(row)
        del a, b, a16, b16, c
    s.destroy()
    return out


FP8_BLOCK_SHAPES = [(4096, 4096, 4096), (8192, 8192, 8192),
                    # M = 4096 against the DeepSeek-V3 projections (N, K); the last has four K-tiles
                    (4096, 7168, 2048), (4096, 4096, 7168), (4096, 24576, 1536), (4096, 7168, 16384), (4096, 32768, 512)]


def gemm_fp8_block(shapes=FP8_BLOCK_SHAPES, iters=20, rounds=5):
    """The block-scaled fp8 GEMM (every configuration and the dispatching entry point) on activations quantised by
    ``gsx_quant_fp8_block`` and weights block-quantised in torch, against ``gsx_gemm_fp8_nt`` with per-row scales on
    the same bytes (the ceiling: the same MFMA work without the fold), ``gsx_gemm_bf16_nt`` on the dequantised
    operands (what a user runs today) and torch's own block-scaled ``_scaled_mm`` where this build takes the call (its
    refusal otherwise).  The variants alternate inside every round of one process; per variant the median TFLOP/s of
    ``rounds`` rounds after a warm-up round, and ``spread_pct``, the largest (max - min) / median of any variant."""
    out = []
    s = hip.Stream(0)
    ts = torch.cuda.ExternalStream(s.ptr)
    for m, n, k in shapes:
        g = k // 128
        x = torch.randn(m, k, device="cuda", dtype=torch.bfloat16)
        blocks = torch.randn(n, k, device="cuda").view(n // 128, 128, g, 128)
        sb = (blocks.abs().amax(dim=(1, 3)) / 448.0).contiguous()
        b = (blocks / sb[:, None, :, None]).reshape(n, k).to(torch.float8_e4m3fn)
        del blocks
        a = torch.empty(m, k, device="cuda", dtype=torch.float8_e4m3fn)
        sa = torch.empty(m, g, device="cuda", dtype=torch.float32)
        c = torch.empty(m, n, device="cuda", dtype=torch.bfloat16)
        torch.cuda.synchronize()
        hip.quant_fp8_block(s, x.data_ptr(), k, a.data_ptr(), k, sa.data_ptr(), g, m, k)
        s.sync()
        a16 = (a.float() * sa.repeat_interleave(128, dim=1)).bfloat16()
        b16 = (b.float() * sb.repeat_interleave(128, dim=0).repeat_interleave(128, dim=1)).bfloat16()
        row_a, row_b = sa[:, 0].contiguous(), torch.ones(n, device="cuda")
        ref = a16.float() @ b16.float().t()
        torch.cuda.synchronize()
        ptrs = (a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k)
        scales = (sa.data_ptr(), g, sb.data_ptr())
        row = {"m": m, "n": n, "k": k}
        variants = {}
        for cfg, name in hip.gemm_fp8_block_cfgs().items():
            try:
                hip.gemm_fp8_block_nt_cfg(s, *ptrs, cfg, *scales)
            except hip.HipError:
                continue
            variants[f"cfg{cfg}_{name}"] = lambda cfg=cfg: hip.gemm_fp8_block_nt_cfg(s, *ptrs, cfg, *scales)
        variants["gsx"] = lambda: hip.gemm_fp8_block_nt(s, *ptrs, *scales)
        variants["fp8_row_gsx"] = lambda: hip.gemm_fp8_nt(s, *ptrs, row_a.data_ptr(), row_b.data_ptr(), hip.SCALE_ROW)
        variants["bf16_gsx"] = lambda: hip.gemm_bf16_nt(s, a16.data_ptr(), b16.data_ptr(), c.data_ptr(), m, n, k)
        c.zero_()
        torch.cuda.synchronize()
        variants["gsx"]()
        s.sync()
        row["gsx_rel_err"] = round(((c.float() - ref).abs().max() / ref.abs().max()).item(), 5)
        del ref
        try:  # torch's block-scaled path: scale_a [m][k / 128], scale_b [k / 128][n / 128]
            sbt = sb.t().contiguous()
            torch._scaled_mm(a, b.t(), scale_a=sa, scale_b=sbt, out_dtype=torch.bfloat16)
            variants["torch"] = lambda: torch._scaled_mm(a, b.t(), scale_a=sa, scale_b=sbt, out_dtype=torch.bfloat16,
                                                         out=c)
        except Exception as e:  # noqa: BLE001 - whatever this build answers is the record
            row["torch_refusal"] = str(e).splitlines()[0][:300]

        def timed(fn):
            torch.cuda.synchronize()
            with torch.cuda.stream(ts):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(ts)
                for _ in range(iters):
                    fn()
                e1.record(ts)
            e1.synchronize()
            return 2 * m * n * k / (e0.elapsed_time(e1) / iters) / 1e9

        runs = {name: [] for name in variants}
        for r in range(rounds + 1):  # the first round warms up clocks and code objects
            for name, fn in variants.items():
                t = timed(fn)
                if r:
                    runs[name].append(t)
        for name, r in runs.items():
            row[f"{name}_tflops"] = round(statistics.median(r), 1)
        row["spread_pct"] = round(max((max(r) - min(r)) / statistics.median(r) for r in runs.values()) * 100, 2)
        out.append(row)
        del x, a, b, a16, b16, c
        torch.cuda.empty_cache()
    s.destroy()
    return out


def dequant_mxfp4(q, sc):
    """fp32 values of an MXFP4 operand (``q`` e2m1 pairs, ``sc`` e8m0 block scales), on the GPU."""
    grid = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], device=q.device)
    codes = torch.stack([q & 15, q >> 4], dim=2).reshape(q.shape[0], -1).long()
    vals = grid[codes & 7] * (1 - 2 * (codes >> 3)).float()
    return vals * torch.exp2(sc.float() - 127).repeat_interleave(32, dim=1)


def gemm_mxfp4(size_list, iters=20, rounds=3):
    """Every mxfp4 configuration on random bf16 operands quantised by ``gsx_quant_mxfp4``, the fp8 default and the
    bf16 default on operands of the same shape, interleaved in one process: median TFLOP/s of ``rounds`` repeats, each
    mxfp4 result's max abs error against the fp32 product of the dequantised operands (the ablation row takes every
    scale as 1, so its error is large by design), and the quantiser's GB/s (bytes read and written) next to
    ``gsx_hbm_fill`` over the same number of bytes."""
    out = []
    s = hip.Stream(0)
    ts = torch.cuda.ExternalStream(s.ptr)
    for m, n, k in size_list:
        a16 = torch.randn(m, k, device="cuda", dtype=torch.bfloat16)
        b16 = torch.randn(n, k, device="cuda", dtype=torch.bfloat16)
        a8, b8 = a16.to(torch.float8_e4m3fn), b16.to(torch.float8_e4m3fn)
        qa, qb = (torch.empty(r, k // 2, device="cuda", dtype=torch.uint8) for r in (m, n))
        sa, sb = (torch.empty(r, k // 32, device="cuda", dtype=torch.uint8) for r in (m, n))
        c = torch.empty(m, n, device="cuda", dtype=torch.bfloat16)
        torch.cuda.synchronize()  # operands come from torch's stream; everything below runs on ours
        quant = (lambda: (hip.quant_mxfp4(s, a16.data_ptr(), qa.data_ptr(), sa.data_ptr(), m, k),
                          hip.quant_mxfp4(s, b16.data_ptr(), qb.data_ptr(), sb.data_ptr(), n, k)))
        quant()
        s.sync()
        ref = dequant_mxfp4(qa, sa) @ dequant_mxfp4(qb, sb).t()
        torch.cuda.synchronize()
        ptrs = (qa.data_ptr(), qb.data_ptr(), c.data_ptr())
        scales = (sa.data_ptr(), sb.data_ptr())
        variants = {f"cfg{cfg}_{name}": (lambda cfg=cfg: hip.gemm_mxfp4_nt_cfg(s, *ptrs, m, n, k, cfg, *scales))
                    for cfg, name in hip.gemm_mxfp4_cfgs().items()}
        row = {"m": m, "n": n, "k": k}
        for name, fn in variants.items():
            c.zero_()
            torch.cuda.synchronize()
            fn()
            s.sync()
            row[f"{name}_err"] = round((c.float() - ref).abs().max().item(), 4)
        row["ref_absmax"] = round(ref.abs().max().item(), 1)
        del ref
        variants["gsx"] = lambda: hip.gemm_mxfp4_nt(s, *ptrs, m, n, k, *scales)
        variants["fp8_gsx"] = lambda: hip.gemm_fp8_nt(s, a8.data_ptr(), b8.data_ptr(), c.data_ptr(), m, n, k)
        variants["bf16_gsx"] = lambda: hip.gemm_bf16_nt(s, a16.data_ptr(), b16.data_ptr(), c.data_ptr(), m, n, k)

        def timed(fn, reps=iters):
            torch.cuda.synchronize()
            with torch.cuda.stream(ts):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(ts)
                for _ in range(reps):
                    fn()
                e1.record(ts)
            e1.synchronize()
            return e0.elapsed_time(e1) / reps  # ms

        runs = {name: [] for name in variants}
        qbytes = (m + n) * (2 * k + k // 2 + k // 32)
        fill = hip.DeviceBuffer(0, qbytes & ~255)
        qruns, fruns = [], []
        for r in range(rounds + 1):  # the first round warms up clocks and code objects
            for name, fn in variants.items():
                t = 2 * m * n * k / timed(fn) / 1e9
                if r:
                    runs[name].append(t)
            tq = qbytes / timed(quant, 5) / 1e6
            tf = (qbytes & ~255) / timed(lambda: hip.hbm_fill(s, fill.addr(), qbytes & ~255, r), 5) / 1e6
            if r:
                qruns.append(tq)
                fruns.append(tf)
        fill.free()
        for name, r in runs.items():
            row[f"{name}_tflops"] = round(statistics.median(r), 1)
        row["mxfp4_over_fp8"] = round(row["gsx_tflops"] / row["fp8_gsx_tflops"], 3)
        row["quant_GBps"] = round(statistics.median(qruns), 1)
        row["hbm_fill_GBps"] = round(statistics.median(fruns), 1)
        out.append(row)
        del a16, b16, a8, b8, qa, qb, sa, sb, c
    s.destroy()
    return out


MEMTEST_RANDOM = 3  # gsx_kernels.h: the pattern the memory test's profile times
DECODE_SHAPES = [(8192, 8192), (28672, 8192), (8192, 28672)]  # (N, K): square, an MLP's up and down projections


def gemm_decode(shapes=DECODE_SHAPES, ms=(1, 4, 16), kinds=("bf16", "fp8", "mxfp4"), ring_bytes=(2 << 30) + 1, reps=3,
                rounds=3):
    """The decode GEMM on a ring of weight matrices of more than 2 GiB (the Infinity Cache holds 256 MiB: every launch
    streams its matrix from HBM): every configuration, the dispatching entry point, and ``torch.matmul`` (bf16) or
    ``torch._scaled_mm`` (fp8) on the same ring, interleaved in one process.  One timing is ``reps`` passes over the
    ring between two events; reported are the median TB/s of weight and weight-scale bytes of ``rounds`` repeats and
    their spread, (max - min) / median.  ``memtest_check_TBps`` is the yardstick: ``gsx_memtest_check``, which reads
    and compares every word, over the same number of bytes, by the wall clock around the call (it synchronises)."""
    out = []
    s = hip.Stream(0)
    ts = torch.cuda.ExternalStream(s.ptr)
    one = torch.ones((), device="cuda", dtype=torch.float32)
    for kind in kinds:
        for n, k in shapes:
            wcols = k // 2 if kind == "mxfp4" else k
            per = n * wcols * (2 if kind == "bf16" else 1) + (n * k // 32 if kind == "mxfp4" else 0)
            layers = max(2, -(-ring_bytes // per))
            wdt = {"bf16": torch.bfloat16, "fp8": torch.float8_e4m3fn, "mxfp4": torch.uint8}[kind]
            w = torch.empty(layers, n, wcols, device="cuda", dtype=wdt)
            ws = torch.empty(layers, n, k // 32, device="cuda", dtype=torch.uint8) if kind == "mxfp4" else None
            for i in range(layers):
                x = torch.randn(n, k, device="cuda", dtype=torch.bfloat16)
                if kind == "mxfp4":
                    torch.cuda.synchronize()
                    hip.quant_mxfp4(s, x.data_ptr(), w[i].data_ptr(), ws[i].data_ptr(), n, k)
                    s.sync()
                else:
                    w[i].copy_(x.to(wdt))
                del x
            yard = hip.DeviceBuffer(0, (layers * per) & ~255)
            hip.memtest_write(s, yard.addr(), yard.nbytes, 0, MEMTEST_RANDOM, 1)
            s.sync()
            for m in ms:
                x = torch.randn(m, k, device="cuda", dtype=torch.bfloat16)
                sa = 0
                if kind == "mxfp4":
                    qa = torch.empty(m, k // 2, device="cuda", dtype=torch.uint8)
                    sat = torch.empty(m, k // 32, device="cuda", dtype=torch.uint8)
                    torch.cuda.synchronize()
                    hip.quant_mxfp4(s, x.data_ptr(), qa.data_ptr(), sat.data_ptr(), m, k)
                    s.sync()
                    a, sa = qa, sat.data_ptr()
                else:
                    a = x.to(wdt)
                c = torch.empty(m, n, device="cuda", dtype=torch.bfloat16)
                torch.cuda.synchronize()
                wb, sb = w[0].numel() * w.element_size(), (ws[0].numel() if ws is not None else 0)

                def ours(cfg):
                    for i in range(layers):
                        args = (s, kind, a.data_ptr(), w.data_ptr() + i * wb, c.data_ptr(), m, n, k)
                        scales = (sa, ws.data_ptr() + i * sb if ws is not None else 0)
                        if cfg is None:
                            hip.decode_gemm_nt(*args, *scales)
                        else:
                            hip.decode_gemm_nt_cfg(*args, cfg, *scales)

                def torch_pass():
                    for i in range(layers):
                        if kind == "fp8":
                            torch._scaled_mm(a, w[i].t(), scale_a=one, scale_b=one, out_dtype=torch.bfloat16, out=c)
                        else:
                            torch.matmul(a, w[i].t(), out=c)

                variants = {f"cfg{cfg}_{name}": (lambda cfg=cfg: ours(cfg))
                            for cfg, (name, bn, _, _) in hip.decode_gemm_cfgs().items() if n % bn == 0}
                variants["gsx"] = lambda: ours(None)
                row = {"kind": kind, "m": m, "n": n, "k": k, "layers": layers, "ring_bytes": layers * per}
                if kind != "mxfp4":
                    try:
                        with torch.cuda.stream(ts):
                            torch_pass()
                        ts.synchronize()
                        variants["torch"] = torch_pass
                    except RuntimeError as e:  # torch refuses the shape: said, not hidden
                        row["torch_refused"] = str(e).splitlines()[0][:200]

                def timed(fn):
                    torch.cuda.synchronize()
                    with torch.cuda.stream(ts):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(ts)
                        for _ in range(reps):
                            fn()
                        e1.record(ts)
                    e1.synchronize()
                    return reps * layers * per / (e0.elapsed_time(e1) * 1e-3) / 1e12

                def yardstick():
                    s.sync()
                    t0 = time.perf_counter()
                    rep = hip.memtest_check(s, yard.addr(), yard.nbytes, 0, MEMTEST_RANDOM, 1)
                    dt = time.perf_counter() - t0
                    assert rep.bad_dwords == 0
                    return yard.nbytes / dt / 1e12

                runs = {name: [] for name in [*variants, "memtest_check"]}
                for r in range(rounds + 1):  # the first round warms up clocks and code objects
                    for name, fn in variants.items():
                        t = timed(fn)
                        if r:
                            runs[name].append(t)
                    t = yardstick()
                    if r:
                        runs["memtest_check"].append(t)
                for name, v in runs.items():
                    med = statistics.median(v)
                    row[f"{name}_TBps"] = round(med, 3)
                    row[f"{name}_spread"] = round((max(v) - min(v)) / med, 3)
                out.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
                del x, a, c
            yard.free()
            del w, ws
            torch.cuda.empty_cache()
    s.destroy()
    return out


SKINNY_SHAPES = [(8192, 8192), (8192, 28672), (1024, 8192)]  # decode_pick()'s table, and a narrow N for the split of K


def gemm_skinny(shapes=SKINNY_SHAPES, ms=(17, 32, 64, 128), kinds=("bf16", "fp8"), ring_bytes=(2 << 30) + 1, reps=3,
                rounds=3):
    """The skinny GEMM by the protocol of :func:`gemm_decode` (a ring of weight matrices of more than 2 GiB, ``reps``
    passes between two events, median TB/s of weight bytes of ``rounds`` repeats and the spread): every configuration
    with the dispatched splits, the dispatched configuration with other splits (``gsx_s<splits>``), the dispatching
    entry point (``gsx``), and the yardsticks: ``decode_slices``, ``ceil(M / 16)`` calls of the decode GEMM on 16-row
    slices of the same operands (how these shapes run without this kernel: the bar); ``decode_m16``, one decode GEMM of
    16 rows; ``gemm128``, the large GEMM's "128x128/4w" on A padded to 128 rows; and torch."""
    out = []
    s = hip.Stream(0)
    ts = torch.cuda.ExternalStream(s.ptr)
    one = torch.ones((), device="cuda", dtype=torch.float32)
    big = {"bf16": ({name: i for i, name in hip.gemm_cfgs().items()}["128x128/4w"], hip.gemm_bf16_nt_cfg),
           "fp8": ({name: i for i, name in hip.gemm_fp8_cfgs().items()}["128x128/4w"], hip.gemm_fp8_nt_cfg)}
    for kind in kinds:
        wdt, unit = (torch.bfloat16, 2) if kind == "bf16" else (torch.float8_e4m3fn, 1)
        for n, k in shapes:
            per = n * k * unit
            layers = max(2, -(-ring_bytes // per))
            w = torch.empty(layers, n, k, device="cuda", dtype=wdt)
            for i in range(layers):
                w[i].copy_(torch.randn(n, k, device="cuda", dtype=torch.bfloat16).to(wdt))
            part = torch.empty(16 * 128 * n * 4, device="cuda", dtype=torch.uint8)
            for m in ms:
                a = torch.zeros(128, k, device="cuda", dtype=torch.bfloat16)  # rows m .. 127: the padding of gemm128
                a[:m] = torch.randn(m, k, device="cuda", dtype=torch.bfloat16)
                a = a.to(wdt)
                c = torch.empty(128, n, device="cuda", dtype=torch.bfloat16)
                torch.cuda.synchronize()
                row_a, row_c = k * unit, n * 2

                def skinny(cfg, splits):
                    for i in range(layers):
                        args = (s, kind, a.data_ptr(), w.data_ptr() + i * per, c.data_ptr(), m, n, k)
                        ws = {"workspace": part.data_ptr(), "workspace_bytes": part.numel()}
                        if cfg is None:
                            hip.skinny_gemm_nt(*args, **ws)
                        else:
                            hip.skinny_gemm_nt_cfg(*args, cfg, splits, **ws)

                def decode(rows):
                    for i in range(layers):
                        for r0 in range(0, rows, 16):
                            hip.decode_gemm_nt(s, kind, a.data_ptr() + r0 * row_a, w.data_ptr() + i * per,
                                               c.data_ptr() + r0 * row_c, min(16, rows - r0), n, k)

                def gemm128():
                    for i in range(layers):
                        big[kind][1](s, a.data_ptr(), w.data_ptr() + i * per, c.data_ptr(), 128, n, k, big[kind][0])

                def torch_pass():
                    for i in range(layers):
                        if kind == "fp8":
                            torch._scaled_mm(a[:m], w[i].t(), scale_a=one, scale_b=one, out_dtype=torch.bfloat16,
                                             out=c[:m])
                        else:
                            torch.matmul(a[:m], w[i].t(), out=c[:m])

                cfg0, splits0 = hip.skinny_gemm_pick(kind, m, n, k)
                variants = {f"cfg{cfg}_{name}": (lambda cfg=cfg: skinny(cfg, splits0))
                            for cfg, (name, bn, _, _) in hip.skinny_gemm_cfgs().items() if n % bn == 0}
                variants.update({f"gsx_s{sp}": (lambda sp=sp: skinny(cfg0, sp)) for sp in (1, 2, 4, 8) if sp != splits0})
                variants.update({"gsx": lambda: skinny(None, 0), "decode_slices": lambda: decode(m),
                                 "decode_m16": lambda: decode(16), "gemm128": gemm128})
                row = {"kind": kind, "m": m, "n": n, "k": k, "layers": layers, "ring_bytes": layers * per,
                       "picked": hip.skinny_gemm_cfgs()[cfg0][0], "picked_splits": splits0}
                try:
                    with torch.cuda.stream(ts):
                        torch_pass()
                    ts.synchronize()
                    variants["torch"] = torch_pass
                except RuntimeError as e:  # torch refuses the shape: said, not hidden
                    row["torch_refused"] = str(e).splitlines()[0][:200]

                def timed(fn):
                    torch.cuda.synchronize()
                    with torch.cuda.stream(ts):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(ts)
                        for _ in range(reps):
                            fn()
                        e1.record(ts)
                    e1.synchronize()
                    return reps * layers * per / (e0.elapsed_time(e1) * 1e-3) / 1e12

                runs = {name: [] for name in variants}
                for r in range(rounds + 1):  # the first round warms up clocks and code objects
                    for name, fn in variants.items():
                        t = timed(fn)
                        if r:
                            runs[name].append(t)
                for name, v in runs.items():
                    med = statistics.median(v)
                    row[f"{name}_TBps"] = round(med, 3)
                    row[f"{name}_spread"] = round((max(v) - min(v)) / med, 3)
                # the bar: faster than the slices by more than the larger of the two spreads
                margin = max(row["gsx_spread"], row["decode_slices_spread"])
                row["beats_decode_slices"] = row["gsx_TBps"] > row["decode_slices_TBps"] * (1 + margin)
                out.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
                del a, c
            del w, part
    s.destroy()
    return out


def gemm_skinny_fp8_block(shapes=(*SKINNY_SHAPES, FP8_BLOCK_SHAPES[3][1:], FP8_BLOCK_SHAPES[5][1:]),
                          ms=(17, 32, 64, 128), ring_bytes=(2 << 30) + 1, reps=3, rounds=3):
    """The block-scaled fp8 skinny GEMM on the method of :func:`gemm_skinny` (a ring of weight matrices of more than
    2 GiB, variants alternating inside a round, one warm-up round, median TB/s of weight bytes and the spread): every
    configuration with the dispatched splits, the dispatched configuration with the neighbouring splits
    (``gsx_s<splits>``), the dispatching entry point (``gsx``), the bar (``pad128``: ``gsx_gemm_fp8_block_nt`` on A
    and scale_a padded to 128 rows, the only way to run these shapes without this kernel) and the ceiling
    (``skinny_fp8_row``: ``gsx_skinny_gemm_nt`` in fp8 with per-row scales on the same codes)."""
    out = []
    s = hip.Stream(0)
    for n, k in shapes:
        per, g = n * k, k // 128
        layers = max(2, -(-ring_bytes // per))
        w = torch.empty(layers, n, k, device="cuda", dtype=torch.float8_e4m3fn)
        wsb = torch.empty(layers, -(-n // 128), g, device="cuda", dtype=torch.float32).uniform_(0.5, 2.0)
        for i in range(layers):
            w[i].copy_(torch.randn(n, k, device="cuda", dtype=torch.bfloat16).to(torch.float8_e4m3fn))
        part = torch.empty(16 * 128 * n * 4, device="cuda", dtype=torch.uint8)
        ws = {"workspace": part.data_ptr(), "workspace_bytes": part.numel()}
        sb_row = torch.ones(n, device="cuda", dtype=torch.float32)
        for m in ms:
            x = torch.zeros(128, k, device="cuda", dtype=torch.bfloat16)  # rows m .. 127: the padding of the bar
            x[:m] = torch.randn(m, k, device="cuda", dtype=torch.bfloat16)
            a = torch.empty(128, k, device="cuda", dtype=torch.uint8)
            sa = torch.empty(128, g, device="cuda", dtype=torch.float32)
            sa_row = torch.ones(128, device="cuda", dtype=torch.float32)
            c = torch.empty(128, n, device="cuda", dtype=torch.bfloat16)
            torch.cuda.synchronize()
            hip.quant_fp8_block(s, x.data_ptr(), k, a.data_ptr(), k, sa.data_ptr(), g, 128, k)
            s.sync()

            def skinny(cfg, splits):
                for i in range(layers):
                    args = (s, a.data_ptr(), w.data_ptr() + i * per, c.data_ptr(), m, n, k)
                    sc = {"scale_a": sa.data_ptr(), "sa_stride": g, "scale_b": wsb[i].data_ptr()}
                    if cfg is None:
                        hip.skinny_gemm_fp8_block_nt(*args, **sc, **ws)
                    else:
                        hip.skinny_gemm_fp8_block_nt_cfg(*args, cfg, splits, **sc, **ws)

            def pad128():
                for i in range(layers):
                    hip.gemm_fp8_block_nt(s, a.data_ptr(), w.data_ptr() + i * per, c.data_ptr(), 128, n, k,
                                          sa.data_ptr(), g, wsb[i].data_ptr())

            def skinny_fp8_row():
                for i in range(layers):
                    hip.skinny_gemm_nt(s, "fp8", a.data_ptr(), w.data_ptr() + i * per, c.data_ptr(), m, n, k,
                                       scale_a=sa_row.data_ptr(), scale_b=sb_row.data_ptr(), scale_mode=hip.SCALE_ROW,
                                       **ws)

            cfg0, splits0 = hip.skinny_gemm_fp8_block_pick(m, n, k)
            cfgs = hip.skinny_gemm_fp8_block_cfgs()
            variants = {f"cfg{cfg}_{name}": (lambda cfg=cfg: skinny(cfg, splits0))
                        for cfg, (name, bn, _, _) in cfgs.items() if n % bn == 0}
            variants.update({f"gsx_s{sp}": (lambda sp=sp: skinny(cfg0, sp))
                             for sp in {max(1, splits0 // 2), min(16, splits0 * 2)} - {splits0}})
            variants.update({"gsx": lambda: skinny(None, 0), "skinny_fp8_row": skinny_fp8_row})
            if n % 128 == 0:
                variants["pad128"] = pad128
            row = {"m": m, "n": n, "k": k, "layers": layers, "ring_bytes": layers * per, "picked": cfgs[cfg0][0],
                   "picked_splits": splits0}

            def timed(fn):
                s.sync()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ts = torch.cuda.ExternalStream(s.ptr)
                e0.record(ts)
                for _ in range(reps):
                    fn()
                e1.record(ts)
                e1.synchronize()
                return reps * layers * per / (e0.elapsed_time(e1) * 1e-3) / 1e12

            runs = {name: [] for name in variants}
            for r in range(rounds + 1):  # the first round warms up clocks and code objects
                for name, fn in variants.items():
                    t = timed(fn)
                    if r:
                        runs[name].append(t)
            for name, v in runs.items():
                med = statistics.median(v)
                row[f"{name}_TBps"] = round(med, 3)
                row[f"{name}_spread"] = round((max(v) - min(v)) / med, 3)
            row["spread"] = max(v for key, v in row.items() if key.endswith("_spread"))
            if "pad128_TBps" in row:
                row["beats_pad128"] = row["gsx_TBps"] > row["pad128_TBps"] * (1 + row["spread"])
            row["of_skinny_fp8_row"] = round(row["gsx_TBps"] / row["skinny_fp8_row_TBps"], 3)
            out.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            del x, a, sa, c
        del w, wsb, part
    s.destroy()
    return out


ATTN_SHAPES =[(1, 32768), (8, 8192), (64, 2048), (256, 1024)]  # (sequences, tokens each)
ATTN_HEADS = [(64, 8), (32, 32)]  # (query heads, KV heads): groups of 8, and plain multi-head attention
ATTN_SPLITS = (1, 2, 4, 8, 16, 32, 64)


def attn_decode(shapes=ATTN_SHAPES, heads=ATTN_HEADS, kinds=("bf16", "fp8"), ring_bytes=(1 << 30) + 1, reps=3,
                rounds=3, page=16, splits=ATTN_SPLITS):
    """The decode attention on a ring of per-layer paged KV caches of more than 1 GiB (the Infinity Cache holds 256
    MiB), pages of 16 tokens handed out through a random permutation: every configuration at every split count that
    leaves a split a tile and the launch no more than 16384 workgroups, the dispatching entry point, and (bf16)
    ``scaled_dot_product_attention(enable_gqa=True)`` on a contiguous copy of the same layers, interleaved in one
    process.  One timing is ``reps`` passes over the ring between two events; reported are the median TB/s of KV bytes
    of ``rounds`` repeats and their spread.  ``memtest_check_TBps`` is the read yardstick over the same number of
    bytes, as in :func:`gemm_decode`: ONE call timed by the host's clock, report read-back included, so the fixed
    host cost of a call of 0.25 to 1.5 ms makes it read low, by an amount that was not measured, and the comparison
    favours the attention, which is timed by events over ``reps`` passes."""
    out = []
    s = hip.Stream(0)
    ts = torch.cuda.ExternalStream(s.ptr)
    d = 128
    sdpa = torch.nn.functional.scaled_dot_product_attention
    for kind in kinds:
        kdt = torch.bfloat16 if kind == "bf16" else torch.float8_e4m3fn
        for hq, hkv in heads:
            for b, ctx in shapes:
                per_seq = -(-ctx // page)
                pages = b * per_seq
                per = 2 * pages * hkv * page * d * (2 if kind == "bf16" else 1)
                layers = max(2, -(-ring_bytes // per))
                kc = torch.empty(layers, pages, hkv, page, d, device="cuda", dtype=kdt)
                vc = torch.empty_like(kc)
                for i in range(layers):
                    for c in (kc, vc):
                        c[i].copy_(torch.randn(pages, hkv, page, d, device="cuda", dtype=torch.bfloat16).to(kdt))
                table = torch.randperm(pages, device="cuda").to(torch.int32).view(b, per_seq).contiguous()
                lens = torch.full((b,), ctx, device="cuda", dtype=torch.int32)
                q = torch.randn(b, hq, d, device="cuda", dtype=torch.bfloat16)
                o = torch.empty_like(q)
                ws = torch.empty(b * hq * max(splits) * 520, device="cuda", dtype=torch.uint8)
                lb = kc[0].numel() * kc.element_size()
                scale = d ** -0.5
                yard = hip.DeviceBuffer(0, (layers * per) & ~255)
                hip.memtest_write(s, yard.addr(), yard.nbytes, 0, MEMTEST_RANDOM, 1)
                s.sync()

                def ours(cfg, sp):
                    for i in range(layers):
                        args = (s, kind, q.data_ptr(), kc.data_ptr() + i * lb, vc.data_ptr() + i * lb,
                                table.data_ptr(), lens.data_ptr(), o.data_ptr(), b, hq, hkv, d, page, pages, per_seq,
                                ctx, scale)
                        if cfg is None:
                            hip.decode_attn(*args, 1.0, 1.0, ws.data_ptr(), ws.numel())
                        else:
                            hip.decode_attn_cfg(*args, cfg, sp, 1.0, 1.0, ws.data_ptr(), ws.numel())

                tiles = -(-ctx // 32)
                variants = {f"cfg{cfg}_{name}_s{sp}": (lambda cfg=cfg, sp=sp: ours(cfg, sp))
                            for cfg, (name, _, _) in hip.decode_attn_cfgs().items() for sp in splits
                            if sp <= tiles and b * hkv * sp <= 16384}
                variants["gsx"] = lambda: ours(None, None)
                row = {"kind": kind, "b": b, "context": ctx, "heads": hq, "kv_heads": hkv, "page": page,
                       "layers": layers, "ring_bytes": layers * per}
                if kind == "bf16":  # torch's SDPA on a contiguous copy of the same layers
                    idx = table.long()
                    kt, vt = (torch.stack([c[i][idx].permute(0, 2, 1, 3, 4).reshape(b, hkv, per_seq * page, d)[:, :, :ctx]
                                           for i in range(layers)]).contiguous() for c in (kc, vc))
                    q4 = q.unsqueeze(2)

                    def torch_pass():
                        for i in range(layers):
                            o.copy_(sdpa(q4, kt[i], vt[i], scale=scale, enable_gqa=hq != hkv).squeeze(2))

                    variants["torch"] = torch_pass

                def timed(fn):
                    torch.cuda.synchronize()
                    with torch.cuda.stream(ts):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(ts)
                        for _ in range(reps):
                            fn()
                        e1.record(ts)
                    e1.synchronize()
                    return reps * layers * per / (e0.elapsed_time(e1) * 1e-3) / 1e12

                def yardstick():
                    s.sync()
                    t0 = time.perf_counter()
                    rep = hip.memtest_check(s, yard.addr(), yard.nbytes, 0, MEMTEST_RANDOM, 1)
                    dt = time.perf_counter() - t0
                    assert rep.bad_dwords == 0
                    return yard.nbytes / dt / 1e12

                if kind == "bf16":  # the two agree (on the ring's last layer) before they are compared for speed
                    torch.cuda.synchronize()  # the operands were made on torch's stream
                    ours(None, None)
                    s.sync()
                    got = o.float().clone()
                    torch.cuda.synchronize()
                    with torch.cuda.stream(ts):
                        torch_pass()
                    torch.cuda.synchronize()
                    row["max_abs_diff_vs_torch"] = round((got - o.float()).abs().max().item(), 5)
                runs = {name: [] for name in [*variants, "memtest_check"]}
                for r in range(rounds + 1):  # the first round warms up clocks and code objects
                    for name, fn in variants.items():
                        t = timed(fn)
                        if r:
                            runs[name].append(t)
                    t = yardstick()
                    if r:
                        runs["memtest_check"].append(t)
                for name, v in runs.items():
                    med = statistics.median(v)
                    row[f"{name}_TBps"] = round(med, 3)
                    row[f"{name}_spread"] = round((max(v) - min(v)) / med, 3)
                out.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
                yard.free()
                del kc, vc, table, lens, q, o, ws
                if kind == "bf16":
                    del kt, vt
                torch.cuda.empty_cache()
    s.destroy()
    return out


ATTN_MULTI_ROWS = [(64, 8, 1, 32768, (2, 4, 8)), (64, 8, 8, 8192, (2, 4, 8)), (64, 8, 64, 2048, (2, 4, 8)),
                   (32, 32, 8, 8192, (2, 4, 8, 16))]  # (query heads, KV heads, sequences, tokens each, new tokens)


def attn_multi(rows=ATTN_MULTI_ROWS, kinds=("bf16", "fp8"), ring_bytes=(1 << 30) + 1, reps=3, rounds=3, page=16,
               splits=ATTN_SPLITS):
    """The multi-token decode attention under the protocol of :func:`attn_decode` (a ring of per-layer paged KV caches
    of more than 1 GiB, pages of 16 tokens in random order, the median of ``rounds`` repeats after a warm-up round,
    everything interleaved in one process): every configuration at every split count that makes 64 to 2048 workgroups
    of at least a tile per wave, the dispatching entry point ``gsx``, and three yardsticks on the same caches:
    ``decode_x_T`` (T launches of ``gsx_decode_attn``: how the shape runs today on the bandwidth path), ``prefill``
    (``gsx_prefill_attn`` at the same T: the only single-launch way today) and ``decode_1`` (one launch of
    ``gsx_decode_attn``: the floor, the cache streamed once).  Reported are microseconds per layer and the spread
    (max - min) / median; ``gsx_beats_both`` says whether ``gsx`` is faster than ``decode_x_T`` and ``prefill`` by more
    than the row's largest spread."""
    out = []
    s = hip.Stream(0)
    ts = torch.cuda.ExternalStream(s.ptr)
    d = 128
    cfgs = {}
    while (name := hip.decode_attn_multi_cfg_name(len(cfgs))) is not None:
        cfgs[len(cfgs)] = (name, *hip.decode_attn_multi_cfg_shape(len(cfgs)))
    for kind in kinds:
        kdt = torch.bfloat16 if kind == "bf16" else torch.float8_e4m3fn
        for hq, hkv, b, ctx, ts_new in rows:
            per_seq = -(-ctx // page)
            pages = b * per_seq
            per = 2 * pages * hkv * page * d * (2 if kind == "bf16" else 1)
            layers = max(2, -(-ring_bytes // per))
            kc = torch.empty(layers, pages, hkv, page, d, device="cuda", dtype=kdt)
            vc = torch.empty_like(kc)
            for i in range(layers):
                for c in (kc, vc):
                    c[i].copy_(torch.randn(pages, hkv, page, d, device="cuda", dtype=torch.bfloat16).to(kdt))
            table = torch.randperm(pages, device="cuda").to(torch.int32).view(b, per_seq).contiguous()
            full = torch.full((b,), ctx, device="cuda", dtype=torch.int32)
            lb = kc[0].numel() * kc.element_size()
            scale = d ** -0.5
            tmax = max(ts_new)
            q = torch.randn(b * tmax, hq, d, device="cuda", dtype=torch.bfloat16)
            o = torch.empty_like(q)
            ws = torch.empty(max(b * tmax * hq * max(splits) * 520,
                                 hip.decode_attn_workspace_bytes(b, hq, d, page, ctx)), device="cuda", dtype=torch.uint8)
            for t in ts_new:
                before = torch.full((b,), ctx - t, device="cuda", dtype=torch.int32)  # the lengths before the chunk
                torch.cuda.synchronize()

                def layer_args(i, lens, *shape):
                    return (s, kind, q.data_ptr(), kc.data_ptr() + i * lb, vc.data_ptr() + i * lb, table.data_ptr(),
                            lens.data_ptr(), o.data_ptr(), b, *shape, hq, hkv, d, page, pages, per_seq, ctx, scale)

                def ours(cfg, sp):
                    for i in range(layers):
                        if cfg is None:
                            hip.decode_attn_multi(*layer_args(i, before, t), 1.0, 1.0, ws.data_ptr(), ws.numel())
                        else:
                            hip.decode_attn_multi_launch_cfg(*layer_args(i, before, t), cfg, sp, 1.0, 1.0,
                                                             ws.data_ptr(), ws.numel())

                def decode(times):
                    for i in range(layers):
                        for _ in range(times):
                            hip.decode_attn(*layer_args(i, full), 1.0, 1.0, ws.data_ptr(), ws.numel())

                def prefill():
                    for i in range(layers):
                        hip.prefill_attn(*layer_args(i, before, t))

                tiles = -(-ctx // 32)
                variants = {f"cfg{cfg}_{name}_s{sp}": (lambda cfg=cfg, sp=sp: ours(cfg, sp))
                            for cfg, (name, waves, _) in cfgs.items() for sp in splits
                            if sp * waves <= tiles and 64 <= b * hkv * sp <= 2048}
                variants.update({"gsx": lambda: ours(None, None), "decode_x_T": lambda: decode(t), "prefill": prefill,
                                 "decode_1": lambda: decode(1)})

                def timed(fn):
                    torch.cuda.synchronize()
                    with torch.cuda.stream(ts):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(ts)
                        for _ in range(reps):
                            fn()
                        e1.record(ts)
                    e1.synchronize()
                    return e0.elapsed_time(e1) * 1e3 / (reps * layers)  # microseconds per layer

                runs = {name: [] for name in variants}
                for r in range(rounds + 1):  # the first round warms up clocks and code objects
                    for name, fn in variants.items():
                        us = timed(fn)
                        if r:
                            runs[name].append(us)
                row = {"kind": kind, "b": b, "context": ctx, "heads": hq, "kv_heads": hkv, "new_tokens": t,
                       "page": page, "layers": layers, "ring_bytes": layers * per}
                for name, v in runs.items():
                    med = statistics.median(v)
                    row[f"{name}_us"] = round(med, 2)
                    row[f"{name}_spread"] = round((max(v) - min(v)) / med, 3)
                margin = max(v for k, v in row.items() if k.endswith("_spread"))
                row["gsx_TBps"] = round(per / (row["gsx_us"] * 1e-6) / 1e12, 3)
                row["gsx_over_decode_1"] = round(row["gsx_us"] / row["decode_1_us"], 3)
                row["best"] = min((k for k in runs if k.startswith("cfg")), key=lambda k: row[f"{k}_us"])
                row["gsx_beats_both"] = row["gsx_us"] * (1 + margin) < min(row["decode_x_T_us"], row["prefill_us"])
                out.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
            del kc, vc, table, full, q, o, ws
            torch.cuda.empty_cache()
    s.destroy()
    return out


def attn_mla(shapes=ATTN_SHAPES[:3], heads=(16, 128), kinds=("bf16", "fp8"), ring_bytes=(1 << 30) + 1, reps=3, rounds=3,
             page=16, splits=ATTN_SPLITS):
    """The MLA decode attention under the protocol of :func:`attn_decode`: a ring of per-layer latent caches
    (``[pages][page][576]``) of more than 1 GiB, pages of 16 tokens handed out through a random permutation, the median
    of ``rounds`` repeats after a warm-up round, every column interleaved in one process.  Columns: every configuration
    at every split count that leaves a split 8 tiles and makes 16 to 4096 workgroups, the dispatching entry point
    ``gsx``, and ``torch``, the yardstick that is not the code under test: torch's own path on the gathered dense
    latent of the same layers in bf16 (batched matmul over 576, softmax in fp32, batched matmul over 512).  Reported
    are microseconds per layer with the spread (max - min) / median, ``gsx_TBps`` (rows of 576 elements) and
    ``gsx_TFLOPs`` (2 * Hq * (576 + 512) per cached token); ``gsx_beats_torch`` says whether ``gsx`` is faster than
    ``torch`` by more than the row's largest spread."""
    out = []
    s = hip.Stream(0)
    ts = torch.cuda.ExternalStream(s.ptr)
    dk, dv = 576, 512
    cfgs = {}
    while (name := hip.mla_decode_attn_cfg_name(len(cfgs))) is not None:
        cfgs[len(cfgs)] = (name, *hip.mla_decode_attn_cfg_shape(len(cfgs)))
    scale = 192 ** -0.5
    for kind in kinds:
        kdt = torch.bfloat16 if kind == "bf16" else torch.float8_e4m3fn
        for b, ctx in shapes:
            per_seq = -(-ctx // page)
            pages = b * per_seq
            per = pages * page * dk * (2 if kind == "bf16" else 1)
            layers = max(2, -(-ring_bytes // per))
            kv = torch.empty(layers, pages, page, dk, device="cuda", dtype=kdt)
            for i in range(layers):
                kv[i].copy_(torch.randn(pages, page, dk, device="cuda", dtype=torch.bfloat16).to(kdt))
            table = torch.randperm(pages, device="cuda").to(torch.int32).view(b, per_seq).contiguous()
            lens = torch.full((b,), ctx, device="cuda", dtype=torch.int32)
            lb = kv[0].numel() * kv.element_size()
            # the dense latent of every layer, gathered and in bf16: [layers][B][ctx][576]
            idx = table.long()
            raw = kv if kind == "bf16" else kv.view(torch.uint8)  # gathered as bytes: the values are the same
            dense = torch.stack([raw[i][idx].view(kdt).reshape(b, per_seq * page, dk)[:, :ctx].to(torch.bfloat16)
                                 for i in range(layers)]).contiguous()
            for hq in heads:
                q = torch.randn(b, hq, dk, device="cuda", dtype=torch.bfloat16)
                o = torch.empty(b, hq, dv, device="cuda", dtype=torch.bfloat16)
                ws = torch.empty(max(b * hq * max(splits) * 2056, 16), device="cuda", dtype=torch.uint8)
                torch.cuda.synchronize()

                def ours(cfg, sp):
                    for i in range(layers):
                        args = (s, kind, q.data_ptr(), kv.data_ptr() + i * lb, table.data_ptr(), lens.data_ptr(),
                                o.data_ptr(), b, hq, page, pages, per_seq, ctx, scale)
                        if cfg is None:
                            hip.mla_decode_attn(*args, 1.0, ws.data_ptr(), ws.numel())
                        else:
                            hip.mla_decode_attn_launch_cfg(*args, cfg, sp, 1.0, ws.data_ptr(), ws.numel())

                def torch_pass():
                    for i in range(layers):
                        p = torch.softmax(torch.matmul(q, dense[i].transpose(1, 2)).float() * scale, dim=-1)
                        o.copy_(torch.matmul(p.to(torch.bfloat16), dense[i][:, :, :dv]))

                tiles, nhb = -(-ctx // 32), 2 if hq > 64 else 1
                variants = {f"cfg{cfg}_{name}_s{sp}": (lambda cfg=cfg, sp=sp: ours(cfg, sp))
                            for cfg, (name, _, _) in cfgs.items() for sp in splits
                            if sp * 8 <= tiles and 16 <= b * nhb * sp <= 4096}
                variants.update({"gsx": lambda: ours(None, None), "torch": torch_pass})

                def timed(fn):
                    torch.cuda.synchronize()
                    with torch.cuda.stream(ts):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(ts)
                        for _ in range(reps):
                            fn()
                        e1.record(ts)
                    e1.synchronize()
                    return e0.elapsed_time(e1) * 1e3 / (reps * layers)  # microseconds per layer

                # the two agree (on the ring's last layer) before they are compared for speed
                ours(None, None)
                s.sync()
                got = o.float().clone()
                with torch.cuda.stream(ts):
                    torch_pass()
                torch.cuda.synchronize()
                row = {"kind": kind, "b": b, "context": ctx, "heads": hq, "page": page, "layers": layers,
                       "ring_bytes": layers * per, "max_abs_diff_vs_torch": round((got - o.float()).abs().max().item(), 5)}
                runs = {name: [] for name in variants}
                for r in range(rounds + 1):  # the first round warms up clocks and code objects
                    for name, fn in variants.items():
                        us = timed(fn)
                        if r:
                            runs[name].append(us)
                for name, v in runs.items():
                    med = statistics.median(v)
                    row[f"{name}_us"] = round(med, 2)
                    row[f"{name}_spread"] = round((max(v) - min(v)) / med, 3)
                margin = max(v for k, v in row.items() if k.endswith("_spread"))
                row["spread"] = margin
                row["gsx_TBps"] = round(per / (row["gsx_us"] * 1e-6) / 1e12, 3)
                row["gsx_TFLOPs"] = round(2.0 * b * ctx * hq * (dk + dv) / (row["gsx_us"] * 1e-6) / 1e12, 1)
                row["best"] = min((k for k in runs if k.startswith("cfg")), key=lambda k: row[f"{k}_us"])
                row["gsx_over_best"] = round(row["gsx_us"] / row[row["best"] + "_us"], 3)
                row["gsx_beats_torch"] = row["gsx_us"] * (1 + margin) < row["torch_us"]
                out.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
                del q, o, ws
            del kv, dense, table, lens
            torch.cuda.empty_cache()
    s.destroy()
    return out


def attn_mla_multi(shapes=ATTN_SHAPES[:3], heads=(16, 128), new_tokens=(2, 4, 8), kinds=("bf16", "fp8"),
                   ring_bytes=(1 << 30) + 1, reps=3, rounds=3, page=16, splits=ATTN_SPLITS):
    """The multi-token MLA decode attention under the protocol of :func:`attn_mla`, against the yardstick that is not
    the code under test: ``single``, T back-to-back ``gsx_mla_decode_attn`` calls (the dispatching single-token entry
    point) on the same ring, the same block table and the same base lengths, call t on the lengths ``base + t + 1``
    and on token t's rows of Q.  ``context`` counts the T new tokens (base = context - T).  Columns: ``gsx``, the
    dispatching ``gsx_mla_decode_attn_multi``; every configuration at every split count that leaves a split 8 tiles
    and makes 16 to 4096 workgroups; ``single``.  Reported are microseconds per layer with the spread (max - min) /
    median, ``single_over_gsx``, and ``gsx_beats_single``: ``gsx`` faster than ``single`` by more than the row's largest
    spread.  ``max_abs_diff_vs_single`` compares the two on the ring's last layer first."""
    out = []
    s = hip.Stream(0)
    ts = torch.cuda.ExternalStream(s.ptr)
    dk, dv = 576, 512
    cfgs = {}
    while (name := hip.mla_decode_attn_multi_cfg_name(len(cfgs))) is not None:
        cfgs[len(cfgs)] = (name, *hip.mla_decode_attn_multi_cfg_shape(len(cfgs)))
    scale = 192 ** -0.5
    for kind in kinds:
        kdt = torch.bfloat16 if kind == "bf16" else torch.float8_e4m3fn
        for b, ctx in shapes:
            per_seq = -(-ctx // page)
            pages = b * per_seq
            per = pages * page * dk * (2 if kind == "bf16" else 1)
            layers = max(2, -(-ring_bytes // per))
            kv = torch.empty(layers, pages, page, dk, device="cuda", dtype=kdt)
            for i in range(layers):
                kv[i].copy_(torch.randn(pages, page, dk, device="cuda", dtype=torch.bfloat16).to(kdt))
            table = torch.randperm(pages, device="cuda").to(torch.int32).view(b, per_seq).contiguous()
            lb = kv[0].numel() * kv.element_size()
            for hq in heads:
                for t in new_tokens:
                    q = torch.randn(b, t, hq, dk, device="cuda", dtype=torch.bfloat16)
                    o = torch.empty(b, t, hq, dv, device="cuda", dtype=torch.bfloat16)
                    q1 = [q[:, j].contiguous() for j in range(t)]  # what the single-token calls take: [B][Hq][576]
                    o1 = torch.empty(t, b, hq, dv, device="cuda", dtype=torch.bfloat16)
                    before = torch.full((b,), ctx - t, device="cuda", dtype=torch.int32)
                    lens1 = [before + j + 1 for j in range(t)]
                    ws = torch.empty(max(b * t * hq * max(splits) * 2056, 16), device="cuda", dtype=torch.uint8)
                    ws1 = torch.empty(max(hip.mla_decode_attn_workspace_bytes(b, hq, page, ctx), 16), device="cuda",
                                      dtype=torch.uint8)
                    torch.cuda.synchronize()

                    def ours(cfg, sp):
                        for i in range(layers):
                            args = (s, kind, q.data_ptr(), kv.data_ptr() + i * lb, table.data_ptr(), before.data_ptr(),
                                    o.data_ptr(), b, t, hq, page, pages, per_seq, ctx, scale)
                            if cfg is None:
                                hip.mla_decode_attn_multi(*args, 1.0, ws.data_ptr(), ws.numel())
                            else:
                                hip.mla_decode_attn_multi_launch_cfg(*args, cfg, sp, 1.0, ws.data_ptr(), ws.numel())

                    def single():
                        for i in range(layers):
                            for j in range(t):
                                hip.mla_decode_attn(s, kind, q1[j].data_ptr(), kv.data_ptr() + i * lb, table.data_ptr(),
                                                    lens1[j].data_ptr(), o1[j].data_ptr(), b, hq, page, pages, per_seq,
                                                    ctx, scale, 1.0, ws1.data_ptr(), ws1.numel())

                    tiles, nblk = -(-ctx // 32), -(-t * hq // 64)
                    variants = {f"cfg{cfg}_{name}_s{sp}": (lambda cfg=cfg, sp=sp: ours(cfg, sp))
                                for cfg, (name, _, _) in cfgs.items() for sp in splits
                                if sp * 8 <= tiles and 16 <= b * nblk * sp <= 4096}
                    variants.update({"gsx": lambda: ours(None, None), "single": single})

                    def timed(fn):
                        torch.cuda.synchronize()
                        with torch.cuda.stream(ts):
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record(ts)
                            for _ in range(reps):
                                fn()
                            e1.record(ts)
                        e1.synchronize()
                        return e0.elapsed_time(e1) * 1e3 / (reps * layers)  # microseconds per layer

                    # the two agree (on the ring's last layer) before they are compared for speed
                    ours(None, None)
                    single()
                    s.sync()
                    diff = (o.float() - o1.float().transpose(0, 1)).abs().max().item()
                    row = {"kind": kind, "b": b, "context": ctx, "heads": hq, "new_tokens": t, "page": page,
                           "layers": layers, "ring_bytes": layers * per, "max_abs_diff_vs_single": round(diff, 5)}
                    runs = {name: [] for name in variants}
                    for r in range(rounds + 1):  # the first round warms up clocks and code objects
                        for name, fn in variants.items():
                            us = timed(fn)
                            if r:
                                runs[name].append(us)
                    for name, v in runs.items():
                        med = statistics.median(v)
                        row[f"{name}_us"] = round(med, 2)
                        row[f"{name}_spread"] = round((max(v) - min(v)) / med, 3)
                    margin = max(v for k, v in row.items() if k.endswith("_spread"))
                    row["spread"] = margin
                    row["best"] = min((k for k in runs if k.startswith("cfg")), key=lambda k: row[f"{k}_us"])
                    row["gsx_over_best"] = round(row["gsx_us"] / row[row["best"] + "_us"], 3)
                    row["single_over_gsx"] = round(row["single_us"] / row["gsx_us"], 2)
                    row["gsx_beats_single"] = row["gsx_us"] * (1 + margin) < row["single_us"]
                    out.append(row)
                    print(json.dumps(row), file=sys.stderr, flush=True)
                    del q, o, q1, o1, ws, ws1
            del kv, table
            torch.cuda.empty_cache()
    s.destroy()
    return out


KV_APPEND_SHAPES = [(8, 2048), (64, 512), (1, 16384)]  # (sequences, new tokens each): prefill chunks of 16384 tokens
KV_APPEND_DECODE = (8, 64, 256)  # sequences of a decode step (T = 1)


def kv_append(shapes=KV_APPEND_SHAPES, heads=ATTN_HEADS, kinds=("bf16", "fp8"), ring_bytes=(1 << 30) + 1, reps=3,
              rounds=3, page=16, decode=KV_APPEND_DECODE, decode_iters=200):
    """RoPE + KV append.  Prefill-sized: ``b`` sequences of ``t`` new tokens from length 0 into a ring of per-layer
    paged caches of more than 1 GiB, pages of 16 tokens handed out through a random permutation, a real cos / sin
    table; one timing is ``reps`` passes over the ring between two events, reported as the median TB/s of ``rounds``
    repeats (and their spread) of the bytes read (QKV rows and cos / sin rows) plus the bytes written (Q_out and the
    cache rows).  ``memtest_rewrite_TBps`` is the yardstick: ``gsx_memtest_check`` with ``rewrite``, which reads and
    writes every byte of a buffer of half the pass's byte total, so both directions count as they do for the kernel;
    as in :func:`attn_decode` it is ONE call timed by the host's clock, report read-back included, so it reads low by
    the fixed host cost of a call and the comparison favours the kernel.  Decode-sized (``T = 1``): microseconds per
    call over ``decode_iters`` back-to-back calls on one layer."""
    out = []
    s = hip.Stream(0)
    ts = torch.cuda.ExternalStream(s.ptr)
    d = 128
    for kind in kinds:
        kdt = torch.bfloat16 if kind == "bf16" else torch.float8_e4m3fn
        esz = 2 if kind == "bf16" else 1
        for hq, hkv in heads:
            rows = hq + 2 * hkv
            for b, t in [*shapes, *((n, 1) for n in decode)]:
                tokens = b * t
                per_seq = -(-t // page)
                pages = b * per_seq
                cache = 2 * pages * hkv * page * d * esz  # K and V of one layer
                layers = max(2, -(-ring_bytes // cache)) if t > 1 else 2
                moved = tokens * (rows * d * 2 + 2 * (d // 2) * 4 + hq * d * 2 + 2 * hkv * d * esz)
                kc = torch.zeros(layers, pages, hkv, page, d, device="cuda", dtype=torch.uint8 if esz == 1 else kdt)
                vc = torch.zeros_like(kc)
                table = torch.randperm(pages, device="cuda").to(torch.int32).view(b, per_seq).contiguous()
                lens = torch.zeros(b, device="cuda", dtype=torch.int32)
                qkv = torch.randn(tokens, rows * d, device="cuda", dtype=torch.bfloat16)
                qo = torch.empty(tokens, hq, d, device="cuda", dtype=torch.bfloat16)
                ang = (torch.arange(t, device="cuda", dtype=torch.float64)[:, None]
                       * 10000.0 ** (-torch.arange(d // 2, device="cuda", dtype=torch.float64) / (d // 2))[None])
                cos, sin = ang.cos().float().contiguous(), ang.sin().float().contiguous()
                lb = kc[0].numel() * kc.element_size()
                torch.cuda.synchronize()

                def args(i):
                    return (s, kind, qkv.data_ptr(), rows * d, qo.data_ptr(), kc.data_ptr() + i * lb,
                            vc.data_ptr() + i * lb, table.data_ptr(), lens.data_ptr(), 0, cos.data_ptr(),
                            sin.data_ptr(), t, b, t, hq, hkv, d, page, pages, per_seq, t)

                row = {"kind": kind, "b": b, "t": t, "heads": hq, "kv_heads": hkv, "page": page, "layers": layers,
                       "bytes_per_call": moved}
                if t == 1:
                    us = []
                    for r in range(rounds + 1):
                        ms = hip.time_kv_append(*args(r % layers), decode_iters)
                        if r:
                            us.append(ms * 1e3 / decode_iters)
                    row["gsx_us_per_call"] = round(statistics.median(us), 2)
                    row["gsx_spread"] = round((max(us) - min(us)) / statistics.median(us), 3)
                else:
                    yard = hip.DeviceBuffer(0, (layers * moved // 2) & ~255)
                    hip.memtest_write(s, yard.addr(), yard.nbytes, 0, MEMTEST_RANDOM, 1)
                    s.sync()
                    flipped = [False]

                    def ours():
                        for i in range(layers):
                            hip.kv_append(*args(i))

                    def timed(fn):
                        torch.cuda.synchronize()
                        with torch.cuda.stream(ts):
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record(ts)
                            for _ in range(reps):
                                fn()
                            e1.record(ts)
                        e1.synchronize()
                        return reps * layers * moved / (e0.elapsed_time(e1) * 1e-3) / 1e12

                    def yardstick():  # every call leaves the complement of what it found
                        s.sync()
                        t0 = time.perf_counter()
                        rep = hip.memtest_check(s, yard.addr(), yard.nbytes, 0, MEMTEST_RANDOM, 1, flipped[0], True)
                        dt = time.perf_counter() - t0
                        flipped[0] = not flipped[0]
                        assert rep.bad_dwords == 0
                        return 2 * yard.nbytes / dt / 1e12

                    runs = {"gsx": [], "memtest_rewrite": []}
                    for r in range(rounds + 1):  # the first round warms up clocks and code objects
                        for name, fn in (("gsx", lambda: timed(ours)), ("memtest_rewrite", yardstick)):
                            v = fn()
                            if r:
                                runs[name].append(v)
                    for name, v in runs.items():
                        med = statistics.median(v)
                        row[f"{name}_TBps"] = round(med, 3)
                        row[f"{name}_spread"] = round((max(v) - min(v)) / med, 3)
                    yard.free()
                out.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
                del kc, vc, table, lens, qkv, qo, cos, sin
                torch.cuda.empty_cache()
    s.destroy()
    return out


NORM_ACT_PREFILL = [("add_rmsnorm", 4096, 8192), ("add_rmsnorm", 16384, 8192), ("silu_mul", 4096, 28672)]
NORM_ACT_DECODE = (1, 4, 16)  # rows of a decode step, at the same widths


def norm_act(shapes=NORM_ACT_PREFILL, kinds=("bf16", "fp8"), ring_bytes=(512 << 20) + 1, reps=3, rounds=3,
             decode=NORM_ACT_DECODE, decode_iters=200):
    """Fused add + RMSNorm (X, R_in, R_out in place, Y) and SwiGLU, to bf16 and to e4m3 with a scale per row.
    Prefill-sized: thousands of rows over a ring of operand sets of more than 512 MiB, twice the Infinity Cache; one
    timing is ``reps`` passes over the ring between two events, reported as the median TB/s of ``rounds`` repeats (and
    their spread) of the bytes read plus the bytes written.  ``memtest_rewrite_TBps`` is the yardstick as in
    :func:`kv_append`: ``gsx_memtest_check`` with ``rewrite`` over half the pass's byte total, ONE call timed by the
    host's clock, so it reads low by the fixed host cost of a call.  Decode-sized (M = 1, 4, 16): microseconds per call
    over ``decode_iters`` back-to-back calls."""
    out = []
    s = hip.Stream(0)
    ts = torch.cuda.ExternalStream(s.ptr)
    widths = sorted({(op, n) for op, _, n in shapes})
    for kind in kinds:
        esz = 2 if kind == "bf16" else 1
        for op, m, n in [*shapes, *((op, m, n) for op, n in widths for m in decode)]:
            small = m <= max(decode)
            if op == "add_rmsnorm":
                moved = m * n * (2 + 2 + 2 + esz) + n * 2  # X, R_in, R_out, Y and W
            else:
                moved = m * n * (4 + esz)  # gate and up, Y
            moved += m * 4 if esz == 1 else 0
            slots = 2 if small else max(2, -(-ring_bytes // moved))
            src = torch.randn(slots, m, 2 * n if op == "silu_mul" else n, device="cuda", dtype=torch.bfloat16)
            res = torch.randn(slots, m, n, device="cuda", dtype=torch.bfloat16) if op == "add_rmsnorm" else None
            w = torch.ones(n, device="cuda", dtype=torch.bfloat16)
            y = torch.empty(slots, m, n * esz, device="cuda", dtype=torch.uint8)
            sc = torch.empty(slots, m, device="cuda", dtype=torch.float32)
            torch.cuda.synchronize()

            def args(i):
                scale = sc[i].data_ptr() if esz == 1 else 0
                if op == "add_rmsnorm":
                    return (s, kind, src[i].data_ptr(), n, res[i].data_ptr(), res[i].data_ptr(), n, w.data_ptr(),
                            y[i].data_ptr(), n, scale, m, n, 1e-5)
                return (s, kind, src[i].data_ptr(), 2 * n, y[i].data_ptr(), n, scale, m, n)

            call, timer = ((hip.add_rmsnorm, hip.time_add_rmsnorm) if op == "add_rmsnorm"
                           else (hip.silu_mul, hip.time_silu_mul))
            row = {"op": op, "kind": kind, "m": m, "n": n, "slots": slots, "bytes_per_call": moved}
            if small:
                us = []
                for r in range(rounds + 1):
                    ms = timer(*args(r % slots), decode_iters)
                    if r:
                        us.append(ms * 1e3 / decode_iters)
                row["gsx_us_per_call"] = round(statistics.median(us), 2)
                row["gsx_spread"] = round((max(us) - min(us)) / statistics.median(us), 3)
            else:
                yard = hip.DeviceBuffer(0, (slots * moved // 2) & ~255)
                hip.memtest_write(s, yard.addr(), yard.nbytes, 0, MEMTEST_RANDOM, 1)
                s.sync()
                flipped = [False]

                def ours():
                    for i in range(slots):
                        call(*args(i))

                def timed(fn):
                    torch.cuda.synchronize()
                    with torch.cuda.stream(ts):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(ts)
                        for _ in range(reps):
                            fn()
                        e1.record(ts)
                    e1.synchronize()
                    return reps * slots * moved / (e0.elapsed_time(e1) * 1e-3) / 1e12

                def yardstick():  # every call leaves the complement of what it found
                    s.sync()
                    t0 = time.perf_counter()
                    rep = hip.memtest_check(s, yard.addr(), yard.nbytes, 0, MEMTEST_RANDOM, 1, flipped[0], True)
                    dt = time.perf_counter() - t0
                    flipped[0] = not flipped[0]
                    assert rep.bad_dwords == 0
                    return 2 * yard.nbytes / dt / 1e12

                runs = {"gsx": [], "memtest_rewrite": []}
                for r in range(rounds + 1):  # the first round warms up clocks and code objects
                    for name, fn in (("gsx", lambda: timed(ours)), ("memtest_rewrite", yardstick)):
                        v = fn()
                        if r:
                            runs[name].append(v)
                for name, v in runs.items():
                    med = statistics.median(v)
                    row[f"{name}_TBps"] = round(med, 3)
                    row[f"{name}_spread"] = round((max(v) - min(v)) / med, 3)
                row["gsx_over_memtest_rewrite"] = round(row["gsx_TBps"] / row["memtest_rewrite_TBps"], 3)
                yard.free()
            out.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            del src, res, y, sc
            torch.cuda.empty_cache()
    s.destroy()
    return out


ATTN_PREFILL_SHAPES = [(16, 2048, 0), (4, 8192, 0), (8, 2048, 6144)]  # (sequences, new tokens each, tokens before them)


def attn_prefill(shapes=ATTN_PREFILL_SHAPES, heads=((64, 8),), kinds=("bf16", "fp8"), iters=5, rounds=3, page=16):
    """The causal prefill attention: ``b`` sequences of ``t`` new tokens behind ``base`` tokens, random normal Q, K and
    V, pages of 16 tokens handed out through a random permutation.  TFLOP/s over visible pairs only
    (``4 * D * Hq * sum of (pos + 1)``), the median of ``rounds`` timings of ``iters`` back-to-back calls (and their
    spread).  The yardstick, for the bf16 cache and ``base == 0``: ``scaled_dot_product_attention(is_causal=True,
    enable_gqa=True)`` on a contiguous bf16 copy of the same data, in the same run, counted with the same FLOPs."""
    out = []
    s = hip.Stream(0)
    d = 128
    sdpa = torch.nn.functional.scaled_dot_product_attention
    for kind in kinds:
        kdt = torch.bfloat16 if kind == "bf16" else torch.float8_e4m3fn
        for hq, hkv in heads:
            for b, t, base in shapes:
                n = base + t
                per_seq = -(-n // page)
                pages = b * per_seq
                flops = 4.0 * d * hq * b * (t * base + t * (t + 1) // 2)
                k = torch.randn(b, hkv, per_seq * page, d, device="cuda", dtype=torch.bfloat16)
                v = torch.randn(b, hkv, per_seq * page, d, device="cuda", dtype=torch.bfloat16)
                q = torch.randn(b * t, hq, d, device="cuda", dtype=torch.bfloat16)
                o = torch.empty_like(q)
                table = torch.randperm(pages, device="cuda").to(torch.int32).view(b, per_seq).contiguous()
                kc = torch.empty(pages, hkv, page, d, device="cuda", dtype=kdt)
                vc = torch.empty_like(kc)
                for src, dst in ((k, kc), (v, vc)):  # token j of sequence i lies at page table[i][j / page]
                    paged = src.view(b, hkv, per_seq, page, d).permute(0, 2, 1, 3, 4).reshape(pages, hkv, page, d)
                    dst[table.view(-1).long()] = paged.to(kdt)
                lens = torch.full((b,), base, device="cuda", dtype=torch.int32)
                torch.cuda.synchronize()
                args = (s, kind, q.data_ptr(), kc.data_ptr(), vc.data_ptr(), table.data_ptr(), lens.data_ptr(),
                        o.data_ptr(), b, t, hq, hkv, d, page, pages, per_seq, n, d ** -0.5)
                row = {"kind": kind, "b": b, "t": t, "base": base, "heads": hq, "kv_heads": hkv, "page": page,
                       "flops_per_call": flops}
                runs = {"gsx": []}
                for r in range(rounds + 1):  # the first round warms up clocks and code objects
                    ms = hip.time_prefill_attn(*args, iters)
                    if r:
                        runs["gsx"].append(iters * flops / (ms * 1e-3) / 1e12)
                if kind == "bf16" and base == 0:
                    q4 = q.view(b, t, hq, d).transpose(1, 2)  # [B][Hq][T][D], a view
                    kk, vv = k[:, :, :n], v[:, :, :n]
                    ref = sdpa(q4, kk, vv, is_causal=True, enable_gqa=True, scale=d ** -0.5)
                    s.sync()
                    row["max_abs_diff_vs_sdpa"] = float((ref.transpose(1, 2).reshape(b * t, hq, d).float()
                                                         - o.float()).abs().max())
                    runs["sdpa"] = []
                    for r in range(rounds + 1):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        torch.cuda.synchronize()
                        e0.record()
                        for _ in range(iters):
                            sdpa(q4, kk, vv, is_causal=True, enable_gqa=True, scale=d ** -0.5)
                        e1.record()
                        e1.synchronize()
                        if r:
                            runs["sdpa"].append(iters * flops / (e0.elapsed_time(e1) * 1e-3) / 1e12)
                    del ref
                for name, vals in runs.items():
                    med = statistics.median(vals)
                    row[f"{name}_TFLOPs"] = round(med, 1)
                    row[f"{name}_spread"] = round((max(vals) - min(vals)) / med, 3)
                if "sdpa" in runs:
                    row["gsx_over_sdpa"] = round(row["gsx_TFLOPs"] / row["sdpa_TFLOPs"], 3)
                out.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
                del k, v, q, o, kc, vc, table, lens
                torch.cuda.empty_cache()
    s.destroy()
    return out


SAMPLE_VOCABS = (128256, 262144)
SAMPLE_ROWS = (1, 8, 16, 256)


def sample(vocabs=SAMPLE_VOCABS, rows=SAMPLE_ROWS, hidden=8192, iters=50, gemm_iters=5, rounds=3, gather_rows=65536):
    """The sampler against torch on the same logits, interleaved, the median of ``rounds`` timings (the first round
    warms up) of ``iters`` back-to-back calls, in microseconds per call.  Greedy: ``torch.argmax``.  Sampling at
    T 0.8, k 50, p 0.95: ``topk`` -> softmax -> cumulative-sum cut -> ``multinomial`` -> gather, which is what a server
    in eager torch runs.  With M <= 16 the logits are what ``gsx_decode_gemm_nt`` (N = V, K = ``hidden``) wrote from
    random normal operands, and that call is timed too: ``sampler_share`` is the sampler's part of LM head plus
    sampler.  With M = 256 they are random normal.  The logits of one case (at most 134 MB) stay in the Infinity Cache
    between calls, as they are after the LM head has written them.  Then ``gsx_embed_gather`` of ``gather_rows``
    random rows of a [V][hidden] table (bytes read plus written) against ``gsx_hbm_fill`` over the bytes written."""
    out = []
    s = hip.Stream(0)
    ts = torch.cuda.ExternalStream(s.ptr)

    def torch_us(fn):
        torch.cuda.synchronize()
        with torch.cuda.stream(ts):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            for _ in range(iters):
                fn()
            e1.record(ts)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    for v in vocabs:
        w = torch.empty(v, hidden, device="cuda", dtype=torch.bfloat16)
        for lo in range(0, v, 16384):
            w[lo:lo + 16384].copy_(torch.randn(min(16384, v - lo), hidden, device="cuda") / hidden ** 0.5)
        for m in rows:
            row = {"v": v, "m": m}
            if m <= 16:
                x = torch.randn(m, hidden, device="cuda", dtype=torch.bfloat16)
                logits = torch.empty(m, v, device="cuda", dtype=torch.bfloat16)
                torch.cuda.synchronize()
                gargs = (s, "bf16", x.data_ptr(), w.data_ptr(), logits.data_ptr(), m, v, hidden)
                hip.decode_gemm_nt(*gargs)
                s.sync()
            else:
                logits = torch.randn(m, v, device="cuda", dtype=torch.bfloat16)
            temp = torch.full((m,), 0.8, device="cuda")
            topk = torch.full((m,), 50, device="cuda", dtype=torch.int32)
            topp = torch.full((m,), 0.95, device="cuda")
            seeds = torch.arange(m, device="cuda", dtype=torch.int64) + 1
            tok = torch.empty(m, device="cuda", dtype=torch.int32)
            torch.cuda.synchronize()

            def torch_sample():
                vals, idx = torch.topk(logits.float() / 0.8, 50, dim=-1)
                probs = torch.softmax(vals, -1)
                before = torch.cumsum(probs, -1) - probs
                probs = probs.masked_fill(before >= 0.95, 0.0)
                return idx.gather(-1, torch.multinomial(probs, 1))

            modes = {"greedy": ((s, logits.data_ptr(), v, 0, 0, 0, 0, 0, tok.data_ptr(), m, v),
                                lambda: torch.argmax(logits, -1)),
                     "k50_p95": ((s, logits.data_ptr(), v, temp.data_ptr(), topk.data_ptr(), topp.data_ptr(),
                                  seeds.data_ptr(), 0, tok.data_ptr(), m, v), torch_sample)}
            runs = {f"{mode}_{who}": [] for mode in modes for who in ("gsx", "torch")}
            if m <= 16:
                runs["lm_head"] = []
            for r in range(rounds + 1):
                for mode, (args, ref) in modes.items():
                    a, b = hip.time_sample(*args, iters) * 1e3 / iters, torch_us(ref)
                    if r:
                        runs[f"{mode}_gsx"].append(a)
                        runs[f"{mode}_torch"].append(b)
                if m <= 16:
                    g = hip.time_decode_gemm(*gargs, gemm_iters) * 1e3 / gemm_iters
                    if r:
                        runs["lm_head"].append(g)
            for name, vals in runs.items():
                med = statistics.median(vals)
                row[f"{name}_us"] = round(med, 2)
                row[f"{name}_spread"] = round((max(vals) - min(vals)) / med, 3)
            for mode in modes:
                row[f"{mode}_torch_over_gsx"] = round(row[f"{mode}_torch_us"] / row[f"{mode}_gsx_us"], 2)
                if m <= 16:
                    row[f"{mode}_sampler_share"] = round(row[f"{mode}_gsx_us"]
                                                         / (row[f"{mode}_gsx_us"] + row["lm_head_us"]), 4)
            out.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            del logits, temp, topk, topp, seeds, tok
        # the gather, with the table of this vocabulary
        ids = torch.randint(0, v, (gather_rows,), device="cuda", dtype=torch.int32)
        dst = torch.empty(gather_rows, hidden, device="cuda", dtype=torch.bfloat16)
        nbytes = gather_rows * hidden * 2
        torch.cuda.synchronize()
        eargs = (s, w.data_ptr(), hidden, ids.data_ptr(), dst.data_ptr(), hidden)
        runs = {"gather": [], "fill": [], "gather_16_us": []}
        for r in range(rounds + 1):
            ms = hip.time_embed_gather(*eargs, gather_rows, hidden, v, 5)
            s.sync()
            t0 = time.perf_counter()
            for _ in range(5):
                hip.hbm_fill(s, dst.data_ptr(), nbytes, r)
            s.sync()
            dt = time.perf_counter() - t0
            small = hip.time_embed_gather(*eargs, 16, hidden, v, iters)
            if r:
                runs["gather"].append(5 * 2 * nbytes / (ms * 1e-3) / 1e12)
                runs["fill"].append(5 * nbytes / dt / 1e12)
                runs["gather_16_us"].append(small * 1e3 / iters)
        row = {"v": v, "op": "embed_gather", "rows": gather_rows, "h": hidden, "bytes_written": nbytes,
               "gather_TBps_read_plus_written": round(statistics.median(runs["gather"]), 3),
               "hbm_fill_TBps_written": round(statistics.median(runs["fill"]), 3),
               "gather_16_rows_us": round(statistics.median(runs["gather_16_us"]), 2)}
        out.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del w, ids, dst
        torch.cuda.empty_cache()
    s.destroy()
    return out


MOE_SHAPES = [(2048, 768, 128, 8), (4096, 14336, 8, 2), (7168, 2048, 256, 8)]  # (hidden, ffn, experts, topk)


def moe(shapes=MOE_SHAPES, ms=(1, 8, 16), kinds=("bf16", "fp8", "mxfp4"), ring_bytes=(2 << 30) + 1, reps=3, rounds=3):
    """The MoE decode kernels by the protocol of :func:`gemm_decode`: rings of expert tensors of more than 2 GiB for
    the up projection ``[E][2 ffn][hidden]`` and for the down projection ``[E][hidden][ffn]``, ``reps`` passes over a
    ring between two events, the median of ``rounds`` repeats after a warm-up and their spread, the variants
    interleaved in one process.  Routing comes from random router weights and inputs through ``moe_route`` and is the
    same for every layer of the ring; ``n_active`` is recorded.  Per row and projection, TB/s over the ACTIVE experts'
    weight and scale bytes for every grouped configuration, the dispatching entry point (``gsx``), one plain
    ``decode_gemm_nt`` per active expert with the routing known in advance and the rows gathered beforehand
    (``per_expert``: what the library offered before, without the host synchronisation it would need), and
    ``gsx_memtest_check`` over the same number of bytes.  ``route_us`` and ``combine_us`` are per call; ``mlp_us`` is
    the whole bf16 MoE MLP of one layer (route, up, SwiGLU, down, combine) over the ring."""
    out = []
    s = hip.Stream(0)
    ts = torch.cuda.ExternalStream(s.ptr)
    unit = {"bf16": 2.0, "fp8": 1.0, "mxfp4": 0.5 + 1 / 32}
    wdt = {"bf16": torch.bfloat16, "fp8": torch.float8_e4m3fn, "mxfp4": torch.uint8}

    def operand(kind, rows, k):
        """``(tensor, scales or None)``: random normal bf16 / e4m3, or bf16 quantised to MXFP4 by the library."""
        x = torch.randn(rows, k, device="cuda", dtype=torch.bfloat16)
        if kind != "mxfp4":
            return x.to(wdt[kind]), None
        q = torch.empty(rows, k // 2, device="cuda", dtype=torch.uint8)
        sc = torch.empty(rows, k // 32, device="cuda", dtype=torch.uint8)
        torch.cuda.synchronize()
        hip.quant_mxfp4(s, x.data_ptr(), q.data_ptr(), sc.data_ptr(), rows, k)
        s.sync()
        return q, sc

    for hidden, ffn, e, topk in shapes:
        gen = torch.Generator(device="cuda").manual_seed(hidden + e)
        rw = torch.randn(e, hidden, device="cuda", generator=gen) / math.sqrt(hidden)
        for kind in kinds:
            if (kind == "mxfp4" and (hidden % 256 or ffn % 256)) or (kind == "fp8" and (hidden % 128 or ffn % 128)):
                continue
            proj = {"up": (2 * ffn, hidden), "down": (hidden, ffn)}  # name: (N, K)
            ring = {}
            for name, (n, k) in proj.items():
                per = int(e * n * k * unit[kind])
                layers = max(2, -(-ring_bytes // per))
                wcols = k // 2 if kind == "mxfp4" else k
                w = torch.empty(layers, e * n, wcols, device="cuda", dtype=wdt[kind])
                ws = torch.empty(layers, e * n, k // 32, device="cuda", dtype=torch.uint8) if kind == "mxfp4" else None
                for i in range(layers):
                    for x0 in range(e):  # an expert at a time: nothing larger is held in bf16
                        t, sc = operand(kind, n, k)
                        w[i, x0 * n:(x0 + 1) * n].copy_(t)
                        if ws is not None:
                            ws[i, x0 * n:(x0 + 1) * n].copy_(sc)
                ring[name] = (w, ws, layers, per // e)
            for m in ms:
                pairs = m * topk
                xin = torch.randn(m, hidden, device="cuda", generator=gen)
                logits = (xin @ rw.t()).bfloat16().contiguous()
                ids = torch.empty(pairs, device="cuda", dtype=torch.int32)
                tw = torch.empty(pairs, device="cuda", dtype=torch.float32)
                plan = torch.empty(hip.MOE_PLAN_INTS, device="cuda", dtype=torch.int32)
                torch.cuda.synchronize()
                hip.moe_route(s, logits.data_ptr(), e, ids.data_ptr(), tw.data_ptr(), plan.data_ptr(), m, e, topk)
                s.sync()
                ph = plan.cpu().numpy()
                n_active = int(ph[0])
                row = {"kind": kind, "hidden": hidden, "ffn": ffn, "experts": e, "topk": topk, "m": m,
                       "n_active": n_active, "empty_slots": min(e, pairs) - n_active}
                row["route_us"] = round(hip.time_moe_route(s, logits.data_ptr(), e, ids.data_ptr(), tw.data_ptr(),
                                                           plan.data_ptr(), m, e, topk, 50) / 50 * 1e3, 2)
                yb = torch.randn(pairs, hidden, device="cuda", dtype=torch.bfloat16)
                ob = torch.empty(m, hidden, device="cuda", dtype=torch.bfloat16)
                torch.cuda.synchronize()
                row["combine_us"] = round(hip.time_moe_combine(s, yb.data_ptr(), hidden, tw.data_ptr(), ob.data_ptr(),
                                                               hidden, m, topk, hidden, 50) / 50 * 1e3, 2)
                for name, (n, k) in proj.items():
                    w, ws, layers, xbytes = ring[name]
                    a_div = topk if name == "up" else 1
                    a, sa = operand(kind, -(-pairs // a_div), k)
                    c = torch.empty(pairs, n, device="cuda", dtype=torch.bfloat16)
                    wb, sbb = w[0].numel() * w.element_size(), (ws[0].numel() if ws is not None else 0)
                    xw, xs = wb // e, sbb // e  # bytes of one expert's matrix and scales
                    slots = []
                    for sl in range(n_active):  # the per-expert loop's operands, gathered beforehand
                        x0, b0, cnt = int(ph[4 + sl]), int(ph[4 + 128 + sl]), int(ph[4 + 256 + sl])
                        src = torch.from_numpy(ph[4 + 384 + b0:4 + 384 + b0 + cnt] // a_div).cuda().long()
                        slots.append((x0, cnt, a[src].contiguous(), None if sa is None else sa[src].contiguous(),
                                      torch.empty(cnt, n, device="cuda", dtype=torch.bfloat16)))
                    torch.cuda.synchronize()
                    sap = 0 if sa is None else sa.data_ptr()

                    def grouped(cfg):
                        for i in range(layers):
                            args = (s, kind, a.data_ptr(), a_div, w.data_ptr() + i * wb, c.data_ptr(), plan.data_ptr(),
                                    m, topk, e, n, k)
                            scales = (sap, ws.data_ptr() + i * sbb if ws is not None else 0)
                            if cfg is None:
                                hip.moe_gemm_nt(*args, *scales)
                            else:
                                hip.moe_gemm_nt_cfg(*args, cfg, *scales)

                    def per_expert():
                        for i in range(layers):
                            for x0, cnt, ga, gsa, gc_ in slots:
                                hip.decode_gemm_nt(s, kind, ga.data_ptr(), w.data_ptr() + i * wb + x0 * xw,
                                                   gc_.data_ptr(), cnt, n, k, 0 if gsa is None else gsa.data_ptr(),
                                                   ws.data_ptr() + i * sbb + x0 * xs if ws is not None else 0)

                    variants = {f"cfg{cfg}_{cn}": (lambda cfg=cfg: grouped(cfg))
                                for cfg, (cn, bn, *_) in hip.moe_gemm_cfgs().items() if n % bn == 0}
                    variants["gsx"] = lambda: grouped(None)
                    variants["per_expert"] = per_expert
                    moved = layers * n_active * xbytes
                    yard = hip.DeviceBuffer(0, moved & ~255)
                    hip.memtest_write(s, yard.addr(), yard.nbytes, 0, MEMTEST_RANDOM, 1)
                    s.sync()

                    def timed(fn):
                        torch.cuda.synchronize()
                        with torch.cuda.stream(ts):
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record(ts)
                            for _ in range(reps):
                                fn()
                            e1.record(ts)
                        e1.synchronize()
                        return reps * moved / (e0.elapsed_time(e1) * 1e-3) / 1e12

                    def yardstick():
                        s.sync()
                        t0 = time.perf_counter()
                        rep = hip.memtest_check(s, yard.addr(), yard.nbytes, 0, MEMTEST_RANDOM, 1)
                        dt = time.perf_counter() - t0
                        assert rep.bad_dwords == 0
                        return yard.nbytes / dt / 1e12

                    runs = {v: [] for v in [*variants, "memtest_check"]}
                    for r in range(rounds + 1):  # the first round warms up clocks and code objects
                        for v, fn in variants.items():
                            t = timed(fn)
                            if r:
                                runs[v].append(t)
                        t = yardstick()
                        if r:
                            runs["memtest_check"].append(t)
                    yard.free()
                    row[f"{name}_layers"], row[f"{name}_active_bytes"] = layers, moved
                    for v, ts_ in runs.items():
                        med = statistics.median(ts_)
                        row[f"{name}_{v}_TBps"] = round(med, 3)
                        row[f"{name}_{v}_spread"] = round((max(ts_) - min(ts_)) / med, 3)
                    del slots, a, sa, c
                if kind == "bf16":  # the whole MLP of a layer, over the rings
                    (wu, _, lu, _), (wd, _, ld, _) = ring["up"], ring["down"]
                    xa = xin.bfloat16().contiguous()
                    gu = torch.empty(pairs, 2 * ffn, device="cuda", dtype=torch.bfloat16)
                    act = torch.empty(pairs, ffn, device="cuda", dtype=torch.bfloat16)
                    torch.cuda.synchronize()
                    ub, db, n_l = wu[0].numel() * 2, wd[0].numel() * 2, min(lu, ld)

                    def mlp():
                        for i in range(n_l):
                            hip.moe_route(s, logits.data_ptr(), e, ids.data_ptr(), tw.data_ptr(), plan.data_ptr(), m, e,
                                          topk)
                            hip.moe_gemm_nt(s, "bf16", xa.data_ptr(), topk, wu.data_ptr() + i * ub, gu.data_ptr(),
                                            plan.data_ptr(), m, topk, e, 2 * ffn, hidden)
                            hip.silu_mul(s, "bf16", gu.data_ptr(), 2 * ffn, act.data_ptr(), ffn, 0, pairs, ffn)
                            hip.moe_gemm_nt(s, "bf16", act.data_ptr(), 1, wd.data_ptr() + i * db, yb.data_ptr(),
                                            plan.data_ptr(), m, topk, e, hidden, ffn)
                            hip.moe_combine(s, yb.data_ptr(), hidden, tw.data_ptr(), ob.data_ptr(), hidden, m, topk,
                                            hidden)

                    us = []
                    for r in range(rounds + 1):
                        torch.cuda.synchronize()
                        with torch.cuda.stream(ts):
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record(ts)
                            for _ in range(reps):
                                mlp()
                            e1.record(ts)
                        e1.synchronize()
                        if r:
                            us.append(e0.elapsed_time(e1) * 1e3 / (reps * n_l))
                    row["mlp_us"] = round(statistics.median(us), 2)
                    row["mlp_spread"] = round((max(us) - min(us)) / statistics.median(us), 3)
                out.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
            del ring
            torch.cuda.empty_cache()
    s.destroy()
    return out


def moe_fp8_block(shapes=MOE_SHAPES, ms=(1, 8, 16), ring_bytes=(2 << 30) + 1, reps=3, rounds=3):
    """The block-scaled fp8 grouped expert GEMM by the protocol of :func:`moe`: rings of more than 2 GiB of e4m3 experts
    for both projections, the routing of ``moe_route`` on random logits, the variants interleaved in one process, the
    median of ``rounds`` repeats after a warm-up and their spread.  TB/s is over the ACTIVE experts' e4m3 bytes for
    every variant, whatever it reads: every configuration, the dispatching entry point (``gsx``), and three yardsticks:
    ``fp8_row``, ``gsx_moe_gemm_nt`` with per-row scales on the same bytes (the same traffic without the fold);
    ``bf16``, ``gsx_moe_gemm_nt`` on a bf16 ring of the same shapes (twice the bytes: the library's only route to such
    experts before); ``per_expert``, one ``gsx_skinny_gemm_fp8_block_nt`` per hit expert on rows gathered beforehand,
    the hit set known to the host in advance, neither of which is timed."""
    out = []
    s = hip.Stream(0)
    ts = torch.cuda.ExternalStream(s.ptr)
    f8 = torch.float8_e4m3fn
    for hidden, ffn, e, topk in shapes:
        if hidden % 128 or ffn % 128:
            continue
        gen = torch.Generator(device="cuda").manual_seed(hidden + e)
        rw = torch.randn(e, hidden, device="cuda", generator=gen) / math.sqrt(hidden)
        ring = {}
        for name, (n, k) in {"up": (2 * ffn, hidden), "down": (hidden, ffn)}.items():
            layers, nb, g = max(2, -(-ring_bytes // (e * n * k))), -(-n // 128), k // 128
            w = torch.empty(layers, e * n, k, device="cuda", dtype=f8)
            wb = torch.empty(layers, e * n, k, device="cuda", dtype=torch.bfloat16)
            for i in range(layers):
                for x0 in range(e):  # an expert at a time
                    t = torch.randn(n, k, device="cuda", dtype=torch.bfloat16)
                    w[i, x0 * n:(x0 + 1) * n].copy_(t.to(f8))
                    wb[i, x0 * n:(x0 + 1) * n].copy_(t)
            sb = torch.rand(layers, e, nb, g, device="cuda") + 0.5
            sbr = torch.rand(layers, e * n, device="cuda") + 0.5
            ring[name] = (n, k, layers, w, wb, sb, sbr)
        for m in ms:
            pairs = m * topk
            logits = (torch.randn(m, hidden, device="cuda", generator=gen) @ rw.t()).bfloat16().contiguous()
            ids = torch.empty(pairs, device="cuda", dtype=torch.int32)
            tw = torch.empty(pairs, device="cuda", dtype=torch.float32)
            plan = torch.empty(hip.MOE_PLAN_INTS, device="cuda", dtype=torch.int32)
            torch.cuda.synchronize()
            hip.moe_route(s, logits.data_ptr(), e, ids.data_ptr(), tw.data_ptr(), plan.data_ptr(), m, e, topk)
            s.sync()
            ph = plan.cpu().numpy()
            n_active = int(ph[0])
            row = {"hidden": hidden, "ffn": ffn, "experts": e, "topk": topk, "m": m, "n_active": n_active}
            for name, (n, k, layers, w, wb, sb, sbr) in ring.items():
                a_div, g = (topk if name == "up" else 1), k // 128
                rows = -(-pairs // a_div)
                x = torch.randn(rows, k, device="cuda", dtype=torch.bfloat16)
                a, sa = torch.empty(rows, k, device="cuda", dtype=f8), torch.empty(rows, g, device="cuda")
                sar = torch.rand(rows, device="cuda") + 0.5
                c = torch.empty(pairs, n, device="cuda", dtype=torch.bfloat16)
                torch.cuda.synchronize()
                hip.quant_fp8_block(s, x.data_ptr(), k, a.data_ptr(), k, sa.data_ptr(), g, rows, k)
                s.sync()
                slots = []
                for sl in range(n_active):  # the per-expert loop's operands, gathered beforehand
                    x0, b0, cnt = int(ph[4 + sl]), int(ph[4 + 128 + sl]), int(ph[4 + 256 + sl])
                    src = torch.from_numpy(ph[4 + 384 + b0:4 + 384 + b0 + cnt] // a_div).cuda().long()
                    slots.append((x0, cnt, a[src].contiguous(), sa[src].contiguous(),
                                  torch.empty(cnt, n, device="cuda", dtype=torch.bfloat16)))
                part = torch.empty(max(16, max(hip.skinny_gemm_fp8_block_workspace_bytes(cnt, n, k)
                                               for _, cnt, *_ in slots)), device="cuda", dtype=torch.uint8)
                torch.cuda.synchronize()
                wbytes, sbytes = e * n * k, sb[0].numel() * 4

                def grouped(cfg):
                    for i in range(layers):
                        args = (s, a.data_ptr(), a_div, w.data_ptr() + i * wbytes, c.data_ptr(), plan.data_ptr(), m,
                                topk, e, n, k)
                        tail = (sa.data_ptr(), g, sb.data_ptr() + i * sbytes)
                        if cfg is None:
                            hip.moe_gemm_fp8_block_nt(*args, *tail)
                        else:
                            hip.moe_gemm_fp8_block_nt_cfg(*args, cfg, *tail)

                def fp8_row():
                    for i in range(layers):
                        hip.moe_gemm_nt(s, "fp8", a.data_ptr(), a_div, w.data_ptr() + i * wbytes, c.data_ptr(),
                                        plan.data_ptr(), m, topk, e, n, k, sar.data_ptr(),
                                        sbr.data_ptr() + i * e * n * 4, hip.SCALE_ROW)

                def bf16():
                    for i in range(layers):
                        hip.moe_gemm_nt(s, "bf16", x.data_ptr(), a_div, wb.data_ptr() + i * 2 * wbytes, c.data_ptr(),
                                        plan.data_ptr(), m, topk, e, n, k)

                def per_expert():
                    for i in range(layers):
                        for x0, cnt, ga, gsa, gc_ in slots:
                            hip.skinny_gemm_fp8_block_nt(s, ga.data_ptr(), w.data_ptr() + i * wbytes + x0 * n * k,
                                                         gc_.data_ptr(), cnt, n, k, gsa.data_ptr(), g,
                                                         sb.data_ptr() + i * sbytes + x0 * (sbytes // e),
                                                         part.data_ptr(), part.numel())

                variants = {f"cfg{cfg}_{cn}": (lambda cfg=cfg: grouped(cfg))
                            for cfg, (cn, *_) in hip.moe_gemm_fp8_block_cfgs().items()}
                variants.update({"gsx": lambda: grouped(None), "fp8_row": fp8_row, "bf16": bf16,
                                 "per_expert": per_expert})
                moved = layers * n_active * n * k

                def timed(fn):
                    torch.cuda.synchronize()
                    with torch.cuda.stream(ts):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(ts)
                        for _ in range(reps):
                            fn()
                        e1.record(ts)
                    e1.synchronize()
                    return reps * moved / (e0.elapsed_time(e1) * 1e-3) / 1e12

                runs = {v: [] for v in variants}
                for r in range(rounds + 1):  # the first round warms up clocks and code objects
                    for v, fn in variants.items():
                        t = timed(fn)
                        if r:
                            runs[v].append(t)
                row[f"{name}_layers"], row[f"{name}_active_bytes"] = layers, moved
                for v, ts_ in runs.items():
                    med = statistics.median(ts_)
                    row[f"{name}_{v}_TBps"] = round(med, 3)
                    row[f"{name}_{v}_spread"] = round((max(ts_) - min(ts_)) / med, 3)
                del slots, a, sa, c, x
            out.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        del ring
        torch.cuda.empty_cache()
    s.destroy()
    return out


def _windows(ts, call, window_ms):
    """``(iters, one)``: ``one(iters)`` times a window of ``iters`` calls by the events of the stream ``ts`` and gives
    the milliseconds per call; ``iters`` fills ``window_ms``, from a first window of 3 calls."""
    def one(iters):
        with torch.cuda.stream(ts):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            for _ in range(iters):
                call()
            e1.record(ts)
        e1.synchronize()
        return e0.elapsed_time(e1) / iters
    iters = max(5, min(500, int(window_ms / max(one(3), 1e-3))))
    return iters, one


def moe_prefill(shapes=((2048, 768, 128, 8), (4096, 14336, 8, 2)), ms=(1024, 8192), rounds=3, window_ms=30.0):
    """The MoE prefill kernels.  Routing comes from random router weights and inputs through ``moe_prefill_route`` and
    ``moe_prefill_plan``.  Per shape, ``m`` and projection the grouped 128x128 GEMM is timed against the dense
    ``128x128/4w`` configuration at ``128 * n_tiles`` rows with the same N and K (the same MFMA work without the gather
    and the row-scattered stores; its B is one expert's matrix, so it reads fewer weights), the two interleaved in one
    process: the median of ``rounds`` windows of about ``window_ms`` each after a warm-up, and their spread.
    ``tflops_real`` counts the P real pairs, ``tflops_padded`` the padded rows; ``route_us``, ``plan_us`` and
    ``combine_us`` are per call."""
    out = []
    s = hip.Stream(0)
    ts = torch.cuda.ExternalStream(s.ptr)
    dense = {name: i for i, name in hip.gemm_cfgs().items()}["128x128/4w"]

    def windows(call):
        return _windows(ts, call, window_ms)

    for hidden, ffn, e, topk in shapes:
        gen = torch.Generator(device="cuda").manual_seed(hidden + e)
        rw = torch.randn(e, hidden, device="cuda", generator=gen) / math.sqrt(hidden)
        proj = {"up": (2 * ffn, hidden), "down": (hidden, ffn)}  # name: (N, K)
        w = {}
        for name, (n, k) in proj.items():
            w[name] = torch.empty(e * n, k, device="cuda", dtype=torch.bfloat16)
            for x0 in range(e):  # an expert at a time: nothing larger is held in fp32
                w[name][x0 * n:(x0 + 1) * n].copy_(torch.randn(n, k, device="cuda", generator=gen) / math.sqrt(k))
        for m in ms:
            pairs = m * topk
            xin = torch.randn(m, hidden, device="cuda", generator=gen)
            logits = (xin @ rw.t()).bfloat16().contiguous()
            ids = torch.empty(pairs, device="cuda", dtype=torch.int32)
            tw = torch.empty(pairs, device="cuda", dtype=torch.float32)
            plan = torch.empty(hip.moe_prefill_plan_ints(m, topk, e), device="cuda", dtype=torch.int32)
            wsb = hip.moe_prefill_workspace_bytes(m, topk, e)
            ws = torch.empty(wsb // 4, device="cuda", dtype=torch.int32)
            torch.cuda.synchronize()
            route = (s, logits.data_ptr(), e, ids.data_ptr(), tw.data_ptr(), m, e, topk)
            mkplan = (s, ids.data_ptr(), plan.data_ptr(), m, topk, e, ws.data_ptr(), wsb)
            hip.moe_prefill_route(*route)
            hip.moe_prefill_plan(*mkplan)
            s.sync()
            n_tiles = int(plan[0].item())
            base = {"hidden": hidden, "ffn": ffn, "experts": e, "topk": topk, "m": m, "pairs": pairs,
                    "n_tiles": n_tiles, "pad_share": round(1 - pairs / (128 * n_tiles), 4),
                    "route_us": round(hip.time_moe_prefill_route(*route, 50) / 50 * 1e3, 2),
                    "plan_us": round(hip.time_moe_prefill_plan(*mkplan, 50) / 50 * 1e3, 2)}
            yb = torch.randn(pairs, hidden, device="cuda", dtype=torch.bfloat16)
            ob = torch.empty(m, hidden, device="cuda", dtype=torch.bfloat16)
            torch.cuda.synchronize()
            base["combine_us"] = round(hip.time_moe_prefill_combine(s, yb.data_ptr(), hidden, tw.data_ptr(),
                                                                    ob.data_ptr(), hidden, m, topk, hidden, 50) / 50 * 1e3, 2)
            del yb, ob
            for name, (n, k) in proj.items():
                a_div = topk if name == "up" else 1
                a = torch.randn(pairs // a_div, k, device="cuda", dtype=torch.bfloat16)
                c = torch.empty(pairs, n, device="cuda", dtype=torch.bfloat16)
                mp = 128 * n_tiles
                da = torch.randn(mp, k, device="cuda", dtype=torch.bfloat16)
                dc = torch.empty(mp, n, device="cuda", dtype=torch.bfloat16)
                torch.cuda.synchronize()
                calls = {"grouped": lambda: hip.moe_prefill_gemm_nt(s, a.data_ptr(), a_div, w[name].data_ptr(),
                                                                    c.data_ptr(), plan.data_ptr(), m, topk, e, n, k),
                         "dense": lambda: hip.gemm_bf16_nt_cfg(s, da.data_ptr(), w[name].data_ptr(), dc.data_ptr(), mp,
                                                               n, k, dense)}
                timers = {v: windows(call) for v, call in calls.items()}  # this is the warm-up too
                got = {v: [] for v in calls}
                for _ in range(rounds):
                    for v, (iters, one) in timers.items():  # interleaved
                        got[v].append(one(iters))
                med = {v: statistics.median(t) for v, t in got.items()}
                row = {**base, "proj": name, "n": n, "k": k}
                for v in calls:
                    row[f"{v}_ms"] = round(med[v], 4)
                    row[f"{v}_spread"] = round((max(got[v]) - min(got[v])) / med[v], 4)
                row["grouped_over_dense"] = round(med["grouped"] / med["dense"], 4)
                row["tflops_real"] = round(2.0 * pairs * n * k / med["grouped"] / 1e9, 1)
                row["tflops_padded"] = round(2.0 * mp * n * k / med["grouped"] / 1e9, 1)
                row["dense_tflops"] = round(2.0 * mp * n * k / med["dense"] / 1e9, 1)
                out.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
                del a, c, da, dc
            torch.cuda.empty_cache()
        del w
        torch.cuda.empty_cache()
    s.destroy()
    return out


def moe_prefill_fp8_block(shapes=((2048, 768, 128, 8), (4096, 14336, 8, 2), (7168, 2048, 256, 8)), ms=(1024, 8192),
                          rounds=3, window_ms=30.0):
    """The block-scaled fp8 grouped GEMM of MoE prefill, on :func:`moe_prefill`'s shapes and DeepSeek-V3's expert shape,
    both projections, routing from ``moe_prefill_route`` and ``moe_prefill_plan``.  Three calls on the same routing,
    interleaved in one process, the median of ``rounds`` windows of about ``window_ms`` after a warm-up and their
    spread (max - min over the median):
    ``fp8``, the new entry point; ``bf16``, ``gsx_moe_prefill_gemm_nt`` on the dequantised operands, the path there was
    before; ``per_expert``, one ``gsx_gemm_fp8_block_nt`` per expert on rows gathered and padded to 128 beforehand (the
    gather is not timed and the host knows the plan), what the tile reaches without a gather.  TFLOP/s count the P real
    pairs.  ``beats_bf16`` holds only where the fp8 median is below the bf16 median by more than the two ranges
    (max - min) together."""
    out = []
    s = hip.Stream(0)
    ts = torch.cuda.ExternalStream(s.ptr)
    f8, bf = torch.float8_e4m3fn, torch.bfloat16
    for hidden, ffn, e, topk in shapes:
        gen = torch.Generator(device="cuda").manual_seed(hidden + e)
        rw = torch.randn(e, hidden, device="cuda", generator=gen) / math.sqrt(hidden)
        plans = {}
        for m in ms:  # the routings, once per shape
            pairs = m * topk
            logits = (torch.randn(m, hidden, device="cuda", generator=gen) @ rw.t()).bfloat16().contiguous()
            ids = torch.empty(pairs, device="cuda", dtype=torch.int32)
            tw = torch.empty(pairs, device="cuda", dtype=torch.float32)
            plan = torch.empty(hip.moe_prefill_plan_ints(m, topk, e), device="cuda", dtype=torch.int32)
            wsb = hip.moe_prefill_workspace_bytes(m, topk, e)
            ws = torch.empty(wsb // 4, device="cuda", dtype=torch.int32)
            torch.cuda.synchronize()
            hip.moe_prefill_route(s, logits.data_ptr(), e, ids.data_ptr(), tw.data_ptr(), m, e, topk)
            hip.moe_prefill_plan(s, ids.data_ptr(), plan.data_ptr(), m, topk, e, ws.data_ptr(), wsb)
            s.sync()
            plans[m] = plan
        for name, (n, k) in {"up": (2 * ffn, hidden), "down": (hidden, ffn)}.items():  # a projection's experts at a time
            g = k // 128
            w = torch.empty(e * n, k, device="cuda", dtype=f8)
            wb = torch.empty(e * n, k, device="cuda", dtype=bf)
            sb = torch.empty(e, n // 128, g, device="cuda")
            for x0 in range(e):  # an expert at a time: block-quantised, and dequantised for the bf16 call
                blocks = (torch.randn(n, k, device="cuda", generator=gen) / math.sqrt(k)).view(n // 128, 128, g, 128)
                sb[x0] = blocks.abs().amax(dim=(1, 3)).clamp_min(2.0 ** -100) / 448.0
                q = (blocks / sb[x0][:, None, :, None]).clamp(-448.0, 448.0).to(f8)
                w[x0 * n:(x0 + 1) * n].copy_(q.view(n, k))
                wb[x0 * n:(x0 + 1) * n].copy_((q.float() * sb[x0][:, None, :, None]).view(n, k))
            for m in ms:
                pairs, plan = m * topk, plans[m]
                a_div = topk if name == "up" else 1
                rows = pairs // a_div
                x = torch.randn(rows, k, device="cuda", dtype=bf, generator=gen)
                a, sa = torch.empty(rows, k, device="cuda", dtype=f8), torch.empty(rows, g, device="cuda")
                c = torch.empty(pairs, n, device="cuda", dtype=bf)
                torch.cuda.synchronize()
                hip.quant_fp8_block(s, x.data_ptr(), k, a.data_ptr(), k, sa.data_ptr(), g, rows, k)
                s.sync()
                xb = (a.float().view(rows, g, 128) * sa[:, :, None]).view(rows, k).to(bf)
                ph = plan.cpu()
                n_tiles = int(ph[0])
                t_max = (len(ph) - 4) // 129
                tile_expert, prow = ph[4:4 + n_tiles], ph[4 + t_max:4 + t_max + 128 * n_tiles].view(n_tiles, 128)
                per = []  # (expert, padded rows, gathered A, gathered scale_a, C) of every expert with a tile
                for x0 in tile_expert.unique().tolist():
                    src = (prow[tile_expert == x0].reshape(-1).clamp_min(0) // a_div).cuda().long()
                    per.append((x0, len(src), a.view(torch.uint8)[src].view(f8), sa[src].contiguous(),
                                torch.empty(len(src), n, device="cuda", dtype=bf)))
                torch.cuda.synchronize()

                def per_expert():
                    for x0, r, ga, gsa, gc_ in per:
                        hip.gemm_fp8_block_nt(s, ga.data_ptr(), w.data_ptr() + x0 * n * k, gc_.data_ptr(), r, n, k,
                                              gsa.data_ptr(), g, sb.data_ptr() + x0 * (n // 128) * g * 4)

                calls = {"fp8": lambda: hip.moe_prefill_gemm_fp8_block_nt(s, a.data_ptr(), a_div, w.data_ptr(),
                                                                          c.data_ptr(), plan.data_ptr(), m, topk, e, n,
                                                                          k, sa.data_ptr(), g, sb.data_ptr()),
                         "bf16": lambda: hip.moe_prefill_gemm_nt(s, xb.data_ptr(), a_div, wb.data_ptr(), c.data_ptr(),
                                                                 plan.data_ptr(), m, topk, e, n, k),
                         "per_expert": per_expert}
                timers = {v: _windows(ts, call, window_ms) for v, call in calls.items()}  # this is the warm-up too
                got = {v: [] for v in calls}
                for _ in range(rounds):
                    for v, (iters, one) in timers.items():  # interleaved
                        got[v].append(one(iters))
                med = {v: statistics.median(t) for v, t in got.items()}
                rng = {v: max(t) - min(t) for v, t in got.items()}
                row = {"hidden": hidden, "ffn": ffn, "experts": e, "topk": topk, "m": m, "pairs": pairs, "proj": name,
                       "n": n, "k": k, "n_tiles": n_tiles, "pad_share": round(1 - pairs / (128 * n_tiles), 4)}
                for v in calls:
                    row[f"{v}_ms"] = round(med[v], 4)
                    row[f"{v}_spread"] = round(rng[v] / med[v], 4)
                    row[f"{v}_tflops_real"] = round(2.0 * pairs * n * k / med[v] / 1e9, 1)
                row["fp8_over_bf16_speedup"] = round(med["bf16"] / med["fp8"], 3)
                row["fp8_over_per_expert_time"] = round(med["fp8"] / med["per_expert"], 3)
                row["beats_bf16"] = bool(med["bf16"] - med["fp8"] > rng["bf16"] + rng["fp8"])
                out.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
                del a, sa, c, x, xb, per
                torch.cuda.empty_cache()
            del w, wb, sb
            torch.cuda.empty_cache()
    s.destroy()
    return out


def hbm(nbytes=16 << 30, reps=5):
    s = hip.Stream(0)
    buf = hip.DeviceBuffer(0, nbytes)
    hip.hbm_fill(s, buf.addr(), nbytes, 1)
    s.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        hip.hbm_fill(s, buf.addr(), nbytes, 2)
    s.sync()
    fill = reps * nbytes / (time.perf_counter() - t0) / 1e12
    gib64 = 64 << 30
    big = hip.DeviceBuffer(0, gib64)
    t0 = time.perf_counter()
    hip.hbm_stamp(s, big.addr(), gib64, 1 << 20, 42)
    s.sync()
    stamp_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    bad = hip.hbm_verify(s, big.addr(), gib64, 1 << 20, 42)
    verify_ms = (time.perf_counter() - t0) * 1e3
    buf.free()
    big.free()
    s.destroy()
    return {"fill_TBps": round(fill, 2), "stamp_64GiB_ms": round(stamp_ms, 3), "verify_64GiB_ms": round(verify_ms, 3),
            "bad": bad}


if __name__ == "__main__":
    sizes = [(4096, 4096, 4096), (8192, 8192, 8192), (2048, 8192, 4096), (16384, 16384, 8192)]
    fp8_sizes = [(4096, 4096, 4096), (8192, 8192, 8192), (16384, 16384, 8192)]
    sections = {"gemm_bf16_nt": lambda: gemm(sizes), "gemm_fp8_nt": lambda: gemm_fp8(fp8_sizes),
                "gemm_fp8_block": gemm_fp8_block, "gemm_mxfp4_nt": lambda: gemm_mxfp4(fp8_sizes), "gemm_decode": gemm_decode, "gemm_skinny": gemm_skinny,
                "gemm_skinny_fp8_block": gemm_skinny_fp8_block,
                "attn_decode": attn_decode, "attn_multi": attn_multi, "attn_mla": attn_mla, "attn_mla_multi": attn_mla_multi,
                "kv_append": kv_append, "norm_act": norm_act, "attn_prefill": attn_prefill, "sample": sample,
                # short single sequences, where attn_pick()'s cap of 4 tiles per wave decides the split count
                "attn_decode_short": lambda: attn_decode(shapes=[(1, 8192), (1, 4096)], heads=[(64, 8)]),
                "moe": moe, "moe_128": lambda: moe(shapes=MOE_SHAPES[:1]),  # the 128-expert shape alone
                "moe_prefill": moe_prefill, "moe_fp8_block": moe_fp8_block,
                "moe_prefill_fp8_block": moe_prefill_fp8_block,
                "hbm": hbm}
    only = sys.argv[2].split(",") if len(sys.argv) > 2 else list(sections)  # [out.json [section,section..]]
    res = {name: sections[name]() for name in only}
    print(json.dumps(res))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)
