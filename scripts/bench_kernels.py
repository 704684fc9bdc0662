#!/usr/bin/env python3
"""Micro-benchmarks of the HIP kernels on one MI355X: bf16, fp8 and mxfp4 GEMM (ours vs torch/hipBLASLt), the decode
GEMM (every configuration vs torch and a read-bandwidth yardstick), the decode attention over a paged KV cache (every
configuration and split count vs torch SDPA and the same yardstick), RoPE + KV append and the fused add + RMSNorm and
SwiGLU (vs a read-and-rewrite yardstick), the causal prefill attention over the paged cache (vs torch SDPA on a
contiguous copy), the sampler, the MoE router, grouped expert GEMM and combine (vs one plain decode GEMM per active
expert and the read yardstick), HBM fill, stamp/verify."""
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


ATTN_SHAPES = [(1, 32768), (8, 8192), (64, 2048), (256, 1024)]  # (sequences, tokens each)
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
                "gemm_mxfp4_nt": lambda: gemm_mxfp4(fp8_sizes), "gemm_decode": gemm_decode, "attn_decode": attn_decode,
                "kv_append": kv_append, "norm_act": norm_act, "attn_prefill": attn_prefill, "sample": sample,
                # short single sequences, where attn_pick()'s cap of 4 tiles per wave decides the split count
                "attn_decode_short": lambda: attn_decode(shapes=[(1, 8192), (1, 4096)], heads=[(64, 8)]),
                "moe": moe, "moe_128": lambda: moe(shapes=MOE_SHAPES[:1]),  # the 128-expert shape alone
                "hbm": hbm}
    only = sys.argv[2].split(",") if len(sys.argv) > 2 else list(sections)  # [out.json [section,section..]]
    res = {name: sections[name]() for name in only}
    print(json.dumps(res))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)
