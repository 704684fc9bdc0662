"""CU-partition isolation benchmark (BASELINE.json config 5: "4 pods co-resident on one MI355X with per-pod CU partitions").

The reference leaves isolation to the application (``docs/designs/designs.md:25-28``)
and lists "integrate Nvidia MPS" as a roadmap item (``README.md:77``).  Our
stand-in is a per-pod CU partition handed out by the device plugin.  This
harness runs the pod workload (:mod:`.workload`) as real processes with the
exact environment the device plugin's Allocate produces, in four scenarios:

* ``solo``          one pod alone on the GPU (reference throughput);
* ``shared``        4 pods co-resident, no partition (time-sliced, unisolated);
* ``partitioned``   4 pods co-resident, 64 CUs each via the stream CU mask;
* ``env``           4 pods co-resident, 64 CUs each via ``HSA_CU_MASK`` only
                    (process-wide; applies to torch's own queues too), hipBLASLt GEMM;
* ``env-gsx``       the same with the libgsx_kernels GEMM (stream mask vs process mask, same kernel);
* ``solo64``        one pod alone inside a 64-CU partition (what a partition is worth);
* ``noisy`` / ``noisy-partitioned``  pod 0 runs a small (latency-bound) GEMM
                    next to 3 pods running large GEMMs, without / with
                    partitions: pod 0's throughput relative to ``solo`` / ``solo64``
                    is the interference the partition removes;
* ``decode-noisy`` / ``decode-noisy-partitioned``  pod 0 runs the decode workload
                    (``--batch`` rows against a ring of weights: bound by HBM bandwidth,
                    which no CU mask partitions) next to 3 pods running large GEMMs;
* ``attn-noisy`` / ``attn-noisy-partitioned``  pod 0 runs the attention workload
                    (``--batch`` sequences of ``--context`` tokens over a ring of paged KV
                    caches: a gather over pages, bound by HBM bandwidth too) next to 3 pods
                    running large GEMMs;
* ``prefill-noisy`` / ``prefill-noisy-partitioned``  pod 0 runs the decode ``layer`` workload
                    (``--batch`` rows, bound by HBM bandwidth) next to ONE prefill pod
                    (``--prefill-batch`` sequences of ``--chunk`` new tokens: compute-bound), the
                    standard interference pair of an inference server.  Each pod also runs alone
                    under the same mask; the summary has ``solo_tflops`` and
                    ``ratio_to_solo`` per pod.

``--workload decode`` or ``--workload attn`` makes every pod of the other scenarios such a pod.  ``--workload server``
(a whole decode layer per ring layer: projections, RoPE and KV append, attention) does so for ``solo``, ``solo64``,
``shared`` and ``partitioned``; it runs on the library's kernels only.  ``--workload layer`` (the same with a residual
stream, two RMSNorms and the SwiGLU MLP of ``--ffn`` columns: a whole decoder layer) takes the same scenarios, and so
does ``--workload prefill`` (that layer on ``--batch`` sequences of ``--chunk`` new tokens each).
Reported per scenario: per-pod TFLOP/s, aggregate, and fairness (min/max); for
decode and attention pods also the TB/s of weight or KV bytes they streamed.
Run: ``python -m gsxtools.isolation --seconds 8``.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

from gpushare_scheduler_extender_amd.deviceplugin.allocator import CUPartitioner, build_response
from gpushare_scheduler_extender_amd.deviceplugin.devices import Device
from gpushare_scheduler_extender_amd.k8s.objects import make_pod
from gpushare_scheduler_extender_amd.models.profile import SHARED_GPU

from . import workload as pod_workload

ROOT = Path(__file__).resolve().parents[1]


def pod_envs(n_pods: int, cus_each: int, gpu_total_gib: int, pod_gib: int, with_mask: bool) -> list[dict]:
    dev = Device(index=0, total_bytes=gpu_total_gib << 30)
    part = CUPartitioner(dev.cu_count, dev.xcc_count)
    envs = []
    for i in range(n_pods):
        pod = make_pod(f"iso-{i}", pod_gib, annotations={SHARED_GPU.annotation_idx: "0",
                                                         SHARED_GPU.annotation_dev: str(gpu_total_gib)})
        cus = part.allocate(f"iso-{i}", cus_each) if with_mask else None
        envs.append(build_response(pod, dev, pod_gib, SHARED_GPU, mount_mode="all", cus=cus).envs)
    return envs


def run_pods(envs: list[dict], seconds: float, kernel: str, size, mask_mode: str,
             dtype: str = "bf16", workload="gemm", batch: int = 8, attn_args: list[str] | None = None) -> list[dict]:
    """``size``, ``workload`` and ``batch`` are one value for every pod or a list with one per pod; ``attn_args`` are
    the command-line options an attention pod gets (a list of lists: one per pod)."""
    start_at = time.time() + 20.0  # time for every process to import torch and warm up
    procs = []
    sizes = size if isinstance(size, list) else [size] * len(envs)
    workloads = workload if isinstance(workload, list) else [workload] * len(envs)
    batches = batch if isinstance(batch, list) else [batch] * len(envs)
    per_pod = attn_args if attn_args and isinstance(attn_args[0], list) else [attn_args] * len(envs)
    for e, sz, wl, batch, attn_args in zip(envs, sizes, workloads, batches, per_pod):
        env = dict(os.environ)
        env.update({k: v for k, v in e.items() if k not in ("GSX_CU_MASK", "HSA_CU_MASK")})
        if mask_mode in ("stream", "both") and "GSX_CU_MASK" in e:
            env["GSX_CU_MASK"] = e["GSX_CU_MASK"]
        if mask_mode in ("env", "both") and "HSA_CU_MASK" in e:
            env["HSA_CU_MASK"] = e["HSA_CU_MASK"]
        env["HIP_VISIBLE_DEVICES"] = "0"
        env["ROCR_VISIBLE_DEVICES"] = "0"
        env["GSX_START_AT"] = str(start_at)
        env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
        cmd = [sys.executable, "-m", "gsxtools.workload", "--total",
               e["SHARED_GPU_MEM_DEV"], "--allocated", e["SHARED_GPU_MEM_CONTAINER"], "--kernel", kernel,
               "--size", str(sz), "--seconds", str(seconds), "--dtype", dtype, "--json"]
        if wl != "gemm":  # the default is left off the command line
            cmd += ["--workload", wl, "--batch", str(batch)]
        if wl in ("attn", "server", "layer", "prefill", "generate"):
            cmd += attn_args or []
        procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                                      cwd=str(ROOT)))
    out = []
    for p in procs:
        so, se = p.communicate(timeout=seconds + 180)
        if p.returncode != 0:
            raise RuntimeError(f"workload failed rc={p.returncode}: {se[-2000:]}")
        out.append(json.loads(so.strip().splitlines()[-1]))
    return out


def summarize(name: str, res: list[dict]) -> dict:
    t = [r["tflops"] for r in res]
    out = {"scenario": name, "pods": len(t), "per_pod_tflops": [round(x, 1) for x in t],
           "aggregate_tflops": round(sum(t), 1), "fairness_min_over_max": round(min(t) / max(t), 3) if t else None}
    if any("tbps" in r for r in res):  # decode pods: the weight bytes they streamed; None for a GEMM pod
        b = [r.get("tbps") for r in res]
        out["per_pod_tbps"] = [None if x is None else round(x, 3) for x in b]
        out["aggregate_tbps"] = round(sum(x for x in b if x is not None), 3)
    return out


SCENARIOS_DECODE_NOISY = ("decode-noisy", "decode-noisy-partitioned")
SCENARIOS_ATTN_NOISY = ("attn-noisy", "attn-noisy-partitioned")
SCENARIOS_PREFILL_NOISY = ("prefill-noisy", "prefill-noisy-partitioned")
SCENARIOS = ("solo", "shared", "partitioned", "env", "env-gsx", "solo-small", "solo64", "noisy", "noisy-partitioned",
             *SCENARIOS_DECODE_NOISY, *SCENARIOS_ATTN_NOISY, *SCENARIOS_PREFILL_NOISY)


def attn_cmdline(a: argparse.Namespace) -> list[str]:
    """The attention pods' options, as the workload's command line takes them."""
    out = ["--context", str(a.context), "--heads", str(a.heads), "--kv-heads", str(a.kv_heads), "--kv-dtype",
           a.kv_dtype, "--page", str(a.page)]
    return out + (["--kv-gib", str(a.kv_gib)] if a.kv_gib is not None else [])


SCENARIOS_SERVER = ("solo", "solo64", "shared", "partitioned")


def server_cmdline(a: argparse.Namespace) -> list[str]:
    """The server pods' options: the attention's shape, and the size of the weight ring."""
    return attn_cmdline(a) + (["--weights-gib", str(a.weights_gib)] if a.weights_gib is not None else [])


SCENARIOS_LAYER = SCENARIOS_SERVER


def dense_layer_cmdline(a: argparse.Namespace) -> list[str]:
    """The server pods' options, and the MLP's width."""
    return server_cmdline(a) + (["--ffn", str(a.ffn)] if a.ffn is not None else [])


def layer_cmdline(a: argparse.Namespace) -> list[str]:
    """The layer pods' options: the server pods', the MLP's width, and its experts where ``--experts`` is set (a
    dense layer's command line is what it was)."""
    experts = getattr(a, "experts", 0)
    moe = ["--experts", str(experts), "--experts-active", str(a.experts_active)] if experts else []
    return dense_layer_cmdline(a) + moe


def generate_cmdline(a: argparse.Namespace) -> list[str]:
    """The generate pods' options: the layer pods', the vocabulary and the sampling parameters."""
    return layer_cmdline(a) + ["--vocab", str(a.vocab), "--temperature", str(a.temperature), "--top-k", str(a.top_k),
                               "--top-p", str(a.top_p), "--seed", str(a.seed)]


def prefill_cmdline(a: argparse.Namespace) -> list[str]:
    """The prefill pods' options: the dense layer pods' (a prefill pod takes no experts), and the chunk."""
    return dense_layer_cmdline(a) + ["--chunk", str(a.chunk)]


def with_solo(summary: dict, solo: list[dict]) -> dict:
    """``summary`` of pods that ran together, with what each did alone and the ratio of the two."""
    alone = [r["tflops"] for r in solo]
    summary["solo_tflops"] = [round(x, 1) for x in alone]
    summary["ratio_to_solo"] = [round(t / x, 3) if x else None for t, x in zip(summary["per_pod_tflops"], alone)]
    return summary


def build_parser() -> argparse.ArgumentParser:
    ap = pod_workload.BatchRangeParser()
    ap.add_argument("--pods", type=int, default=4)
    ap.add_argument("--cus", type=int, default=64)
    ap.add_argument("--pod-gib", type=int, default=64)
    ap.add_argument("--gpu-gib", type=int, default=287)
    ap.add_argument("--seconds", type=float, default=8.0)
    ap.add_argument("--kernel", default="gsx", choices=["gsx", "torch"])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp8", "mxfp4"],
                    help="the pods' GEMM operand type (mxfp4: with --kernel gsx only)")
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--workload", default="gemm",
                    choices=["gemm", "decode", "attn", "server", "layer", "prefill", "generate"],
                    help="what the pods run: the large GEMM, the decode workload (--batch rows against a ring of "
                         "--size x --size weights), the attention workload (--batch sequences of --context tokens), "
                         "the server workload (a decode layer per ring layer; solo, solo64, shared, partitioned), the "
                         "layer workload (a whole decoder layer per ring layer; the same scenarios), or the prefill "
                         "workload (that layer on --batch sequences of --chunk new tokens; the same scenarios), or the generate "
                         "workload (the layer workload with the embedding lookup, the LM head and the sampler: the "
                         "latency-sensitive decode pod; the same scenarios)")
    ap.add_argument("--batch", type=int, default=8, metavar="N",
                    help="the decode pods' activation rows (1..16), or the attention pods' sequences (1..256, with "
                         "--workload attn)")
    pod_workload.add_attn_arguments(ap)
    pod_workload.add_generate_arguments(ap)
    pod_workload.add_moe_arguments(ap)
    ap.add_argument("--weights-gib", type=float, default=None,
                    help="--workload server and layer: size of the pods' weight ring (default: the workload's)")
    ap.add_argument("--ffn", type=int, default=None,
                    help="--workload layer: width of the pods' MLP (default: the workload's)")
    ap.add_argument("--prefill-batch", type=int, default=1,
                    help="prefill-noisy scenarios: the prefill pod's sequences (of --chunk new tokens each)")
    ap.add_argument("--small-size", type=int, default=2048)
    ap.add_argument("--scenarios",
                    default="solo,shared,partitioned,env,env-gsx,solo-small,solo64,noisy,noisy-partitioned")
    ap.add_argument("--json-out", default="")
    return ap


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    results = []
    own_size = a.workload in ("decode", "attn", "server", "layer", "prefill", "generate")  # pods whose work --size does not scale
    pod_args = {"server": server_cmdline, "layer": layer_cmdline, "prefill": prefill_cmdline,
                "generate": generate_cmdline}.get(a.workload, attn_cmdline)(a)

    def run(*args):  # every scenario's pods get the attention options: only attention, server and layer pods use them
        return run_pods(*args, attn_args=pod_args)

    for sc in a.scenarios.split(","):
        if sc not in SCENARIOS:
            raise SystemExit(f"unknown scenario {sc}")
        if a.workload in ("server", "layer", "prefill", "generate") and sc not in SCENARIOS_SERVER:
            raise SystemExit(f"--workload {a.workload}: scenario {sc} is not one of {', '.join(SCENARIOS_SERVER)}")
        if sc == "solo":
            envs = pod_envs(1, a.cus, a.gpu_gib, a.pod_gib, False)
            res = run(envs, a.seconds, a.kernel, a.size, "none", a.dtype, a.workload, a.batch)
        elif sc == "shared":
            envs = pod_envs(a.pods, a.cus, a.gpu_gib, a.pod_gib, False)
            res = run(envs, a.seconds, a.kernel, a.size, "none", a.dtype, a.workload, a.batch)
        elif sc == "partitioned":
            envs = pod_envs(a.pods, a.cus, a.gpu_gib, a.pod_gib, True)
            res = run(envs, a.seconds, a.kernel, a.size, "stream", a.dtype, a.workload, a.batch)
        elif sc == "solo64":
            envs = pod_envs(1, a.cus, a.gpu_gib, a.pod_gib, True)
            # what a partition is worth: to the small GEMM of `noisy`, or to a decode pod (its own size)
            res = run(envs, a.seconds, a.kernel, a.size if own_size else a.small_size, "stream",
                      a.dtype, a.workload, a.batch)
        elif sc == "solo-small":
            envs = pod_envs(1, a.cus, a.gpu_gib, a.pod_gib, False)
            res = run(envs, a.seconds, a.kernel, a.small_size, "none", a.dtype, a.workload, a.batch)
        elif sc in ("noisy", "noisy-partitioned"):
            masked = sc == "noisy-partitioned"
            envs = pod_envs(a.pods, a.cus, a.gpu_gib, a.pod_gib, masked)
            sizes = [a.small_size] + [a.size] * (a.pods - 1)
            res = run(envs, a.seconds, a.kernel, sizes, "stream" if masked else "none", a.dtype, a.workload,
                      a.batch)
        elif sc in SCENARIOS_DECODE_NOISY:
            masked = sc == "decode-noisy-partitioned"
            envs = pod_envs(a.pods, a.cus, a.gpu_gib, a.pod_gib, masked)
            res = run(envs, a.seconds, a.kernel, a.size, "stream" if masked else "none", a.dtype,
                      ["decode"] + ["gemm"] * (a.pods - 1), a.batch)
        elif sc in SCENARIOS_ATTN_NOISY:
            masked = sc == "attn-noisy-partitioned"
            envs = pod_envs(a.pods, a.cus, a.gpu_gib, a.pod_gib, masked)
            res = run(envs, a.seconds, a.kernel, a.size, "stream" if masked else "none", a.dtype,
                      ["attn"] + ["gemm"] * (a.pods - 1), a.batch)
        elif sc in SCENARIOS_PREFILL_NOISY:
            masked = sc == "prefill-noisy-partitioned"
            if why := pod_workload.prefill_refusal(a.prefill_batch, a.chunk, a.context):
                raise SystemExit(f"{sc}: {why}")
            if not 1 <= a.batch <= 16:
                raise SystemExit(f"{sc}: --batch {a.batch}: the layer pod takes 1..16 rows")
            envs = pod_envs(2, a.cus, a.gpu_gib, a.pod_gib, masked)
            wls, batches = ["layer", "prefill"], [a.batch, a.prefill_batch]
            args = [layer_cmdline(a), prefill_cmdline(a)]
            mode = "stream" if masked else "none"
            solo = [run_pods([envs[i]], a.seconds, a.kernel, a.size, mode, a.dtype, wls[i], batches[i],
                             attn_args=args[i])[0] for i in range(2)]
            res = run_pods(envs, a.seconds, a.kernel, a.size, mode, a.dtype, wls, batches, attn_args=args)
            s = with_solo(summarize(sc, res), solo)
            print(json.dumps(s), flush=True)
            results.append(s)
            continue
        elif sc == "env":
            envs = pod_envs(a.pods, a.cus, a.gpu_gib, a.pod_gib, True)
            res = run(envs, a.seconds, "torch" if a.kernel == "gsx" else a.kernel, a.size, "env", a.dtype,
                      a.workload, a.batch)
        elif sc == "env-gsx":
            envs = pod_envs(a.pods, a.cus, a.gpu_gib, a.pod_gib, True)
            res = run(envs, a.seconds, a.kernel, a.size, "env", a.dtype, a.workload, a.batch)
        else:
            raise SystemExit(f"unknown scenario {sc}")
        s = summarize(sc, res)
        print(json.dumps(s), flush=True)
        results.append(s)
    if a.json_out:
        with open(a.json_out, "w") as f:
            json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
