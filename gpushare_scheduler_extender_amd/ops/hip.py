"""ctypes binding of ``libgsx_kernels.so`` (native/kernels, C ABI in gsx_kernels.h).

No silent fallback: on a host with a GPU every call goes to the HIP code,
and a missing library raises with the command that builds it.  Callers that
must also run on CPU-only hosts check :func:`gpu_available` first.
"""
from __future__ import annotations

import ctypes
import os
import threading
from pathlib import Path

_LIB = None
_LOCK = threading.Lock()
SO = Path(__file__).resolve().parents[1] / "_native" / "libgsx_kernels.so"


class HipError(RuntimeError):
    pass


class DevInfo(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 64), ("arch", ctypes.c_char * 32), ("pci_bus_id", ctypes.c_char * 32),
                ("total_mem", ctypes.c_uint64), ("cu_count", ctypes.c_int32), ("xcc_count", ctypes.c_int32),
                ("clock_khz", ctypes.c_int32), ("wave_size", ctypes.c_int32), ("lds_per_block", ctypes.c_uint64)]


class MemtestErr(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_uint64), ("expected", ctypes.c_uint32), ("actual", ctypes.c_uint32)]


class MemtestPass(ctypes.Structure):
    _fields_ = [("pattern", ctypes.c_int), ("seed", ctypes.c_uint32), ("invert", ctypes.c_int),
                ("rewrite", ctypes.c_int), ("write", ctypes.c_int)]


class MemtestReport(ctypes.Structure):
    """``gsx_memtest_report``: checks accumulate into it; a new one is all zero."""
    _fields_ = [("bad_dwords", ctypes.c_uint64), ("flipped_or", ctypes.c_uint32), ("n_errs", ctypes.c_uint32),
                ("errs", MemtestErr * 32)]

    def errors(self) -> list[tuple[int, int, int]]:
        """The recorded ``(offset, expected, actual)`` of up to 32 bad dwords."""
        return [(e.offset, e.expected, e.actual) for e in self.errs[:self.n_errs]]


class CutestRecord(ctypes.Structure):
    """``gsx_cutest_record``: what one wave of the compute test wrote."""
    _fields_ = [("hw_id", ctypes.c_uint32), ("xcc_id", ctypes.c_uint32), ("fail_mask", ctypes.c_uint32),
                ("seed", ctypes.c_uint32), ("sig", ctypes.c_uint64 * 9)]

    def where(self) -> tuple[int, int, int, int]:
        """The physical CU ``(xcc, se, sh, cu)`` the wave ran on."""
        d = decode_hw_id(self.hw_id, self.xcc_id)
        return d["xcc"], d["se"], d["sh"], d["cu"]

    @property
    def simd(self) -> int:
        return decode_hw_id(self.hw_id, self.xcc_id)["simd"]


class CutestInject(ctypes.Structure):
    _fields_ = [("xcc", ctypes.c_int32), ("se", ctypes.c_int32), ("sh", ctypes.c_int32), ("cu", ctypes.c_int32),
                ("simd", ctypes.c_int32), ("unit", ctypes.c_int32), ("xor_mask", ctypes.c_uint32)]


class CutestCu(ctypes.Structure):
    _fields_ = [("waves", ctypes.c_uint32), ("bad_waves", ctypes.c_uint32), ("fail_mask", ctypes.c_uint16),
                ("simds", ctypes.c_uint8), ("bad_simds", ctypes.c_uint8)]


class CutestBad(ctypes.Structure):
    _fields_ = [("xcc", ctypes.c_uint8), ("se", ctypes.c_uint8), ("sh", ctypes.c_uint8), ("cu", ctypes.c_uint8),
                ("simds", ctypes.c_uint8), ("unit", ctypes.c_uint8), ("units", ctypes.c_uint16),
                ("seed", ctypes.c_uint32), ("expected", ctypes.c_uint64), ("got", ctypes.c_uint64)]


class CutestReport(ctypes.Structure):
    """``gsx_cutest_report``: launches accumulate into it; a new one is all zero."""
    _fields_ = [("waves", ctypes.c_uint64), ("bad_waves", ctypes.c_uint64), ("cus_seen", ctypes.c_uint32),
                ("simds_seen", ctypes.c_uint32), ("cus_covered", ctypes.c_uint32), ("bad_cus", ctypes.c_uint32),
                ("n_bad", ctypes.c_uint32), ("launches", ctypes.c_uint32), ("cus_expected", ctypes.c_uint32),
                ("covered", ctypes.c_uint32), ("bad", CutestBad * 16), ("cu", CutestCu * 4096)]

    def cus(self) -> dict[tuple[int, int, int, int], CutestCu]:
        """``{(xcc, se, sh, cu): entry}`` of the physical CUs that ran a wave."""
        return {slot_cu(s): c for s, c in enumerate(self.cu) if c.waves}

    def bad_entries(self) -> list[CutestBad]:
        return list(self.bad[:self.n_bad])


class Slice(ctypes.Structure):
    _fields_ = [("addr", ctypes.c_uint64), ("bytes", ctypes.c_uint64), ("tag", ctypes.c_uint64)]


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    with _LOCK:
        if _LIB is not None:
            return _LIB
        if not SO.exists():
            if os.environ.get("GSX_AUTOBUILD", "1") == "1":
                from ..utils.build import build_native  # noqa: PLC0415

                build_native(["kernels"])
            if not SO.exists():
                raise ImportError(f"{SO} missing; run `python native/build.py kernels`")
        L = ctypes.CDLL(str(SO))
        vp, u32p, u64, i32 = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64, ctypes.c_int
        # stream, kind, Q, K_cache, V_cache, block_table, seq_lens, O; B, Hq, Hkv, D, page, num_pages, table_stride,
        # max_seq_len; scale, k_scale, v_scale; workspace, workspace_bytes
        _attn_sig = [vp, i32] + [vp] * 6 + [i32] * 8 + [ctypes.c_float] * 3 + [vp, u64]
        # stream, kind, QKV, qkv_stride, Q_out, K_cache, V_cache, block_table, seq_lens, lens_out, rope_cos, rope_sin;
        # rope_len, B, T, Hq, Hkv, D, page, num_pages, table_stride, max_seq_len; k_inv_scale, v_inv_scale
        _kv_append_sig = [vp, i32, vp, ctypes.c_int64] + [vp] * 8 + [i32] * 10 + [ctypes.c_float] * 2
        # stream, kind, Q, K_cache, V_cache, block_table, seq_lens, O; B, T, Hq, Hkv, D, page, num_pages, table_stride,
        # max_seq_len; scale, k_scale, v_scale
        _prefill_sig = [vp, i32] + [vp] * 6 + [i32] * 9 + [ctypes.c_float] * 3
        # stream, out_kind, X, x_stride, R_in, R_out, r_stride, W, Y, y_stride, scale_out; M, H; eps
        _norm_sig = [vp, i32, vp, ctypes.c_int64, vp, vp, ctypes.c_int64, vp, vp, ctypes.c_int64, vp, i32, i32,
                     ctypes.c_float]
        # stream, out_kind, GU, gu_stride, Y, y_stride, scale_out; M, I
        _silu_sig = [vp, i32, vp, ctypes.c_int64, vp, ctypes.c_int64, vp, i32, i32]
        # stream, logits, logits_stride, temperature, top_k, top_p, seeds, counter, tokens_out; M, V
        _sample_sig = [vp, vp, ctypes.c_int64, vp, vp, vp, vp, u64, vp, i32, i32]
        # stream, table, table_stride, tokens, out, out_stride; M, H, V
        _embed_sig = [vp, vp, ctypes.c_int64, vp, vp, ctypes.c_int64, i32, i32, i32]
        # stream, logits, logits_stride, topk_ids, topk_w, plan; M, E, topk
        _moe_route_sig = [vp, vp, ctypes.c_int64, vp, vp, vp, i32, i32, i32]
        # stream, kind, A, a_div, B, C, plan; M, topk, E, N, K; scale_a, scale_b, scale_mode
        _moe_gemm_sig = [vp, i32, vp, i32, vp, vp, vp] + [i32] * 5 + [vp, vp, i32]
        # stream, Y, y_stride, topk_w, out, out_stride; M, topk, H
        _moe_combine_sig = [vp, vp, ctypes.c_int64, vp, vp, ctypes.c_int64, i32, i32, i32]
        sig = {
            "gsx_last_error": ([], ctypes.c_char_p),
            "gsx_device_count": ([ctypes.POINTER(i32)], i32),
            "gsx_device_info": ([i32, ctypes.POINTER(DevInfo)], i32),
            "gsx_mem_info": ([i32, ctypes.POINTER(u64), ctypes.POINTER(u64)], i32),
            "gsx_synchronize": ([i32], i32),
            "gsx_stream_create": ([i32, u32p, i32, ctypes.POINTER(vp)], i32),
            "gsx_stream_get_mask": ([vp, u32p, i32], i32),
            "gsx_stream_destroy": ([vp], i32),
            "gsx_stream_sync": ([vp], i32),
            "gsx_malloc": ([i32, u64, ctypes.POINTER(vp)], i32),
            "gsx_free": ([vp], i32),
            "gsx_memcpy_d2h": ([vp, vp, u64], i32),
            "gsx_memcpy_h2d": ([vp, vp, u64], i32),
            "gsx_cuprobe": ([vp, i32, i32, u32p], i32),
            "gsx_hbm_stamp": ([vp, vp, u64, u64, u64], i32),
            "gsx_hbm_verify": ([vp, vp, u64, u64, u64, ctypes.POINTER(u64)], i32),
            "gsx_hbm_admit_n": ([vp, ctypes.POINTER(Slice), i32, i32, i32, u64, ctypes.POINTER(u64)], i32),
            "gsx_hbm_fill": ([vp, vp, u64, ctypes.c_uint32], i32),
            "gsx_gemm_bf16_nt": ([vp, vp, vp, vp, i32, i32, i32], i32),
            "gsx_gemm_bf16_nt_launch_cfg": ([vp, vp, vp, vp, i32, i32, i32, i32], i32),
            "gsx_gemm_cfg_tile": ([i32, ctypes.POINTER(i32), ctypes.POINTER(i32)], i32),
            "gsx_gemm_cfg_name": ([i32], ctypes.c_char_p),
            "gsx_event_time_gemm": ([vp, vp, vp, vp, i32, i32, i32, i32, ctypes.POINTER(ctypes.c_float)], i32),
            "gsx_gemm_fp8_nt": ([vp, vp, vp, vp, i32, i32, i32, vp, vp, i32], i32),
            "gsx_gemm_fp8_nt_launch_cfg": ([vp, vp, vp, vp, i32, i32, i32, vp, vp, i32, i32], i32),
            "gsx_gemm_fp8_cfg_tile": ([i32, ctypes.POINTER(i32), ctypes.POINTER(i32)], i32),
            "gsx_gemm_fp8_cfg_name": ([i32], ctypes.c_char_p),
            "gsx_event_time_gemm_fp8": ([vp, vp, vp, vp, i32, i32, i32, vp, vp, i32, i32,
                                         ctypes.POINTER(ctypes.c_float)], i32),
            "gsx_gemm_mxfp4_nt": ([vp, vp, vp, vp, i32, i32, i32, vp, vp], i32),
            "gsx_gemm_mxfp4_nt_launch_cfg": ([vp, vp, vp, vp, i32, i32, i32, vp, vp, i32], i32),
            "gsx_gemm_mxfp4_cfg_tile": ([i32, ctypes.POINTER(i32), ctypes.POINTER(i32)], i32),
            "gsx_gemm_mxfp4_cfg_name": ([i32], ctypes.c_char_p),
            "gsx_event_time_gemm_mxfp4": ([vp, vp, vp, vp, i32, i32, i32, vp, vp, i32,
                                           ctypes.POINTER(ctypes.c_float)], i32),
            "gsx_quant_mxfp4": ([vp, vp, vp, vp, i32, i32], i32),
            "gsx_decode_gemm_nt": ([vp, i32, vp, vp, vp, i32, i32, i32, vp, vp, i32], i32),
            "gsx_decode_gemm_nt_launch_cfg": ([vp, i32, vp, vp, vp, i32, i32, i32, vp, vp, i32, i32], i32),
            "gsx_decode_gemm_cfg_name": ([i32], ctypes.c_char_p),
            "gsx_decode_gemm_cfg_shape": ([i32] + [ctypes.POINTER(i32)] * 3, i32),
            "gsx_event_time_decode_gemm": ([vp, i32, vp, vp, vp, i32, i32, i32, vp, vp, i32, i32,
                                            ctypes.POINTER(ctypes.c_float)], i32),
            "gsx_decode_attn": (_attn_sig, i32),
            "gsx_decode_attn_launch_cfg": ([*_attn_sig, i32, i32], i32),
            "gsx_decode_attn_workspace_bytes": ([i32] * 5 + [ctypes.POINTER(u64)], i32),
            "gsx_decode_attn_cfg_name": ([i32], ctypes.c_char_p),
            "gsx_decode_attn_cfg_shape": ([i32] + [ctypes.POINTER(i32)] * 2, i32),
            "gsx_event_time_decode_attn": ([*_attn_sig, i32, ctypes.POINTER(ctypes.c_float)], i32),
            "gsx_kv_append": (_kv_append_sig, i32),
            "gsx_event_time_kv_append": ([*_kv_append_sig, i32, ctypes.POINTER(ctypes.c_float)], i32),
            "gsx_prefill_attn": (_prefill_sig, i32),
            "gsx_prefill_attn_launch_cfg": ([*_prefill_sig, i32], i32),
            "gsx_prefill_attn_cfg_name": ([i32], ctypes.c_char_p),
            "gsx_prefill_attn_cfg_shape": ([i32] + [ctypes.POINTER(i32)] * 3, i32),
            "gsx_event_time_prefill_attn": ([*_prefill_sig, i32, ctypes.POINTER(ctypes.c_float)], i32),
            "gsx_add_rmsnorm": (_norm_sig, i32),
            "gsx_event_time_add_rmsnorm": ([*_norm_sig, i32, ctypes.POINTER(ctypes.c_float)], i32),
            "gsx_silu_mul": (_silu_sig, i32),
            "gsx_event_time_silu_mul": ([*_silu_sig, i32, ctypes.POINTER(ctypes.c_float)], i32),
            "gsx_sample": (_sample_sig, i32),
            "gsx_event_time_sample": ([*_sample_sig, i32, ctypes.POINTER(ctypes.c_float)], i32),
            "gsx_embed_gather": (_embed_sig, i32),
            "gsx_event_time_embed_gather": ([*_embed_sig, i32, ctypes.POINTER(ctypes.c_float)], i32),
            "gsx_moe_route": (_moe_route_sig, i32),
            "gsx_event_time_moe_route": ([*_moe_route_sig, i32, ctypes.POINTER(ctypes.c_float)], i32),
            "gsx_moe_gemm_nt": (_moe_gemm_sig, i32),
            "gsx_moe_gemm_nt_launch_cfg": ([*_moe_gemm_sig, i32], i32),
            "gsx_moe_gemm_cfg_name": ([i32], ctypes.c_char_p),
            "gsx_moe_gemm_cfg_shape": ([i32] + [ctypes.POINTER(i32)] * 4, i32),
            "gsx_event_time_moe_gemm": ([*_moe_gemm_sig, i32, ctypes.POINTER(ctypes.c_float)], i32),
            "gsx_moe_combine": (_moe_combine_sig, i32),
            "gsx_event_time_moe_combine": ([*_moe_combine_sig, i32, ctypes.POINTER(ctypes.c_float)], i32),
            "gsx_memtest_write": ([vp, vp, u64, u64, i32, ctypes.c_uint32, i32], i32),
            "gsx_memtest_check": ([vp, vp, u64, u64, i32, ctypes.c_uint32, i32, i32, ctypes.POINTER(MemtestReport)],
                                  i32),
            "gsx_memtest_pass": ([i32, ctypes.c_uint32, ctypes.POINTER(MemtestPass)], i32),
            "gsx_memtest_run": ([vp, vp, u64, u64, i32, ctypes.POINTER(MemtestReport),
                                 ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_double)], i32),
            "gsx_cutest_unit_name": ([i32], ctypes.c_char_p),
            "gsx_cutest_unit_shape": ([i32] + [ctypes.POINTER(i32)] * 5, i32),
            "gsx_cutest_seeds": ([i32], ctypes.c_uint32),
            "gsx_cutest_expected": ([i32, ctypes.c_uint32, ctypes.POINTER(u64)], i32),
            "gsx_cutest_launch": ([vp, ctypes.c_uint32, i32, ctypes.POINTER(CutestInject),
                                   ctypes.POINTER(CutestRecord), ctypes.c_uint32], i32),
            "gsx_cutest_aggregate": ([ctypes.POINTER(CutestRecord), ctypes.c_uint32, ctypes.POINTER(CutestReport)],
                                     i32),
            "gsx_cutest_run": ([vp, i32, ctypes.c_uint32, ctypes.POINTER(CutestReport),
                                ctypes.POINTER(ctypes.c_double)], i32),
            "gsx_cutest_stream_cus": ([vp, ctypes.POINTER(ctypes.c_uint32)], i32),
        }
        for name, (args, res) in sig.items():
            f = getattr(L, name)
            f.argtypes = args
            f.restype = res
        _LIB = L
    return _LIB


def _ck(rc: int, what: str):
    if rc != 0:
        raise HipError(f"{what}: {lib().gsx_last_error().decode(errors='replace')}")


def device_count() -> int:
    n = ctypes.c_int(0)
    rc = lib().gsx_device_count(ctypes.byref(n))
    if rc != 0:
        return 0
    return n.value


def gpu_available() -> bool:
    try:
        return device_count() > 0
    except (OSError, ImportError):
        return False


def device_info(dev: int) -> dict:
    d = DevInfo()
    _ck(lib().gsx_device_info(dev, ctypes.byref(d)), "device_info")
    return {"name": d.name.decode(), "arch": d.arch.decode(), "pci_bus_id": d.pci_bus_id.decode(),
            "total_mem": d.total_mem, "cu_count": d.cu_count, "clock_khz": d.clock_khz,
            "wave_size": d.wave_size, "lds_per_block": d.lds_per_block}


def mem_info(dev: int) -> tuple[int, int]:
    f, t = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _ck(lib().gsx_mem_info(dev, ctypes.byref(f), ctypes.byref(t)), "mem_info")
    return f.value, t.value


def synchronize(dev: int):
    _ck(lib().gsx_synchronize(dev), "synchronize")


def mask_words(cus: list[int] | range, total_cus: int = 256) -> list[int]:
    words = [0] * ((total_cus + 31) // 32)
    for c in cus:
        if not 0 <= c < total_cus:
            raise ValueError(f"CU {c} out of range 0..{total_cus - 1}")
        words[c // 32] |= 1 << (c % 32)
    return words


class Stream:
    """A HIP stream, optionally restricted to a CU mask (hipExtStreamCreateWithCUMask)."""

    def __init__(self, dev: int = 0, cu_mask: list[int] | None = None):
        self.dev = dev
        self.handle = ctypes.c_void_p()
        if cu_mask:
            arr = (ctypes.c_uint32 * len(cu_mask))(*cu_mask)
            _ck(lib().gsx_stream_create(dev, arr, len(cu_mask), ctypes.byref(self.handle)), "stream_create(cu_mask)")
        else:
            _ck(lib().gsx_stream_create(dev, None, 0, ctypes.byref(self.handle)), "stream_create")

    def mask(self, words: int = 8) -> list[int]:
        arr = (ctypes.c_uint32 * words)()
        _ck(lib().gsx_stream_get_mask(self.handle, arr, words), "stream_get_mask")
        return list(arr)

    def sync(self):
        _ck(lib().gsx_stream_sync(self.handle), "stream_sync")

    def destroy(self):
        if self.handle:
            lib().gsx_stream_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    @property
    def ptr(self) -> int:
        return self.handle.value or 0


class DeviceBuffer:
    def __init__(self, dev: int, nbytes: int):
        self.dev = dev
        self.nbytes = int(nbytes)
        self.ptr = ctypes.c_void_p()
        _ck(lib().gsx_malloc(dev, self.nbytes, ctypes.byref(self.ptr)), f"malloc({self.nbytes})")

    def free(self):
        if self.ptr:
            lib().gsx_free(self.ptr)
            self.ptr = ctypes.c_void_p()

    def addr(self, offset: int = 0) -> int:
        return (self.ptr.value or 0) + offset

    def to_host(self, nbytes: int | None = None, offset: int = 0) -> bytes:
        n = self.nbytes - offset if nbytes is None else nbytes
        buf = ctypes.create_string_buffer(n)
        _ck(lib().gsx_memcpy_d2h(buf, ctypes.c_void_p(self.addr(offset)), n), "memcpy_d2h")
        return buf.raw

    def from_host(self, data: bytes, offset: int = 0):
        _ck(lib().gsx_memcpy_h2d(ctypes.c_void_p(self.addr(offset)), data, len(data)), "memcpy_h2d")


def cuprobe(stream: Stream, blocks: int = 4096, spin: int = 20000) -> list[tuple[int, int]]:
    out = (ctypes.c_uint32 * (2 * blocks))()
    _ck(lib().gsx_cuprobe(stream.handle, blocks, spin, out), "cuprobe")
    return [(out[2 * i], out[2 * i + 1] & 0x7FFFFFFF) for i in range(blocks)]


def decode_hw_id(hw: int, xcc: int) -> dict:
    """gfx9 HW_REG_HW_ID fields (WAVE, SIMD, PIPE, CU, SH, SE, TG, VM, QUEUE, STATE, ME)."""
    return {"wave": hw & 0xF, "simd": (hw >> 4) & 0x3, "pipe": (hw >> 6) & 0x3, "cu": (hw >> 8) & 0xF,
            "sh": (hw >> 12) & 0x1, "se": (hw >> 13) & 0x7, "tg": (hw >> 16) & 0xF, "vm": (hw >> 20) & 0xF,
            "queue": (hw >> 24) & 0x7, "xcc": xcc & 0xF}


def cu_slot(xcc: int, se: int, sh: int, cu: int) -> int:
    """A physical CU's index in ``CutestReport.cu`` (native/kernels/hwid.h)."""
    return xcc << 8 | se << 5 | sh << 4 | cu


def slot_cu(slot: int) -> tuple[int, int, int, int]:
    """``(xcc, se, sh, cu)`` of a slot: the inverse of :func:`cu_slot`."""
    return slot >> 8, (slot >> 5) & 0x7, (slot >> 4) & 0x1, slot & 0xF


def physical_cus(records: list[tuple[int, int]]) -> set[tuple[int, int, int, int]]:
    out = set()
    for hw, xcc in records:
        d = decode_hw_id(hw, xcc)
        out.add((d["xcc"], d["se"], d["sh"], d["cu"]))
    return out


def hbm_stamp(stream: Stream, addr: int, nbytes: int, stride: int, tag: int):
    _ck(lib().gsx_hbm_stamp(stream.handle, ctypes.c_void_p(addr), nbytes, stride, tag & 0xFFFFFFFFFFFFFFFF),
        "hbm_stamp")


def hbm_verify(stream: Stream, addr: int, nbytes: int, stride: int, tag: int) -> int:
    bad = ctypes.c_uint64(0)
    _ck(lib().gsx_hbm_verify(stream.handle, ctypes.c_void_p(addr), nbytes, stride, tag & 0xFFFFFFFFFFFFFFFF,
                             ctypes.byref(bad)), "hbm_verify")
    return bad.value


def hbm_fill(stream: Stream, addr: int, nbytes: int, pattern: int = 0):
    _ck(lib().gsx_hbm_fill(stream.handle, ctypes.c_void_p(addr), nbytes, pattern & 0xFFFFFFFF), "hbm_fill")


def memtest_write(stream: Stream, addr: int, nbytes: int, origin: int, pattern: int, seed: int = 0,
                  invert: bool = False):
    """Store the pattern's words ``origin // 16 ...`` into ``[addr, addr + nbytes)``; not synchronised."""
    _ck(lib().gsx_memtest_write(stream.handle, ctypes.c_void_p(addr), nbytes, origin, pattern, seed & 0xFFFFFFFF,
                                int(invert)), "memtest_write")


def memtest_check(stream: Stream, addr: int, nbytes: int, origin: int, pattern: int, seed: int = 0,
                  invert: bool = False, rewrite: bool = False, report: MemtestReport | None = None) -> MemtestReport:
    """Compare every dword with the regenerated pattern, accumulating into ``report`` (a fresh one by default);
    ``rewrite`` stores the complement of the expected word in the same pass.  Synchronises the stream."""
    rep = MemtestReport() if report is None else report
    _ck(lib().gsx_memtest_check(stream.handle, ctypes.c_void_p(addr), nbytes, origin, pattern, seed & 0xFFFFFFFF,
                                int(invert), int(rewrite), ctypes.byref(rep)), "memtest_check")
    return rep


def memtest_run(stream: Stream, addr: int, nbytes: int, origin: int = 0, level: str = "quick",
                report: MemtestReport | None = None) -> tuple[MemtestReport, int, float]:
    """Run a level's pass sequence (``ops.memtest.LEVELS``): ``(report, passes, seconds)``."""
    from .memtest import LEVEL_IDS  # noqa: PLC0415

    rep = MemtestReport() if report is None else report
    passes, seconds = ctypes.c_uint32(0), ctypes.c_double(0.0)
    _ck(lib().gsx_memtest_run(stream.handle, ctypes.c_void_p(addr), nbytes, origin, LEVEL_IDS[level],
                              ctypes.byref(rep), ctypes.byref(passes), ctypes.byref(seconds)), "memtest_run")
    return rep, passes.value, seconds.value


def memtest_pass_table(level: str) -> list[tuple[str, int, int, int, int]]:
    """The native pass sequence of a level, in the form of ``ops.memtest.LEVELS``."""
    from .memtest import LEVEL_IDS  # noqa: PLC0415

    out, p = [], MemtestPass()
    while lib().gsx_memtest_pass(LEVEL_IDS[level], len(out), ctypes.byref(p)) == 0:
        out.append(("write" if p.write else "check", p.pattern, p.seed, p.invert, p.rewrite))
    return out


def cutest_expected(unit: int, seed: int) -> int:
    """The native host twin's signature of ``unit`` for ``seed`` (``ops.cutest.expected_signature``); no device call."""
    sig = ctypes.c_uint64(0)
    _ck(lib().gsx_cutest_expected(unit, seed & 0xFFFFFFFF, ctypes.byref(sig)), "cutest_expected")
    return sig.value


def cutest_unit_table() -> list[tuple]:
    """The native unit table: ``(name, m, n, k, rounds, span)`` per matrix unit, ``(name,)`` for the others."""
    out = []
    while (name := lib().gsx_cutest_unit_name(len(out))) is not None:
        v = [ctypes.c_int(0) for _ in range(5)]
        shaped = lib().gsx_cutest_unit_shape(len(out), *map(ctypes.byref, v)) == 0
        out.append((name.decode(), *(x.value for x in v)) if shaped else (name.decode(),))
    return out


def cutest_seeds(level: str) -> int:
    from .cutest import LEVEL_IDS  # noqa: PLC0415

    return lib().gsx_cutest_seeds(LEVEL_IDS[level])


def cutest_launch(stream: Stream, seed: int, blocks: int, inject: tuple | None = None):
    """One launch of the compute test: the ``4 * blocks`` waves' records (a ctypes array of :class:`CutestRecord`).
    ``inject`` is ``(xcc, se, sh, cu, simd or -1, unit, xor_mask)``.  Synchronises the stream."""
    recs = (CutestRecord * (4 * blocks))()
    inj = ctypes.byref(CutestInject(*inject)) if inject else None
    _ck(lib().gsx_cutest_launch(stream.handle, seed & 0xFFFFFFFF, blocks, inj, recs, len(recs)), "cutest_launch")
    return recs


def cutest_aggregate(records, report: CutestReport | None = None) -> CutestReport:
    """Accumulate records (a ctypes array or a list of :class:`CutestRecord`) into ``report``; pure host code."""
    rep = CutestReport() if report is None else report
    arr = records if isinstance(records, ctypes.Array) else (CutestRecord * max(1, len(records)))(*records)
    _ck(lib().gsx_cutest_aggregate(arr, len(records), ctypes.byref(rep)), "cutest_aggregate")
    return rep


def cutest_run(stream: Stream, level: str = "quick", expect_cus: int = 0,
               report: CutestReport | None = None) -> tuple[CutestReport, float]:
    """A level's launches, and more while coverage is short (``ops.cutest.SEEDS``): ``(report, seconds)``."""
    from .cutest import LEVEL_IDS  # noqa: PLC0415

    rep = CutestReport() if report is None else report
    seconds = ctypes.c_double(0.0)
    _ck(lib().gsx_cutest_run(stream.handle, LEVEL_IDS[level], expect_cus, ctypes.byref(rep), ctypes.byref(seconds)),
        "cutest_run")
    return rep, seconds.value


def gemm_bf16_nt(stream: Stream, a: int, b: int, c: int, m: int, n: int, k: int):
    _ck(lib().gsx_gemm_bf16_nt(stream.handle, ctypes.c_void_p(a), ctypes.c_void_p(b), ctypes.c_void_p(c), m, n, k),
        "gemm_bf16_nt")


def time_gemm(stream: Stream, a: int, b: int, c: int, m: int, n: int, k: int, iters: int) -> float:
    ms = ctypes.c_float(0)
    _ck(lib().gsx_event_time_gemm(stream.handle, ctypes.c_void_p(a), ctypes.c_void_p(b), ctypes.c_void_p(c),
                                  m, n, k, iters, ctypes.byref(ms)), "time_gemm")
    return ms.value


def hbm_admit_n(stream: Stream, slices: list[tuple[int, int, int]], n_stamp: int, stride: int,
                verify: bool = True) -> int:
    """Stamp the first ``n_stamp`` ``(addr, bytes, tag)`` extents, then verify all of them; one stream sync."""
    arr = (Slice * max(1, len(slices)))(*[Slice(a, b, t & 0xFFFFFFFFFFFFFFFF) for a, b, t in slices])
    bad = ctypes.c_uint64(0)
    _ck(lib().gsx_hbm_admit_n(stream.handle, arr, len(slices), n_stamp, int(verify), stride, ctypes.byref(bad)),
        "hbm_admit_n")
    return bad.value


def gemm_cfgs() -> dict[int, str]:
    """``{index: name}`` of the tile configurations, read from the library's table (native/kernels/gemm.hip)."""
    out: dict[int, str] = {}
    while (name := lib().gsx_gemm_cfg_name(len(out))) is not None:
        out[len(out)] = name.decode()
    return out


def gemm_bf16_nt_cfg(stream: Stream, a: int, b: int, c: int, m: int, n: int, k: int, cfg: int):
    """Launch one tile configuration of the GEMM; an unknown config or a shape it cannot take raises HipError."""
    _ck(lib().gsx_gemm_bf16_nt_launch_cfg(stream.handle, ctypes.c_void_p(a), ctypes.c_void_p(b), ctypes.c_void_p(c),
                                          m, n, k, cfg), f"gemm cfg {cfg}")


# ``scale_mode`` of the fp8 GEMM (gsx_kernels.h): c = bf16((acc * scale_a[row or 0]) * scale_b[col or 0])
SCALE_NONE, SCALE_TENSOR, SCALE_ROW = 0, 1, 2


def gemm_fp8_nt(stream: Stream, a: int, b: int, c: int, m: int, n: int, k: int, scale_a: int = 0, scale_b: int = 0,
                scale_mode: int = SCALE_NONE):
    """``C`` (bf16) ``= A * B^T`` on OCP e4m3 operands (``torch.float8_e4m3fn``); the scales are device addresses of
    fp32 values, one each (``SCALE_TENSOR``) or ``m`` and ``n`` of them (``SCALE_ROW``).  Not synchronised."""
    _ck(lib().gsx_gemm_fp8_nt(stream.handle, ctypes.c_void_p(a), ctypes.c_void_p(b), ctypes.c_void_p(c), m, n, k,
                              ctypes.c_void_p(scale_a), ctypes.c_void_p(scale_b), scale_mode), "gemm_fp8_nt")


def gemm_fp8_cfgs() -> dict[int, str]:
    """``{index: name}`` of the fp8 tile configurations, read from the library's table (native/kernels/gemm_fp8.hip)."""
    out: dict[int, str] = {}
    while (name := lib().gsx_gemm_fp8_cfg_name(len(out))) is not None:
        out[len(out)] = name.decode()
    return out


def gemm_fp8_nt_cfg(stream: Stream, a: int, b: int, c: int, m: int, n: int, k: int, cfg: int, scale_a: int = 0,
                    scale_b: int = 0, scale_mode: int = SCALE_NONE):
    """Launch one configuration of the fp8 GEMM; an unknown config or a shape it cannot take raises HipError."""
    _ck(lib().gsx_gemm_fp8_nt_launch_cfg(stream.handle, ctypes.c_void_p(a), ctypes.c_void_p(b), ctypes.c_void_p(c),
                                         m, n, k, ctypes.c_void_p(scale_a), ctypes.c_void_p(scale_b), scale_mode,
                                         cfg), f"gemm fp8 cfg {cfg}")


def time_gemm_fp8(stream: Stream, a: int, b: int, c: int, m: int, n: int, k: int, iters: int, scale_a: int = 0,
                  scale_b: int = 0, scale_mode: int = SCALE_NONE) -> float:
    ms = ctypes.c_float(0)
    _ck(lib().gsx_event_time_gemm_fp8(stream.handle, ctypes.c_void_p(a), ctypes.c_void_p(b), ctypes.c_void_p(c),
                                      m, n, k, ctypes.c_void_p(scale_a), ctypes.c_void_p(scale_b), scale_mode, iters,
                                      ctypes.byref(ms)), "time_gemm_fp8")
    return ms.value


def gemm_mxfp4_nt(stream: Stream, a: int, b: int, c: int, m: int, n: int, k: int, scale_a: int, scale_b: int):
    """``C`` (bf16) ``= A * B^T`` on MXFP4 operands: ``a`` and ``b`` are e2m1, two per byte
    (``torch.float4_e2m1fn_x2``, rows of ``k / 2`` bytes), ``scale_a`` and ``scale_b`` the device addresses of their
    e8m0 block scales (``torch.float8_e8m0fnu``, ``[rows][k / 32]``).  Not synchronised."""
    _ck(lib().gsx_gemm_mxfp4_nt(stream.handle, ctypes.c_void_p(a), ctypes.c_void_p(b), ctypes.c_void_p(c), m, n, k,
                                ctypes.c_void_p(scale_a), ctypes.c_void_p(scale_b)), "gemm_mxfp4_nt")


def gemm_mxfp4_cfgs() -> dict[int, str]:
    """``{index: name}`` of the mxfp4 tile configurations, read from the library's table
    (native/kernels/gemm_mxfp4.hip)."""
    out: dict[int, str] = {}
    while (name := lib().gsx_gemm_mxfp4_cfg_name(len(out))) is not None:
        out[len(out)] = name.decode()
    return out


def gemm_mxfp4_nt_cfg(stream: Stream, a: int, b: int, c: int, m: int, n: int, k: int, cfg: int, scale_a: int,
                      scale_b: int):
    """Launch one configuration of the mxfp4 GEMM; an unknown config or a shape it cannot take raises HipError."""
    _ck(lib().gsx_gemm_mxfp4_nt_launch_cfg(stream.handle, ctypes.c_void_p(a), ctypes.c_void_p(b),
                                           ctypes.c_void_p(c), m, n, k, ctypes.c_void_p(scale_a),
                                           ctypes.c_void_p(scale_b), cfg), f"gemm mxfp4 cfg {cfg}")


def time_gemm_mxfp4(stream: Stream, a: int, b: int, c: int, m: int, n: int, k: int, iters: int, scale_a: int,
                    scale_b: int) -> float:
    ms = ctypes.c_float(0)
    _ck(lib().gsx_event_time_gemm_mxfp4(stream.handle, ctypes.c_void_p(a), ctypes.c_void_p(b), ctypes.c_void_p(c),
                                        m, n, k, ctypes.c_void_p(scale_a), ctypes.c_void_p(scale_b), iters,
                                        ctypes.byref(ms)), "time_gemm_mxfp4")
    return ms.value


def quant_mxfp4(stream: Stream, x: int, q: int, s: int, rows: int, k: int):
    """Quantise bf16 ``x[rows][k]`` (``k`` a multiple of 32) to MXFP4 per OCP MX v1.0: ``q[rows][k / 2]`` e2m1 pairs
    and ``s[rows][k / 32]`` e8m0 block scales, the operand format of ``gemm_mxfp4_nt``.  Not synchronised."""
    _ck(lib().gsx_quant_mxfp4(stream.handle, ctypes.c_void_p(x), ctypes.c_void_p(q), ctypes.c_void_p(s), rows, k),
        "quant_mxfp4")


# ``kind`` of the decode GEMM (gsx_kernels.h): the operand format, each that of the GEMM family of the same name
DECODE_KINDS = {"bf16": 0, "fp8": 1, "mxfp4": 2}


def _decode_kind(kind: str) -> int:
    if kind not in DECODE_KINDS:
        raise ValueError(f"decode kind {kind!r}: one of {', '.join(DECODE_KINDS)}")
    return DECODE_KINDS[kind]


def _decode_args(stream: Stream, kind: str, a: int, b: int, c: int, m: int, n: int, k: int, scale_a: int,
                 scale_b: int, scale_mode: int) -> tuple:
    return (stream.handle, _decode_kind(kind), ctypes.c_void_p(a), ctypes.c_void_p(b), ctypes.c_void_p(c), m, n, k,
            ctypes.c_void_p(scale_a), ctypes.c_void_p(scale_b), scale_mode)


def decode_gemm_nt(stream: Stream, kind: str, a: int, b: int, c: int, m: int, n: int, k: int, scale_a: int = 0,
                   scale_b: int = 0, scale_mode: int = SCALE_NONE):
    """``C[m][n]`` (bf16) ``= A[m][k] * B[n][k]^T`` for ``1 <= m <= 16``: the decode GEMM, which streams ``b`` from
    HBM once.  ``kind`` is ``"bf16"``, ``"fp8"`` (scales and ``scale_mode`` as :func:`gemm_fp8_nt`) or ``"mxfp4"``
    (``scale_a[m][k / 32]`` and ``scale_b[n][k / 32]`` as :func:`gemm_mxfp4_nt`, ``scale_mode`` none).  Not
    synchronised."""
    _ck(lib().gsx_decode_gemm_nt(*_decode_args(stream, kind, a, b, c, m, n, k, scale_a, scale_b, scale_mode)),
        "decode_gemm_nt")


def decode_gemm_cfgs() -> dict[int, tuple[str, int, int, int]]:
    """``{index: (name, bn, waves, inflight)}`` of the decode configurations, read from the library's table
    (native/kernels/gemm_decode.hip): columns of a workgroup's strip, waves per workgroup, K-tiles a wave keeps in
    flight."""
    out: dict[int, tuple[str, int, int, int]] = {}
    while (name := lib().gsx_decode_gemm_cfg_name(len(out))) is not None:
        v = [ctypes.c_int(0) for _ in range(3)]
        if lib().gsx_decode_gemm_cfg_shape(len(out), *map(ctypes.byref, v)) != 0:
            raise HipError(f"decode cfg {len(out)} has a name and no shape")
        out[len(out)] = (name.decode(), *(x.value for x in v))
    return out


def decode_gemm_nt_cfg(stream: Stream, kind: str, a: int, b: int, c: int, m: int, n: int, k: int, cfg: int,
                       scale_a: int = 0, scale_b: int = 0, scale_mode: int = SCALE_NONE):
    """Launch one configuration of the decode GEMM; an unknown config or a shape it cannot take raises HipError."""
    _ck(lib().gsx_decode_gemm_nt_launch_cfg(*_decode_args(stream, kind, a, b, c, m, n, k, scale_a, scale_b,
                                                          scale_mode), cfg), f"decode gemm cfg {cfg}")


def time_decode_gemm(stream: Stream, kind: str, a: int, b: int, c: int, m: int, n: int, k: int, iters: int,
                     scale_a: int = 0, scale_b: int = 0, scale_mode: int = SCALE_NONE) -> float:
    ms = ctypes.c_float(0)
    _ck(lib().gsx_event_time_decode_gemm(*_decode_args(stream, kind, a, b, c, m, n, k, scale_a, scale_b, scale_mode),
                                         iters, ctypes.byref(ms)), "time_decode_gemm")
    return ms.value


# ``kind`` of the decode attention (gsx_kernels.h): the type of the paged KV cache
ATTN_KV_KINDS = {"bf16": 0, "fp8": 1}


def _attn_args(stream: Stream, kind: str, q: int, k_cache: int, v_cache: int, block_table: int, seq_lens: int, o: int,
               b: int, hq: int, hkv: int, d: int, page: int, num_pages: int, table_stride: int, max_seq_len: int,
               scale: float, k_scale: float, v_scale: float, workspace: int, workspace_bytes: int) -> tuple:
    if kind not in ATTN_KV_KINDS:
        raise ValueError(f"attention cache kind {kind!r}: one of {', '.join(ATTN_KV_KINDS)}")
    return (stream.handle, ATTN_KV_KINDS[kind], *(ctypes.c_void_p(x) for x in (q, k_cache, v_cache, block_table,
                                                                               seq_lens, o)),
            b, hq, hkv, d, page, num_pages, table_stride, max_seq_len, scale, k_scale, v_scale,
            ctypes.c_void_p(workspace), workspace_bytes)


def decode_attn(stream: Stream, kind: str, q: int, k_cache: int, v_cache: int, block_table: int, seq_lens: int,
                o: int, b: int, hq: int, hkv: int, d: int, page: int, num_pages: int, table_stride: int,
                max_seq_len: int, scale: float, k_scale: float = 1.0, v_scale: float = 1.0, workspace: int = 0,
                workspace_bytes: int = 0):
    """One decode step of grouped-query attention over a paged KV cache: ``o[b][hq][d]`` (bf16) from ``q[b][hq][d]``
    (bf16) and the caches ``[num_pages][hkv][page][d]`` of ``kind`` ``"bf16"`` or ``"fp8"`` (OCP e4m3 with the
    per-tensor factors ``k_scale`` and ``v_scale``), reached through ``block_table[b][table_stride]`` and
    ``seq_lens[b]`` (int32, device addresses).  ``workspace`` is device memory of at least
    :func:`decode_attn_workspace_bytes` bytes for the split-KV partials.  Not synchronised."""
    _ck(lib().gsx_decode_attn(*_attn_args(stream, kind, q, k_cache, v_cache, block_table, seq_lens, o, b, hq, hkv, d,
                                          page, num_pages, table_stride, max_seq_len, scale, k_scale, v_scale,
                                          workspace, workspace_bytes)), "decode_attn")


def decode_attn_workspace_bytes(b: int, hq: int, d: int, page: int, max_seq_len: int) -> int:
    """Bytes of workspace :func:`decode_attn` can need for these arguments, whatever ``hkv`` (0: none)."""
    n = ctypes.c_uint64(0)
    _ck(lib().gsx_decode_attn_workspace_bytes(b, hq, d, page, max_seq_len, ctypes.byref(n)),
        "decode_attn_workspace_bytes")
    return n.value


def decode_attn_cfgs() -> dict[int, tuple[str, int, int]]:
    """``{index: (name, waves, inflight)}`` of the attention configurations, read from the library's table
    (native/kernels/attn_decode.hip): waves per workgroup, tiles of 32 tokens a wave keeps in flight."""
    out: dict[int, tuple[str, int, int]] = {}
    while (name := lib().gsx_decode_attn_cfg_name(len(out))) is not None:
        v = [ctypes.c_int(0) for _ in range(2)]
        if lib().gsx_decode_attn_cfg_shape(len(out), *map(ctypes.byref, v)) != 0:
            raise HipError(f"attention cfg {len(out)} has a name and no shape")
        out[len(out)] = (name.decode(), *(x.value for x in v))
    return out


def decode_attn_cfg(stream: Stream, kind: str, q: int, k_cache: int, v_cache: int, block_table: int, seq_lens: int,
                    o: int, b: int, hq: int, hkv: int, d: int, page: int, num_pages: int, table_stride: int,
                    max_seq_len: int, scale: float, cfg: int, splits: int, k_scale: float = 1.0, v_scale: float = 1.0,
                    workspace: int = 0, workspace_bytes: int = 0):
    """Launch one configuration of the decode attention with ``splits`` (1..64) splits of every sequence; the
    workspace needs ``b * hq * splits * 520`` bytes when ``splits > 1``.  An unknown config raises HipError."""
    _ck(lib().gsx_decode_attn_launch_cfg(*_attn_args(stream, kind, q, k_cache, v_cache, block_table, seq_lens, o, b,
                                                     hq, hkv, d, page, num_pages, table_stride, max_seq_len, scale,
                                                     k_scale, v_scale, workspace, workspace_bytes), cfg, splits),
        f"decode attn cfg {cfg} splits {splits}")


def time_decode_attn(stream: Stream, kind: str, q: int, k_cache: int, v_cache: int, block_table: int, seq_lens: int,
                     o: int, b: int, hq: int, hkv: int, d: int, page: int, num_pages: int, table_stride: int,
                     max_seq_len: int, scale: float, iters: int, k_scale: float = 1.0, v_scale: float = 1.0,
                     workspace: int = 0, workspace_bytes: int = 0) -> float:
    ms = ctypes.c_float(0)
    _ck(lib().gsx_event_time_decode_attn(*_attn_args(stream, kind, q, k_cache, v_cache, block_table, seq_lens, o, b,
                                                     hq, hkv, d, page, num_pages, table_stride, max_seq_len, scale,
                                                     k_scale, v_scale, workspace, workspace_bytes), iters,
                                         ctypes.byref(ms)), "time_decode_attn")
    return ms.value


def _kv_append_args(stream: Stream, kind: str, qkv: int, qkv_stride: int, q_out: int, k_cache: int, v_cache: int,
                    block_table: int, seq_lens: int, lens_out: int, rope_cos: int, rope_sin: int, rope_len: int, b: int,
                    t: int, hq: int, hkv: int, d: int, page: int, num_pages: int, table_stride: int, max_seq_len: int,
                    k_inv_scale: float, v_inv_scale: float) -> tuple:
    if kind not in ATTN_KV_KINDS:
        raise ValueError(f"KV cache kind {kind!r}: one of {', '.join(ATTN_KV_KINDS)}")
    return (stream.handle, ATTN_KV_KINDS[kind], ctypes.c_void_p(qkv), qkv_stride,
            *(ctypes.c_void_p(x) for x in (q_out, k_cache, v_cache, block_table, seq_lens, lens_out, rope_cos,
                                           rope_sin)),
            rope_len, b, t, hq, hkv, d, page, num_pages, table_stride, max_seq_len, k_inv_scale, v_inv_scale)


def kv_append(stream: Stream, kind: str, qkv: int, qkv_stride: int, q_out: int, k_cache: int, v_cache: int,
              block_table: int, seq_lens: int, lens_out: int, rope_cos: int, rope_sin: int, rope_len: int, b: int,
              t: int, hq: int, hkv: int, d: int, page: int, num_pages: int, table_stride: int, max_seq_len: int,
              k_inv_scale: float = 1.0, v_inv_scale: float = 1.0):
    """RoPE and KV-cache append for ``b`` sequences of ``t`` new tokens each: row ``n`` of ``qkv[b * t][qkv_stride]``
    (bf16: ``hq`` query, ``hkv`` key, ``hkv`` value heads of ``d`` = 128) is token ``n % t`` of sequence ``n // t`` at
    position ``seq_lens[n // t] + n % t``.  Q and K are rotated by ``rope_cos`` / ``rope_sin`` (fp32
    ``[rope_len][d / 2]``); Q goes to ``q_out[b * t][hq][d]`` and K and V into the token's slot of the paged caches
    ``[num_pages][hkv][page][d]`` of ``kind`` ``"bf16"`` or ``"fp8"`` (OCP e4m3, saturating, after a multiplication by
    ``k_inv_scale`` / ``v_inv_scale``).  ``lens_out`` (0: none) receives the new lengths.  All addresses are device
    addresses.  Not synchronised."""
    _ck(lib().gsx_kv_append(*_kv_append_args(stream, kind, qkv, qkv_stride, q_out, k_cache, v_cache, block_table,
                                             seq_lens, lens_out, rope_cos, rope_sin, rope_len, b, t, hq, hkv, d, page,
                                             num_pages, table_stride, max_seq_len, k_inv_scale, v_inv_scale)),
        "kv_append")


def time_kv_append(stream: Stream, kind: str, qkv: int, qkv_stride: int, q_out: int, k_cache: int, v_cache: int,
                   block_table: int, seq_lens: int, lens_out: int, rope_cos: int, rope_sin: int, rope_len: int, b: int,
                   t: int, hq: int, hkv: int, d: int, page: int, num_pages: int, table_stride: int, max_seq_len: int,
                   iters: int, k_inv_scale: float = 1.0, v_inv_scale: float = 1.0) -> float:
    ms = ctypes.c_float(0)
    _ck(lib().gsx_event_time_kv_append(*_kv_append_args(stream, kind, qkv, qkv_stride, q_out, k_cache, v_cache,
                                                        block_table, seq_lens, lens_out, rope_cos, rope_sin, rope_len,
                                                        b, t, hq, hkv, d, page, num_pages, table_stride, max_seq_len,
                                                        k_inv_scale, v_inv_scale), iters, ctypes.byref(ms)),
        "time_kv_append")
    return ms.value


def _prefill_args(stream: Stream, kind: str, q: int, k_cache: int, v_cache: int, block_table: int, seq_lens: int,
                  o: int, b: int, t: int, hq: int, hkv: int, d: int, page: int, num_pages: int, table_stride: int,
                  max_seq_len: int, scale: float, k_scale: float, v_scale: float) -> tuple:
    if kind not in ATTN_KV_KINDS:
        raise ValueError(f"attention cache kind {kind!r}: one of {', '.join(ATTN_KV_KINDS)}")
    return (stream.handle, ATTN_KV_KINDS[kind], *(ctypes.c_void_p(x) for x in (q, k_cache, v_cache, block_table,
                                                                               seq_lens, o)),
            b, t, hq, hkv, d, page, num_pages, table_stride, max_seq_len, scale, k_scale, v_scale)


def prefill_attn(stream: Stream, kind: str, q: int, k_cache: int, v_cache: int, block_table: int, seq_lens: int,
                 o: int, b: int, t: int, hq: int, hkv: int, d: int, page: int, num_pages: int, table_stride: int,
                 max_seq_len: int, scale: float, k_scale: float = 1.0, v_scale: float = 1.0):
    """Causal grouped-query attention of a prefill chunk over the paged KV cache: ``o[b * t][hq][d]`` (bf16) from
    ``q[b * t][hq][d]`` (bf16, the ``q_out`` of :func:`kv_append`) and the caches ``[num_pages][hkv][page][d]`` of
    ``kind`` ``"bf16"`` or ``"fp8"``.  ``seq_lens[b]`` is the length BEFORE the chunk, the buffer :func:`kv_append`
    took: row ``n`` is at position ``seq_lens[n // t] + n % t`` and attends to the tokens up to and including its
    own.  All addresses are device addresses.  Not synchronised."""
    _ck(lib().gsx_prefill_attn(*_prefill_args(stream, kind, q, k_cache, v_cache, block_table, seq_lens, o, b, t, hq,
                                              hkv, d, page, num_pages, table_stride, max_seq_len, scale, k_scale,
                                              v_scale)), "prefill_attn")


def prefill_attn_cfg_name(cfg: int) -> str | None:
    """The name of prefill attention configuration ``cfg``, or None outside the library's table."""
    name = lib().gsx_prefill_attn_cfg_name(cfg)
    return None if name is None else name.decode()


def prefill_attn_cfg_shape(cfg: int) -> tuple[int, int, int]:
    """``(q_rows, kv_tile, waves)`` of prefill attention configuration ``cfg`` (native/kernels/attn_prefill.hip):
    query rows per workgroup, tokens per KV tile, waves per workgroup.  An unknown config raises HipError."""
    v = [ctypes.c_int(0) for _ in range(3)]
    if lib().gsx_prefill_attn_cfg_shape(cfg, *map(ctypes.byref, v)) != 0:
        raise HipError(f"prefill attn cfg {cfg}: unknown config")
    return tuple(x.value for x in v)


def prefill_attn_launch_cfg(stream: Stream, kind: str, q: int, k_cache: int, v_cache: int, block_table: int,
                            seq_lens: int, o: int, b: int, t: int, hq: int, hkv: int, d: int, page: int,
                            num_pages: int, table_stride: int, max_seq_len: int, scale: float, cfg: int,
                            k_scale: float = 1.0, v_scale: float = 1.0):
    """Launch one configuration of the prefill attention.  An unknown config raises HipError."""
    _ck(lib().gsx_prefill_attn_launch_cfg(*_prefill_args(stream, kind, q, k_cache, v_cache, block_table, seq_lens, o,
                                                         b, t, hq, hkv, d, page, num_pages, table_stride, max_seq_len,
                                                         scale, k_scale, v_scale), cfg), f"prefill attn cfg {cfg}")


def time_prefill_attn(stream: Stream, kind: str, q: int, k_cache: int, v_cache: int, block_table: int, seq_lens: int,
                      o: int, b: int, t: int, hq: int, hkv: int, d: int, page: int, num_pages: int, table_stride: int,
                      max_seq_len: int, scale: float, iters: int, k_scale: float = 1.0, v_scale: float = 1.0) -> float:
    ms = ctypes.c_float(0)
    _ck(lib().gsx_event_time_prefill_attn(*_prefill_args(stream, kind, q, k_cache, v_cache, block_table, seq_lens, o,
                                                         b, t, hq, hkv, d, page, num_pages, table_stride, max_seq_len,
                                                         scale, k_scale, v_scale), iters, ctypes.byref(ms)),
        "time_prefill_attn")
    return ms.value


# ``out_kind`` of the norm and activation kernels (gsx_kernels.h): bf16, or OCP e4m3 with one scale per row
ACT_OUT_KINDS = {"bf16": 0, "fp8": 1}


def _act_kind(out_kind: str) -> int:
    if out_kind not in ACT_OUT_KINDS:
        raise ValueError(f"output kind {out_kind!r}: one of {', '.join(ACT_OUT_KINDS)}")
    return ACT_OUT_KINDS[out_kind]


def _add_rmsnorm_args(stream: Stream, out_kind: str, x: int, x_stride: int, r_in: int, r_out: int, r_stride: int,
                      w: int, y: int, y_stride: int, scale_out: int, m: int, h: int, eps: float) -> tuple:
    return (stream.handle, _act_kind(out_kind), ctypes.c_void_p(x), x_stride, ctypes.c_void_p(r_in),
            ctypes.c_void_p(r_out), r_stride, ctypes.c_void_p(w), ctypes.c_void_p(y), y_stride,
            ctypes.c_void_p(scale_out), m, h, eps)


def add_rmsnorm(stream: Stream, out_kind: str, x: int, x_stride: int, r_in: int, r_out: int, r_stride: int, w: int,
                y: int, y_stride: int, scale_out: int, m: int, h: int, eps: float):
    """Fused residual add and RMSNorm of ``m`` rows of ``h`` bf16 elements: ``hid = bf16(x + r_in)`` (``x`` itself
    with ``r_in`` 0), ``r_out = hid`` (0: not written; ``r_out == r_in``: in place) and ``y = hid / sqrt(mean(hid^2) +
    eps) * w``.  ``out_kind`` ``"bf16"`` writes ``y`` as bf16 and takes ``scale_out`` 0; ``"fp8"`` writes OCP e4m3
    bytes and ``scale_out[m]`` (fp32) ``= max|y| / 448`` per row: the ``a`` and ``scale_a`` of
    ``decode_gemm_nt("fp8", ..., scale_mode=SCALE_ROW)``.  Strides are in elements.  All addresses are device
    addresses; 0 means NULL.  Not synchronised."""
    _ck(lib().gsx_add_rmsnorm(*_add_rmsnorm_args(stream, out_kind, x, x_stride, r_in, r_out, r_stride, w, y, y_stride,
                                                 scale_out, m, h, eps)), "add_rmsnorm")


def time_add_rmsnorm(stream: Stream, out_kind: str, x: int, x_stride: int, r_in: int, r_out: int, r_stride: int,
                     w: int, y: int, y_stride: int, scale_out: int, m: int, h: int, eps: float, iters: int) -> float:
    ms = ctypes.c_float(0)
    _ck(lib().gsx_event_time_add_rmsnorm(*_add_rmsnorm_args(stream, out_kind, x, x_stride, r_in, r_out, r_stride, w, y,
                                                            y_stride, scale_out, m, h, eps), iters, ctypes.byref(ms)),
        "time_add_rmsnorm")
    return ms.value


def _silu_mul_args(stream: Stream, out_kind: str, gu: int, gu_stride: int, y: int, y_stride: int, scale_out: int,
                   m: int, i: int) -> tuple:
    return (stream.handle, _act_kind(out_kind), ctypes.c_void_p(gu), gu_stride, ctypes.c_void_p(y), y_stride,
            ctypes.c_void_p(scale_out), m, i)


def silu_mul(stream: Stream, out_kind: str, gu: int, gu_stride: int, y: int, y_stride: int, scale_out: int, m: int,
             i: int):
    """SwiGLU: row ``r`` of ``gu[m][gu_stride]`` (bf16) holds ``i`` gate values, then ``i`` up values;
    ``y[r][c] = silu(gate[c]) * up[c]``, as bf16 or (``out_kind`` ``"fp8"``) as OCP e4m3 with ``scale_out[m]``, as
    :func:`add_rmsnorm` writes them.  All addresses are device addresses; 0 means NULL.  Not synchronised."""
    _ck(lib().gsx_silu_mul(*_silu_mul_args(stream, out_kind, gu, gu_stride, y, y_stride, scale_out, m, i)), "silu_mul")


def time_silu_mul(stream: Stream, out_kind: str, gu: int, gu_stride: int, y: int, y_stride: int, scale_out: int,
                  m: int, i: int, iters: int) -> float:
    ms = ctypes.c_float(0)
    _ck(lib().gsx_event_time_silu_mul(*_silu_mul_args(stream, out_kind, gu, gu_stride, y, y_stride, scale_out, m, i),
                                      iters, ctypes.byref(ms)), "time_silu_mul")
    return ms.value


def _sample_args(stream: Stream, logits: int, logits_stride: int, temperature: int, top_k: int, top_p: int,
                 seeds: int, counter: int, tokens_out: int, m: int, v: int) -> tuple:
    return (stream.handle, ctypes.c_void_p(logits), logits_stride, ctypes.c_void_p(temperature),
            ctypes.c_void_p(top_k), ctypes.c_void_p(top_p), ctypes.c_void_p(seeds), counter & 0xFFFFFFFFFFFFFFFF,
            ctypes.c_void_p(tokens_out), m, v)


def sample(stream: Stream, logits: int, logits_stride: int, temperature: int, top_k: int, top_p: int, seeds: int,
           counter: int, tokens_out: int, m: int, v: int):
    """One token id (int32, ``tokens_out[m]``) from each of ``m`` rows of ``v`` bf16 logits, what ``decode_gemm_nt``
    writes as an LM head; a ``logits_stride`` of 0 makes every row read the same logits.  ``temperature`` (fp32),
    ``top_k`` (int32), ``top_p`` (fp32) and ``seeds`` (uint64) are per-row arrays in device memory; ``temperature`` 0
    (NULL) makes every row greedy, ``top_k`` 0 and ``top_p`` 0 mean no limit.  A row whose temperature is NaN or <= 0
    is greedy: the lowest index of the largest logit.  ``counter`` is the step number, a host value.  The result is
    exact (tests/sample_cases.py is its twin).  All addresses are device addresses; 0 means NULL.  Not synchronised."""
    _ck(lib().gsx_sample(*_sample_args(stream, logits, logits_stride, temperature, top_k, top_p, seeds, counter,
                                       tokens_out, m, v)), "sample")


def time_sample(stream: Stream, logits: int, logits_stride: int, temperature: int, top_k: int, top_p: int, seeds: int,
                counter: int, tokens_out: int, m: int, v: int, iters: int) -> float:
    ms = ctypes.c_float(0)
    _ck(lib().gsx_event_time_sample(*_sample_args(stream, logits, logits_stride, temperature, top_k, top_p, seeds,
                                                  counter, tokens_out, m, v), iters, ctypes.byref(ms)), "time_sample")
    return ms.value


def _embed_gather_args(stream: Stream, table: int, table_stride: int, tokens: int, out: int, out_stride: int, m: int,
                       h: int, v: int) -> tuple:
    return (stream.handle, ctypes.c_void_p(table), table_stride, ctypes.c_void_p(tokens), ctypes.c_void_p(out),
            out_stride, m, h, v)


def embed_gather(stream: Stream, table: int, table_stride: int, tokens: int, out: int, out_stride: int, m: int, h: int,
                 v: int):
    """``out[r][0..h)`` is a raw 16-bit copy of ``table[tokens[r]][0..h)`` for ``m`` int32 token ids in device memory; a
    token outside ``[0, v)`` gives a row of zeros.  Strides are in elements.  All addresses are device addresses.  Not
    synchronised."""
    _ck(lib().gsx_embed_gather(*_embed_gather_args(stream, table, table_stride, tokens, out, out_stride, m, h, v)),
        "embed_gather")


def time_embed_gather(stream: Stream, table: int, table_stride: int, tokens: int, out: int, out_stride: int, m: int,
                      h: int, v: int, iters: int) -> float:
    ms = ctypes.c_float(0)
    _ck(lib().gsx_event_time_embed_gather(*_embed_gather_args(stream, table, table_stride, tokens, out, out_stride, m,
                                                              h, v), iters, ctypes.byref(ms)), "time_embed_gather")
    return ms.value


# Mixture-of-experts decode (gsx_kernels.h): at most 16 tokens x 8 experts = 128 (token, expert) pairs, and a plan of
# 516 int32 in device memory that groups them by expert
MOE_MAX_PAIRS = 128
MOE_PLAN_INTS = 4 + 4 * MOE_MAX_PAIRS


def _moe_route_args(stream: Stream, logits: int, logits_stride: int, topk_ids: int, topk_w: int, plan: int, m: int,
                    e: int, topk: int) -> tuple:
    return (stream.handle, ctypes.c_void_p(logits), logits_stride, ctypes.c_void_p(topk_ids), ctypes.c_void_p(topk_w),
            ctypes.c_void_p(plan), m, e, topk)


def moe_route(stream: Stream, logits: int, logits_stride: int, topk_ids: int, topk_w: int, plan: int, m: int, e: int,
              topk: int):
    """The MoE router: from ``m <= 16`` rows of ``e`` bf16 router logits, ``topk_ids[m][topk]`` (int32, descending
    logit, ties to the lowest index), ``topk_w[m][topk]`` (fp32, a softmax over the selected logits) and ``plan``
    (``MOE_PLAN_INTS`` int32: the pairs grouped by expert, what :func:`moe_gemm_nt` reads).  Ids and plan are exact
    (tests/moe_cases.py is their twin).  All addresses are device addresses.  Not synchronised."""
    _ck(lib().gsx_moe_route(*_moe_route_args(stream, logits, logits_stride, topk_ids, topk_w, plan, m, e, topk)),
        "moe_route")


def time_moe_route(stream: Stream, logits: int, logits_stride: int, topk_ids: int, topk_w: int, plan: int, m: int,
                   e: int, topk: int, iters: int) -> float:
    ms = ctypes.c_float(0)
    _ck(lib().gsx_event_time_moe_route(*_moe_route_args(stream, logits, logits_stride, topk_ids, topk_w, plan, m, e,
                                                        topk), iters, ctypes.byref(ms)), "time_moe_route")
    return ms.value


def _moe_gemm_args(stream: Stream, kind: str, a: int, a_div: int, b: int, c: int, plan: int, m: int, topk: int, e: int,
                   n: int, k: int, scale_a: int, scale_b: int, scale_mode: int) -> tuple:
    return (stream.handle, _decode_kind(kind), ctypes.c_void_p(a), a_div, ctypes.c_void_p(b), ctypes.c_void_p(c),
            ctypes.c_void_p(plan), m, topk, e, n, k, ctypes.c_void_p(scale_a), ctypes.c_void_p(scale_b), scale_mode)


def moe_gemm_nt(stream: Stream, kind: str, a: int, a_div: int, b: int, c: int, plan: int, m: int, topk: int, e: int,
                n: int, k: int, scale_a: int = 0, scale_b: int = 0, scale_mode: int = SCALE_NONE):
    """The grouped expert GEMM: for every pair ``p`` of ``plan`` with expert ``x``, ``C[p][n]`` (bf16) ``=
    A[p // a_div][k] * B[x][n][k]^T``.  ``a_div = topk`` is the up projection (a pair reads its token's row),
    ``a_div = 1`` the down projection (a pair reads its own row).  ``kind`` and operand formats as
    :func:`decode_gemm_nt`; fp8 takes ``SCALE_NONE`` or ``SCALE_ROW`` (``scale_a`` per row of A, ``scale_b[e][n]``),
    mxfp4 ``scale_a[rows of A][k / 32]`` and ``scale_b[e][n][k / 32]``.  Only the experts the plan names are read.
    Not synchronised."""
    _ck(lib().gsx_moe_gemm_nt(*_moe_gemm_args(stream, kind, a, a_div, b, c, plan, m, topk, e, n, k, scale_a, scale_b,
                                              scale_mode)), "moe_gemm_nt")


def moe_gemm_cfgs() -> dict[int, tuple[str, int, int, int, int]]:
    """``{index: (name, bn, waves, inflight, decode_cfg)}`` of the grouped GEMM's configurations, read from the
    library's table: the four shapes the decode GEMM dispatches to, each with the index of the decode configuration
    (:func:`decode_gemm_cfgs`) it equals."""
    out: dict[int, tuple[str, int, int, int, int]] = {}
    while (name := lib().gsx_moe_gemm_cfg_name(len(out))) is not None:
        v = [ctypes.c_int(0) for _ in range(4)]
        if lib().gsx_moe_gemm_cfg_shape(len(out), *map(ctypes.byref, v)) != 0:
            raise HipError(f"moe gemm cfg {len(out)} has a name and no shape")
        out[len(out)] = (name.decode(), *(x.value for x in v))
    return out


def moe_gemm_nt_cfg(stream: Stream, kind: str, a: int, a_div: int, b: int, c: int, plan: int, m: int, topk: int,
                    e: int, n: int, k: int, cfg: int, scale_a: int = 0, scale_b: int = 0,
                    scale_mode: int = SCALE_NONE):
    """Launch one configuration of the grouped GEMM; an unknown config or a shape it cannot take raises HipError."""
    _ck(lib().gsx_moe_gemm_nt_launch_cfg(*_moe_gemm_args(stream, kind, a, a_div, b, c, plan, m, topk, e, n, k,
                                                         scale_a, scale_b, scale_mode), cfg), f"moe gemm cfg {cfg}")


def time_moe_gemm(stream: Stream, kind: str, a: int, a_div: int, b: int, c: int, plan: int, m: int, topk: int, e: int,
                  n: int, k: int, iters: int, scale_a: int = 0, scale_b: int = 0,
                  scale_mode: int = SCALE_NONE) -> float:
    ms = ctypes.c_float(0)
    _ck(lib().gsx_event_time_moe_gemm(*_moe_gemm_args(stream, kind, a, a_div, b, c, plan, m, topk, e, n, k, scale_a,
                                                      scale_b, scale_mode), iters, ctypes.byref(ms)), "time_moe_gemm")
    return ms.value


def _moe_combine_args(stream: Stream, y: int, y_stride: int, topk_w: int, out: int, out_stride: int, m: int, topk: int,
                      h: int) -> tuple:
    return (stream.handle, ctypes.c_void_p(y), y_stride, ctypes.c_void_p(topk_w), ctypes.c_void_p(out), out_stride, m,
            topk, h)


def moe_combine(stream: Stream, y: int, y_stride: int, topk_w: int, out: int, out_stride: int, m: int, topk: int,
                h: int):
    """``out[r][0..h)`` (bf16) is the sum over ``j`` of ``topk_w[r][j] * Y[r * topk + j][0..h)``, in fp32, in the order
    of ``j``, every multiply and add rounded on its own: bit-exact.  Strides are in elements.  Not synchronised."""
    _ck(lib().gsx_moe_combine(*_moe_combine_args(stream, y, y_stride, topk_w, out, out_stride, m, topk, h)),
        "moe_combine")


def time_moe_combine(stream: Stream, y: int, y_stride: int, topk_w: int, out: int, out_stride: int, m: int, topk: int,
                     h: int, iters: int) -> float:
    ms = ctypes.c_float(0)
    _ck(lib().gsx_event_time_moe_combine(*_moe_combine_args(stream, y, y_stride, topk_w, out, out_stride, m, topk, h),
                                         iters, ctypes.byref(ms)), "time_moe_combine")
    return ms.value
