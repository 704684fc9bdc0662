"""HIP/CDNA4 kernels on a real MI355X (run with ``-m gpu`` on the GPU box).

Numerics are checked against plain PyTorch fp32 references; the CU probe and
HBM stamp tests check the isolation/placement properties the device plugin
relies on.
"""
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    from gpushare_scheduler_extender_amd.ops import hip as h

    assert h.SO.exists()
    return h


def test_device_info_is_mi355x(hip):
    info = hip.device_info(0)
    assert info["arch"].startswith("gfx950"), info
    assert info["cu_count"] == 256
    free, total = hip.mem_info(0)
    assert total > 250 * 10**9 and free <= total


def test_hbm_stamp_verify_and_overlap_detection(hip):
    s = hip.Stream(0)
    buf = hip.DeviceBuffer(0, 256 << 20)
    half = 128 << 20
    hip.hbm_stamp(s, buf.addr(0), half, 1 << 16, 111)
    hip.hbm_stamp(s, buf.addr(half), half, 1 << 16, 222)
    assert hip.hbm_verify(s, buf.addr(0), half, 1 << 16, 111) == 0
    assert hip.hbm_verify(s, buf.addr(half), half, 1 << 16, 222) == 0
    # a third "pod" placed over the second half of pod 111 corrupts exactly its stamps
    hip.hbm_stamp(s, buf.addr(half // 2), half // 2, 1 << 16, 333)
    assert hip.hbm_verify(s, buf.addr(0), half, 1 << 16, 111) == (half // 2) // (1 << 16)
    buf.free()
    s.destroy()


def test_hbm_admit_batched_stamp_and_verify(hip):
    s = hip.Stream(0)
    buf = hip.DeviceBuffer(0, 64 << 20)
    mib16, st = 16 << 20, 1 << 16
    a = (buf.addr(0), mib16, 11)
    b = (buf.addr(mib16), mib16, 22)
    assert hip.hbm_admit_n(s, [a], 1, st) == 0
    assert hip.hbm_admit_n(s, [b, a], 1, st) == 0
    # a pod wrongly placed over the second half of a and the first half of b
    c = (buf.addr(mib16 // 2), mib16, 33)
    assert hip.hbm_admit_n(s, [c, a, b], 1, st) == 2 * (mib16 // 2) // st
    assert hip.hbm_admit_n(s, [c], 0, st) == 0
    # more slices than one launch's table (32): chunked launches
    many = [(buf.addr(i * (1 << 20)), 1 << 20, 100 + i) for i in range(40)]
    for i in range(40):
        assert hip.hbm_admit_n(s, [many[i]] + many[:i], 1, st) == 0
    buf.free()
    s.destroy()


def test_hbm_admit_n_multi_extent_pods(hip):
    """A pod whose slice is two extents (fragmented arena): both stamped in one launch, every slice verified."""
    s = hip.Stream(0)
    buf = hip.DeviceBuffer(0, 64 << 20)
    mib8, st = 8 << 20, 1 << 16
    a = (buf.addr(0), mib8, 11)
    b = (buf.addr(2 * mib8), mib8, 22)
    assert hip.hbm_admit_n(s, [a, b], 2, st) == 0  # two pods stamped at once
    # pod 33 lives in the holes around b: [8, 16) MiB and [24, 40) MiB
    c = [(buf.addr(mib8), mib8, 33), (buf.addr(3 * mib8), 2 * mib8, 33)]
    assert hip.hbm_admit_n(s, c + [a, b], 2, st) == 0
    # stamp-only admission (verify off) does not report, the next full verify does
    d = [(buf.addr(mib8 + mib8 // 2), mib8, 44)]  # wrongly over the second half of c[0] and first half of b
    assert hip.hbm_admit_n(s, d, 1, st, verify=False) == 0
    assert hip.hbm_admit_n(s, c + [a, b], 0, st) == 2 * (mib8 // 2) // st
    # more extents than one launch's table (32)
    many = [(buf.addr(i * (1 << 20)), 1 << 20, 500) for i in range(40)]
    assert hip.hbm_admit_n(s, many, 40, st) == 0
    buf.free()
    s.destroy()


def test_hbm_admit_n_counts_damage_and_overlap(hip):
    """A verify-only table counts a resident slice's overwritten stamps, and an admission placed over two resident
    extents adds the stamps it overwrote to that count."""
    s = hip.Stream(0)
    buf = hip.DeviceBuffer(0, 64 << 20)
    mib8, st = 8 << 20, 1 << 16
    a, b = (buf.addr(0), mib8, 11), (buf.addr(2 * mib8), mib8, 22)
    assert hip.hbm_admit_n(s, [a, b], 2, st) == 0  # two new, nothing resident
    c = [(buf.addr(mib8), mib8, 33), (buf.addr(3 * mib8), 2 * mib8, 33)]
    assert hip.hbm_admit_n(s, c + [a, b], 2, st) == 0  # two more, the first two resident
    hip.hbm_fill(s, buf.addr(0), 1 << 20, 0)  # damage a
    s.sync()
    assert hip.hbm_admit_n(s, c + [a, b], 0, st) == (1 << 20) // st  # verify-only table
    d = [(buf.addr(mib8 + mib8 // 2), mib8, 44)]  # overlaps c[0] and b
    assert hip.hbm_admit_n(s, d + c + [a, b], 1, st) == 2 * (mib8 // 2) // st + (1 << 20) // st
    buf.free()
    s.destroy()


def test_hbm_fill_pattern_and_bandwidth(hip):
    s = hip.Stream(0)
    n = 4 << 30
    t = torch.empty(n // 4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    hip.hbm_fill(s, t.data_ptr(), 4096, 0x1234ABCD)
    s.sync()
    assert (t[:1024] == 0x1234ABCD).all()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    hip.hbm_fill(s, t.data_ptr(), n, 7)
    s.sync()
    ev0.record()
    for _ in range(5):
        hip.hbm_fill(s, t.data_ptr(), n, 7)
    s.sync()
    ev1.record()
    torch.cuda.synchronize()
    # events are on the default stream, our stream was synced in between: wall time via python instead
    import time
    t0 = time.perf_counter()
    for _ in range(5):
        hip.hbm_fill(s, t.data_ptr(), n, 9)
    s.sync()
    dt = time.perf_counter() - t0
    bw = 5 * n / dt / 1e12
    print(f"hbm fill {bw:.2f} TB/s")
    assert int(t[-1].item()) == 9
    assert bw > 2.0  # write roofline ~5-6 TB/s on MI355X; a broken kernel is far below


@pytest.mark.parametrize("m,n,k", [(128, 128, 64), (256, 384, 192), (1024, 512, 1024)])
def test_gemm_bf16_matches_fp32_reference(hip, m, n, k):
    torch.manual_seed(m + n + k)
    a = torch.randn(m, k, device="cuda", dtype=torch.bfloat16)
    b = torch.randn(n, k, device="cuda", dtype=torch.bfloat16)
    c = torch.empty(m, n, device="cuda", dtype=torch.bfloat16)
    s = hip.Stream(0)
    torch.cuda.synchronize()
    hip.gemm_bf16_nt(s, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k)
    s.sync()
    ref = a.float() @ b.float().t()
    torch.testing.assert_close(c.float(), ref, atol=0.05 * (k ** 0.5), rtol=1e-2)
    s.destroy()


def test_gemm_asymmetric_identity(hip):
    """A = I with an asymmetric B catches a transposed C write (guide §3)."""
    m = 128
    a = torch.eye(m, device="cuda", dtype=torch.bfloat16)
    b = (torch.arange(128 * 128, device="cuda", dtype=torch.float32).reshape(128, 128) % 97).to(torch.bfloat16)
    c = torch.empty(m, 128, device="cuda", dtype=torch.bfloat16)
    s = hip.Stream(0)
    torch.cuda.synchronize()
    hip.gemm_bf16_nt(s, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, 128, 128)
    s.sync()
    torch.testing.assert_close(c.float(), b.float().t(), atol=0, rtol=0)
    s.destroy()


def test_gemm_rejects_bad_shapes(hip):
    s = hip.Stream(0)
    with pytest.raises(hip.HipError):
        hip.gemm_bf16_nt(s, 0, 0, 0, 100, 128, 64)
    s.destroy()


def test_cuprobe_full_and_masked(hip):
    s = hip.Stream(0)
    full = hip.physical_cus(hip.cuprobe(s, 8192, 20000))
    s.destroy()
    print("distinct CUs unmasked:", len(full))
    assert len(full) >= 200
    words = hip.mask_words(range(0, 64))
    m = hip.Stream(0, words)
    assert m.mask(8)[:2] == [0xFFFFFFFF, 0xFFFFFFFF]
    part = hip.physical_cus(hip.cuprobe(m, 8192, 20000))
    m.destroy()
    print("distinct CUs with a 64-CU mask:", len(part))
    # exactly the 64 CUs of the mask run work, and four disjoint masks cover four disjoint CU sets
    assert len(part) == 64 and part <= full
    quarters = []
    for q in range(4):
        ms = hip.Stream(0, hip.mask_words(range(64 * q, 64 * (q + 1))))
        quarters.append(hip.physical_cus(hip.cuprobe(ms, 8192, 20000)))
        ms.destroy()
    assert [len(x) for x in quarters] == [64] * 4
    assert all(not (quarters[i] & quarters[j]) for i in range(4) for j in range(i + 1, 4))
    assert set().union(*quarters) == full and len(full) == 256
    assert quarters[0] == part


def test_hsa_cu_mask_env_limits_process():
    """The device plugin's HSA_CU_MASK env restricts a whole process (checked in a child)."""
    code = ("from gpushare_scheduler_extender_amd.ops import hip;"
            "s=hip.Stream(0);print(len(hip.physical_cus(hip.cuprobe(s,8192,20000))))")
    env = dict(os.environ, HSA_CU_MASK="0:0-31")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, r.stderr
    n = int(r.stdout.strip().splitlines()[-1])
    print("distinct CUs under HSA_CU_MASK=0:0-31:", n)
    assert n == 32  # the process sees exactly the 32 CUs ROCr's mask leaves it


def test_arena_runtime_admits_four_64gib_pods():
    """BASELINE config 2: 4 x 64 GiB pods co-resident on one MI355X, stamps verified."""
    from gpushare_scheduler_extender_amd.deviceplugin.runtime import HbmArenaRuntime, AdmissionError

    gib = 1 << 30
    rt = HbmArenaRuntime({0: 256 * gib})
    try:
        for i in range(4):
            rt.start(f"pod-{i}", 0, 64 * gib)
        assert rt.verify() == 0
        with pytest.raises(AdmissionError):
            rt.start("pod-5", 0, 1 * gib)
        rt.stop("pod-1")
        rt.start("pod-6", 0, 64 * gib)
        assert rt.verify() == 0
    finally:
        rt.close()


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10])
def test_gemm_tile_configs_match_fp32_reference(hip, cfg):
    m, n, k = 512, 512, 256
    torch.manual_seed(cfg)
    a = torch.randn(m, k, device="cuda", dtype=torch.bfloat16)
    b = torch.randn(n, k, device="cuda", dtype=torch.bfloat16)
    c = torch.empty(m, n, device="cuda", dtype=torch.bfloat16)
    s = hip.Stream(0)
    torch.cuda.synchronize()
    hip.gemm_bf16_nt_cfg(s, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, cfg)
    s.sync()
    torch.testing.assert_close(c.float(), a.float() @ b.float().t(), atol=0.05 * (k ** 0.5), rtol=1e-2)
    # asymmetric identity check: C = I * B^T must be exact
    eye = torch.eye(m, k, device="cuda", dtype=torch.bfloat16)
    bb = (torch.arange(n * k, device="cuda", dtype=torch.float32).reshape(n, k) % 61).to(torch.bfloat16)
    torch.cuda.synchronize()
    hip.gemm_bf16_nt_cfg(s, eye.data_ptr(), bb.data_ptr(), c.data_ptr(), m, n, k, cfg)
    s.sync()
    torch.testing.assert_close(c.float()[:, :], (eye.float() @ bb.float().t()), atol=0, rtol=0)
    s.destroy()


@pytest.mark.parametrize("m,n,k", [(256, 256, 64), (768, 1280, 320), (2048, 512, 4096)])
def test_gemm_phased_edge_shapes(hip, m, n, k):
    """Phased kernel: one K-tile (clamped prefetch), odd tile counts, long K (many buffer reuses)."""
    torch.manual_seed(k)
    a = torch.randn(m, k, device="cuda", dtype=torch.bfloat16)
    b = torch.randn(n, k, device="cuda", dtype=torch.bfloat16)
    ref = a.float() @ b.float().t()
    s = hip.Stream(0)
    for cfg in (5, 6, 7, 8, 9, 10):
        c = torch.full((m, n), float("nan"), device="cuda", dtype=torch.bfloat16)
        torch.cuda.synchronize()
        hip.gemm_bf16_nt_cfg(s, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, cfg)
        s.sync()
        torch.testing.assert_close(c.float(), ref, atol=0.05 * (k ** 0.5), rtol=1e-2)
    s.destroy()


def test_gemm_phased_is_deterministic(hip):
    """Race screen for the counted-vmcnt schedule: 30 back-to-back runs must be bit-identical."""
    m, n, k = 4096, 4096, 1024
    torch.manual_seed(7)
    a = torch.rand(m, k, device="cuda", dtype=torch.bfloat16) * 2 - 1
    b = torch.rand(n, k, device="cuda", dtype=torch.bfloat16) * 2 - 1
    s = hip.Stream(0)
    for cfg in (5, 6, 7, 8, 9, 10):
        c0 = torch.empty(m, n, device="cuda", dtype=torch.bfloat16)
        c = torch.empty_like(c0)
        torch.cuda.synchronize()
        hip.gemm_bf16_nt_cfg(s, a.data_ptr(), b.data_ptr(), c0.data_ptr(), m, n, k, cfg)
        s.sync()
        for _ in range(30):
            hip.gemm_bf16_nt_cfg(s, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, cfg)
            s.sync()
            assert torch.equal(c, c0)
        torch.testing.assert_close(c0.float(), a.float() @ b.float().t(), atol=0.05 * (k ** 0.5), rtol=1e-2)
    s.destroy()


GEMM_CFG_NAMES = ["128x128/4w", "256x128/8w", "128x256/8w", "256x256/8w", "128x128/4w-nogroup",
                  "256x256/8w-phased-g4", "256x256/8w-phased-g8", "256x256/4w-agpr-g4", "256x256/4w-agpr-g8",
                  "256x256/4w-asm-agpr-g4", "256x256/8w-phased-g4-mfma32"]


@pytest.fixture(scope="module")
def gemm_exact_case():
    """Host-built operands whose product has no rounding before the final bf16 conversion: every input is k/16 with
    |k| <= 15 (a bf16), every product a multiple of 2^-8 and every partial sum below 71, so fp32 accumulation is
    exact in any order and the kernel has to equal the fp64 product rounded once."""
    from tests.gemm_cases import exact_case  # the generator lives with the other GEMM test operands

    return exact_case(768, 1280, 320)


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10])
def test_gemm_tile_configs_exact_on_ragged_grid(hip, gemm_exact_case, cfg):
    """768 x 1280 x 320: a ragged last tile-row group for every GROUP_M, grids of 15 / 30 / 60 blocks (no multiple
    of the 8 XCDs), 5 K-tiles; row / column periods 31 and 29 put different data under every tile."""
    a_h, b_h, want = gemm_exact_case
    (m, k), n = a_h.shape, b_h.shape[0]
    a, b = a_h.cuda(), b_h.cuda()
    c = torch.full((m, n), float("nan"), device="cuda", dtype=torch.bfloat16)
    s = hip.Stream(0)
    torch.cuda.synchronize()
    hip.gemm_bf16_nt_cfg(s, a.data_ptr(), b.data_ptr(), c.data_ptr(), m, n, k, cfg)
    s.sync()
    torch.testing.assert_close(c.cpu(), want, atol=0, rtol=0)
    s.destroy()


def test_gemm_cfg_table(hip):
    import ctypes

    L = hip.lib()
    assert [L.gsx_gemm_cfg_name(c) for c in range(11)] == [x.encode() for x in GEMM_CFG_NAMES]
    assert L.gsx_gemm_cfg_name(-1) is None and L.gsx_gemm_cfg_name(11) is None
    for c, name in enumerate(GEMM_CFG_NAMES):
        bm, bn = ctypes.c_int(0), ctypes.c_int(0)
        assert L.gsx_gemm_cfg_tile(c, ctypes.byref(bm), ctypes.byref(bn)) == 0
        assert f"{bm.value}x{bn.value}" == name.split("/")[0]
    assert L.gsx_gemm_cfg_tile(11, ctypes.byref(bm), ctypes.byref(bn)) != 0
    assert hip.gemm_cfgs() == dict(enumerate(GEMM_CFG_NAMES))


def test_gemm_launch_cfg_rejects_in_c(hip):
    """The exported launcher itself refuses what a configuration cannot take.  Every call gets real buffers for
    512 x 512 x 128 (A and B with a spare block on either side), so a check that went missing would show as a
    wrong answer and not as an access outside the buffers."""
    import ctypes

    m, n, k = 512, 512, 128
    torch.manual_seed(3)
    ab = torch.randint(-3, 4, (2, 3, m, k), device="cuda").to(torch.bfloat16)
    a, b = ab[0, 1], ab[1, 1]
    c = torch.full((m, n), float("nan"), device="cuda", dtype=torch.bfloat16)
    pa, pb, pc = a.data_ptr(), b.data_ptr(), c.data_ptr()
    s = hip.Stream(0)
    torch.cuda.synchronize()
    cases = [(0, pa, pb, pc, 200, n, k), (5, pa, pb, pc, m, 384, k), (11, pa, pb, pc, m, n, k)]
    for cfg in range(11):
        cases += [(cfg, pa, pb, pc, m, n, 0), (cfg, pa, pb, pc, m, n, 96)]
        # misaligned operands, at a shape that stays inside the buffers
        cases += [(cfg, pa + 8, pb, pc, 256, 256, 64), (cfg, pa, pb + 8, pc, 256, 256, 64),
                  (cfg, pa, pb, pc + 8, 256, 256, 64)]
    L = hip.lib()
    for cfg, xa, xb, xc, xm, xn, xk in cases:
        rc = L.gsx_gemm_bf16_nt_launch_cfg(s.handle, ctypes.c_void_p(xa), ctypes.c_void_p(xb), ctypes.c_void_p(xc),
                                           xm, xn, xk, cfg)
        assert rc != 0, (cfg, xm, xn, xk)
        assert L.gsx_last_error().decode().startswith("gsx_gemm_bf16_nt_launch_cfg:"), L.gsx_last_error()
        with pytest.raises(hip.HipError):
            hip.gemm_bf16_nt_cfg(s, xa, xb, xc, xm, xn, xk, cfg)
    s.sync()
    assert bool(torch.isnan(c.float()).all())  # no rejected call launched anything
    hip.gemm_bf16_nt_cfg(s, pa, pb, pc, m, n, k, 5)
    s.sync()
    want = (a.double() @ b.double().t()).float().bfloat16()  # small integers: exact up to the one final rounding
    torch.testing.assert_close(c, want, atol=0, rtol=0)
    s.destroy()


def test_hbm_verify_counts_are_per_call_under_concurrency(hip):
    """two host threads verifying on one device must each get their own bad-stamp count (the
    per-device counter's reset -> launch -> readback is serialised).  ctypes drops the GIL, so the calls
    really overlap."""
    import threading

    st, mib = 1 << 16, 1 << 20
    bufs = [hip.DeviceBuffer(0, 32 * mib) for _ in range(2)]
    streams = [hip.Stream(0) for _ in range(2)]
    for b, s in zip(bufs, streams):
        hip.hbm_stamp(s, b.addr(0), 32 * mib, st, 77)
        s.sync()
    n = (32 * mib) // st
    errs, done = [], []

    def run(i):
        want = 0 if i == 0 else n  # thread 1 verifies against the wrong tag: every stamp is bad
        tag = 77 if i == 0 else 78
        for _ in range(300):
            got = hip.hbm_verify(streams[i], bufs[i].addr(0), 32 * mib, st, tag)
            if got != want:
                errs.append((i, got, want))
                return
            got = hip.hbm_admit_n(streams[i], [(bufs[i].addr(0), 32 * mib, tag)], 0, st)
            if got != want:
                errs.append((i, "admit", got, want))
                return
        done.append(i)  # a call that raised ends its thread before this line
    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for b, s in zip(bufs, streams):
        b.free()
        s.destroy()
    assert not errs, errs[:3]
    assert sorted(done) == [0, 1], done


# ---- characterisation of the stamp / verify paths against a NumPy twin --------------------------------------
# Stamp i of an extent is the 16 bytes {tag, i * stride} (two little-endian u64) at byte i * stride of the extent;
# a stamp is bad when either word differs.  The twin works on a host byte array that mirrors the device buffer.

def _twin_stamp(arr, off, nbytes, stride, tag):
    import numpy as np

    for i in range(nbytes // stride):
        arr[off + i * stride: off + i * stride + 16] = np.array([tag, i * stride], dtype="<u8").view(np.uint8)


def _twin_bad(arr, off, nbytes, stride, tag):
    import numpy as np

    bad = 0
    for i in range(nbytes // stride):
        got = arr[off + i * stride: off + i * stride + 16].view("<u8")
        bad += int(got[0] != tag or got[1] != i * stride)
    return bad


def _readback(buf):
    import numpy as np

    return np.frombuffer(buf.to_host(), dtype=np.uint8)


def test_hbm_stamp_content_byte_for_byte(hip):
    """Both stamping entry points write exactly the twin's bytes: an extent that is only 16-B aligned, a stride
    that is no power of two, a trailing partial stride, and nothing outside the stamps is touched."""
    import numpy as np

    size, off, stride, tag = 1 << 20, 48, 4112, 0x1122334455667788
    nbytes = 5 * stride + 40
    want = np.full(size, 0xA5, dtype=np.uint8)
    _twin_stamp(want, off, nbytes, stride, tag)
    assert int((want != 0xA5).sum()) > 0
    s = hip.Stream(0)
    for how in ("stamp", "admit_n"):
        buf = hip.DeviceBuffer(0, size)
        buf.from_host(bytes([0xA5]) * size)
        if how == "stamp":
            hip.hbm_stamp(s, buf.addr(off), nbytes, stride, tag)
            s.sync()
        else:
            assert hip.hbm_admit_n(s, [(buf.addr(off), nbytes, tag)], 1, stride, verify=False) == 0
        got = _readback(buf)
        buf.free()
        assert np.array_equal(got, want), (how, np.flatnonzero(got != want)[:8])
    s.destroy()


@pytest.mark.parametrize("cap,how", [(8192, "single"), (1024, "table")])
def test_hbm_stamps_beyond_one_pass_of_the_grid(hip, cap, how):
    """``cap * 256 + 257`` stamps at stride 16: every lane of the capped grid takes a second trip of the grid-stride
    loop and one block a ragged third (single-range cap 8192 blocks, table cap 1024 blocks per row)."""
    import numpy as np

    n, stride, tag = cap * 256 + 257, 16, 0xC0FFEE
    nbytes = n * stride
    s = hip.Stream(0)
    buf = hip.DeviceBuffer(0, nbytes)
    buf.from_host(bytes(nbytes))
    ext = (buf.addr(0), nbytes, tag)
    if how == "single":
        hip.hbm_stamp(s, *ext[:2], stride, tag)
        assert hip.hbm_verify(s, *ext[:2], stride, tag) == 0
    else:
        assert hip.hbm_admit_n(s, [ext], 1, stride) == 0
    want = np.empty((n, 2), dtype="<u8")
    want[:, 0] = tag
    want[:, 1] = np.arange(n, dtype=np.uint64) * stride
    got = _readback(buf).view("<u8").reshape(n, 2)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]
    # five bad stamps written from the host, around the ends of the grid's first pass: wrong tag or wrong offset
    for k, i in enumerate((0, cap * 256 - 1, cap * 256, n - 1, n // 2 + 3)):
        words = [tag + 1, i * stride] if k % 2 == 0 else [tag, i * stride + 16]
        buf.from_host(np.array(words, dtype="<u8").tobytes(), i * stride)
    assert hip.hbm_verify(s, *ext[:2], stride, tag) == 5
    assert hip.hbm_admit_n(s, [ext], 0, stride) == 5
    buf.free()
    s.destroy()


def test_hbm_admit_n_ragged_table_across_the_chunk(hip):
    """40 disjoint extents of differing sizes (zero stamps, one stamp, several with more than one block's 256),
    33 of them stamped: two chunks of the 32-row table for the stamp and for the verify.  Then an extent placed
    over two of them: the count is the one the twin gets by replaying the same writes on a host byte array."""
    import numpy as np

    stride, slot = 64, 1 << 16
    counts = [0, 1, 257, 300, 700, 1000] + [(k * 37) % 90 + 2 for k in range(6, 40)]
    lens = [stride - 16 if c == 0 else c * stride + (k % 3) * 8 for k, c in enumerate(counts)]
    assert all(n <= slot for n in lens)
    size = 40 * slot
    s = hip.Stream(0)
    buf = hip.DeviceBuffer(0, size)
    ext = [(buf.addr(k * slot), lens[k], 900 + k) for k in range(40)]
    # the seven extents that this admission does not stamp are resident already: their stamps come from the host
    host = np.full(size, 0x3C, dtype=np.uint8)
    for k in range(33, 40):
        _twin_stamp(host, k * slot, lens[k], stride, 900 + k)
    buf.from_host(host.tobytes())
    assert hip.hbm_admit_n(s, ext, 33, stride) == 0
    for k in range(33):
        _twin_stamp(host, k * slot, lens[k], stride, 900 + k)
    got = _readback(buf)
    assert np.array_equal(got, host), np.flatnonzero(got != host)[:8]
    # over the tail of extent 4 (from its stamp 100) and the first 50 stamps of extent 5
    x_off, x_len = 4 * slot + 100 * stride, (slot - 100 * stride) + 50 * stride + 8
    assert hip.hbm_admit_n(s, [(buf.addr(x_off), x_len, 77)], 1, stride, verify=False) == 0
    _twin_stamp(host, x_off, x_len, stride, 77)
    want = sum(_twin_bad(host, k * slot, lens[k], stride, 900 + k) for k in range(40))
    assert want == 600 + 50
    assert hip.hbm_admit_n(s, ext, 0, stride) == want
    got = _readback(buf)
    assert np.array_equal(got, host), np.flatnonzero(got != host)[:8]
    buf.free()
    s.destroy()


def test_hbm_rejected_arguments_name_their_entry_point(hip):
    """Every rejected call raises with the entry point's name in the text and leaves nothing held: valid calls on
    the same device succeed right afterwards."""
    st = 1 << 12
    s = hip.Stream(0)
    buf = hip.DeviceBuffer(0, 1 << 20)
    a, nb = buf.addr(0), 1 << 20
    cases = []
    for stride, base in ((8, a), (24, a), (st, a + 8)):
        cases += [("gsx_hbm_stamp", lambda stride=stride, base=base: hip.hbm_stamp(s, base, nb // 2, stride, 5)),
                  ("gsx_hbm_verify", lambda stride=stride, base=base: hip.hbm_verify(s, base, nb // 2, stride, 5)),
                  ("gsx_hbm_admit_n", lambda stride=stride, base=base:
                   hip.hbm_admit_n(s, [(a, 4096, 5), (base, nb // 2, 5)], 1, stride))]
    cases += [("gsx_hbm_stamp", lambda: hip.hbm_stamp(s, 0, nb, st, 5)),
              ("gsx_hbm_verify", lambda: hip.hbm_verify(s, 0, nb, st, 5)),
              ("gsx_hbm_admit_n", lambda: hip.hbm_admit_n(s, [(a, nb, 5), (0, nb, 6)], 1, st)),
              ("gsx_hbm_admit_n", lambda: hip.hbm_admit_n(s, [(a, nb, 5)], 2, st))]
    for name, call in cases:
        with pytest.raises(hip.HipError) as e:
            call()
        assert name + ":" in str(e.value), (name, str(e.value))
    assert hip.hbm_admit_n(s, [(a, nb, 5)], 1, st) == 0
    assert hip.hbm_verify(s, a, nb, st, 5) == 0
    assert hip.hbm_verify(s, a, nb, st, 6) == nb // st
    buf.free()
    s.destroy()
