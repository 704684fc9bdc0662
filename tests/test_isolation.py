"""Enforced isolation, CPU side: the library against a fake HSA runtime, and the plugin's per-pod files and
mounts (the GPU behaviour is tests/test_gpu_isolate.py)."""
import asyncio
import json
import os
import subprocess
from pathlib import Path

from gpushare_scheduler_extender_amd.deviceplugin.allocator import CUPartitioner
from gpushare_scheduler_extender_amd.deviceplugin.isolation import CONTAINER_DIR, IsolationManager, config_text

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "gpushare_scheduler_extender_amd" / "_native" / "libgsx_isolate.so"


def test_library_against_fake_hsa_runtime(tmp_path):
    from gpushare_scheduler_extender_amd.utils.build import build_native

    build_native(["isolate"])
    r = subprocess.run([str(ROOT / "build" / "isolate_test"), str(LIB), str(tmp_path)], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0 and "isolate_test: OK" in r.stdout, r.stderr


def test_config_text_words_match_the_cu_mask_annotation():
    cus = CUPartitioner(256, 8).allocate("u", 64)
    t = config_text(cus, 256, 64 << 30)
    words = [int(w, 16) for w in t.split("cu_mask=")[1].split("\n")[0].split(",")]
    assert len(words) == 8 and sum(bin(w).count("1") for w in words) == 64
    assert all(bin(w).count("1") == 8 for w in words)  # 8 CUs on each XCD (32-CU block)
    assert f"hbm_limit_bytes={64 << 30}" in t and f"ledger={CONTAINER_DIR}/hbm.ledger" in t


def test_manager_files_mounts_and_release(tmp_path):
    m = IsolationManager(str(tmp_path / "iso"), library=str(LIB))
    mounts, envs = m.prepare("uid-1", [0, 1, 2], 256, 8 << 30)
    paths = {x["container_path"]: x for x in mounts}
    assert paths["/etc/ld.so.preload"]["read_only"] and paths[f"{CONTAINER_DIR}/isolation.conf"]["read_only"]
    assert not paths[f"{CONTAINER_DIR}/hbm.ledger"]["read_only"]  # every process of the pod writes its slot
    assert envs["HSA_TOOLS_LIB"] == f"{CONTAINER_DIR}/libgsx_isolate.so"
    assert Path(paths["/etc/ld.so.preload"]["host_path"]).read_text().strip() == f"{CONTAINER_DIR}/libgsx_isolate.so"
    conf = Path(paths[f"{CONTAINER_DIR}/isolation.conf"]["host_path"])
    assert oct(conf.stat().st_mode & 0o777) == "0o444" and "hbm_limit_bytes=8589934592" in conf.read_text()
    assert os.path.getsize(paths[f"{CONTAINER_DIR}/libgsx_isolate.so"]["host_path"]) > 0
    # host processes: no mounts, host paths in env
    mounts2, envs2 = m.prepare("uid-2", None, 256, 4 << 30, host_process=True)
    assert mounts2 == [] and Path(envs2["GSX_ISOLATION_CONFIG"]).exists()
    assert "cu_mask" not in Path(envs2["GSX_ISOLATION_CONFIG"]).read_text()
    m.release("uid-1")
    assert not m.pod_dir("uid-1").exists() and m.pod_dir("uid-2").exists()
    assert m.gc({"uid-3"}) == 1 and not m.pod_dir("uid-2").exists()


def test_plugin_allocate_mounts_isolation_and_records(tmp_path, sock_dir):
    """The gRPC Allocate answers the isolation mounts, and the record of the allocation is checkpointed."""
    from gpushare_scheduler_extender_amd.deviceplugin.devices import Device
    from gpushare_scheduler_extender_amd.deviceplugin.plugin import GpuSharePlugin
    from gsxtools.kubeletapi import PluginClient
    from gpushare_scheduler_extender_amd.k8s.client import KubeClient
    from tests.fixtures.fakeapi import FakeApiServerRunner
    from gpushare_scheduler_extender_amd.k8s.objects import make_node, make_pod
    from gpushare_scheduler_extender_amd.models.profile import SHARED_GPU

    async def go():
        api = await FakeApiServerRunner().start()
        c = KubeClient(api.url)
        await c.create("nodes", make_node("n", 16, 1))
        ann = {SHARED_GPU.annotation_idx: "0", SHARED_GPU.annotation_dev: "16", SHARED_GPU.annotation_pod: "4",
               SHARED_GPU.annotation_assigned: "false", SHARED_GPU.annotation_assume_time: "1",
               "gpushare.amd.com/cu-count": "64"}
        pod = await c.create("pods", make_pod("a", 4, node="n", annotations=ann))
        iso = IsolationManager(str(tmp_path / "iso"), library=str(LIB))
        plugin = GpuSharePlugin(KubeClient(api.url), "n", [Device(index=0, total_bytes=16 << 30)], SHARED_GPU,
                                socket_dir=str(sock_dir / "dp"), isolation=iso)
        await plugin.start(register=False, publish=False)
        cl = PluginClient(plugin.socket_path)
        try:
            r = (await cl.allocate([[f"gpu0-_-{i}" for i in range(4)]])).container_responses[0]
            mounts = {m.container_path: m for m in r.mounts}
            assert set(mounts) == {"/run/gsx/isolation.conf", "/run/gsx/hbm.ledger", "/run/gsx/libgsx_isolate.so",
                                   "/etc/ld.so.preload"}
            conf = Path(mounts["/run/gsx/isolation.conf"].host_path).read_text()
            assert "cu_mask=" in conf and f"hbm_limit_bytes={4 << 30}" in conf
            assert r.envs["HSA_TOOLS_LIB"] == "/run/gsx/libgsx_isolate.so"
            assert len(plugin.state.records) == 1
            import json
            for _ in range(100):  # the checkpoint write is debounced (one write per burst of Allocates)
                if Path(plugin.checkpoint).exists():
                    break
                await asyncio.sleep(0.02)
            saved = json.loads(Path(plugin.checkpoint).read_text())["records"]
            assert saved[0]["uid"] == pod["metadata"]["uid"] and len(saved[0]["ids"]) == 4
            # the pod goes away: its record and its isolation files go with it
            await c.delete("pods", "a", "default")
            for _ in range(100):
                if not plugin.state.records and not iso.pod_dir(pod["metadata"]["uid"]).exists():
                    break
                await asyncio.sleep(0.02)
            assert not plugin.state.records and not iso.pod_dir(pod["metadata"]["uid"]).exists()
        finally:
            await cl.close()
            await plugin.stop()
            await plugin.client.close()
            await c.close()
            await api.stop()
    asyncio.run(go())


def test_library_loads_into_any_container_userland():
    """ld.so skips a preload that fails to load with only a warning, and the container image's userland is not
    ours: the library may need nothing but libc, and no glibc symbol version newer than 2.17 (CentOS 7 /
    Ubuntu 18.04 era); no libstdc++ (whose GLIBCXX versions would tie it to this build host's GCC)."""
    import re
    import shutil
    import subprocess

    objdump = shutil.which("objdump") or "/opt/rocm/lib/llvm/bin/llvm-objdump"
    p = subprocess.run([objdump, "-p", str(LIB)], capture_output=True, text=True, check=True).stdout
    needed = set(re.findall(r"NEEDED\s+(\S+)", p))
    assert needed <= {"libc.so.6", "ld-linux-x86-64.so.2"}, needed
    t = subprocess.run([objdump, "-T", str(LIB)], capture_output=True, text=True, check=True).stdout
    assert "GLIBCXX" not in t and "CXXABI" not in t
    versions = {tuple(int(x) for x in v.split(".")) for v in re.findall(r"GLIBC_(\d+\.\d+(?:\.\d+)?)", t)}
    assert versions and max(versions) <= (2, 17), sorted(versions)
    exported = {ln.split()[-1] for ln in t.splitlines() if " g " in ln and ".text" in ln}
    assert exported == {"OnLoad", "OnUnload", "gsx_isolate_stats", "gsx_isolate_scratch", "gsx_isolate_scratch_queues",
                        "hsa_init"}, exported


def test_hsa_init_puts_the_tools_library_back(tmp_path):
    """VERDICT r3 missing 4: ROCr reads HSA_TOOLS_LIB at hsa_init.  Preloaded, the library's own hsa_init runs first
    (it precedes libhsa-runtime64 in the global scope), puts itself back into HSA_TOOLS_LIB whatever the process did
    to its environment, and forwards to the runtime's hsa_init (found without libdl).  CPU-only: no GPU here, so the
    runtime's own status is compared with the status it gives unconfined."""
    import subprocess
    import sys

    conf = tmp_path / "isolation.conf"
    conf.write_text("cu_mask=0x000000ff\nhbm_limit_bytes=1073741824\n")
    code = (
        "import ctypes, json, os\n"
        "ctypes.CDLL('/opt/rocm/lib/libhsa-runtime64.so.1', mode=os.RTLD_NOW | os.RTLD_GLOBAL)\n"
        "libc = ctypes.CDLL(None)\n"
        "libc.getenv.restype = ctypes.c_char_p\n"
        "before = libc.getenv(b'HSA_TOOLS_LIB')\n"
        "os.environ.pop('HSA_TOOLS_LIB', None)\n"  # the process drops it before its first HSA call
        "dropped = libc.getenv(b'HSA_TOOLS_LIB')\n"
        "st = ctypes.CDLL(None).hsa_init()\n"  # global lookup: the preloaded definition first
        "after = libc.getenv(b'HSA_TOOLS_LIB')\n"
        "print(json.dumps({'before': (before or b'').decode(), 'dropped': (dropped or b'').decode(),\n"
        "                  'after': (after or b'').decode(), 'status': st}))\n")
    env = {k: v for k, v in os.environ.items() if k not in ("HSA_TOOLS_LIB", "LD_PRELOAD")}
    plain = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0, plain.stderr[-2000:]
    ref = json.loads(plain.stdout.strip().splitlines()[-1])
    env.update(LD_PRELOAD=str(LIB), GSX_ISOLATION_CONFIG=str(conf))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert str(LIB) in out["before"] and out["dropped"] == "", out  # the constructor set it; the process dropped it
    assert str(LIB) in out["after"], out  # hsa_init put it back before the runtime read it
    assert out["status"] == ref["status"], (out, ref)  # and the runtime's own hsa_init ran
