"""Device health and partition handling of the device plugin against the native fake amdsmi backend (VERDICT r2
#7): uncorrectable ECC / RAS / xGMI errors make a GPU's IDs Unhealthy in ListAndWatch within one poll, thermal
throttling is exported without taking the GPU away, a reset event marks it Unhealthy, and a runtime compute /
memory partition change re-advertises a new ID set and re-publishes the per-device totals."""
import asyncio
import json

from gpushare_scheduler_extender_amd.deviceplugin.devices import Device, apply_memory_pools
from gpushare_scheduler_extender_amd.deviceplugin.plugin import GpuSharePlugin, device_tags
from gsxtools.kubeletapi import PluginClient
from gpushare_scheduler_extender_amd.k8s.client import KubeClient
from tests.fixtures.fakeapi import FakeApiServerRunner
from gpushare_scheduler_extender_amd.k8s.objects import make_node
from gpushare_scheduler_extender_amd.models.profile import NODE_DEVICE_MEMORY_ANNOTATION, SHARED_GPU
from gpushare_scheduler_extender_amd.ops import mxdev


def test_native_fake_backend_fault_injection():
    s = mxdev.native().Session("fake:2x288GB")  # a session of its own (not the cached one)
    h = s.health(1)
    assert h["healthy"] and h["reason"] == "" and h["partition"] == "SPX"
    s.inject(1, "ras_xgmi_uncorrectable=2")
    h = s.health(1)
    assert not h["healthy"] and "xGMI uncorrectable=2" in h["reason"]
    s.inject(0, "thermal_throttle=1")
    h0 = s.health(0)
    assert h0["healthy"] and h0["thermal_throttle"]  # throttling slows a pod, it does not corrupt it
    s.inject(0, "xgmi_error=2")
    assert "xGMI multiple errors" in s.health(0)["reason"]
    s.inject(0, "partition=CPX")
    devs = s.devices()
    assert len(devs) == 16 and {d["partition"] for d in devs} == {"CPX"}
    s.inject(0, "memory_partition=NPS2")
    assert {d["memory_partition"] for d in s.devices()} == {"NPS2"}
    s.watch_events()
    s.inject(3, "event=GPU_PRE_RESET")
    ev = s.poll_events(1000)
    assert ev and ev[0]["name"] == "GPU_PRE_RESET" and ev[0]["index"] == 3


def test_plugin_health_and_partition_change(sock_dir):
    backend = "fake:2x64GiB"

    async def go():
        api = await FakeApiServerRunner().start()
        c = KubeClient(api.url)
        await c.create("nodes", make_node("n", 128, 2))
        devs = apply_memory_pools([Device(**d) for d in mxdev.enumerate_devices(backend)])
        plugin = GpuSharePlugin(KubeClient(api.url), "n", devs, SHARED_GPU, socket_dir=str(sock_dir / "dp"),
                                health_backend=backend, health_interval=0.05)
        await plugin.start(register=False)
        cl = PluginClient(plugin.socket_path)
        stream = cl.list_and_watch()
        try:
            first = await asyncio.wait_for(stream.read(), 5)
            assert len(first.devices) == 128 and all(d.health == "Healthy" for d in first.devices)

            async def next_list():
                return await asyncio.wait_for(stream.read(), 5)

            mxdev.inject(1, "ras_umc_uncorrectable=1", backend)  # an HBM uncorrectable error on GPU 1
            upd = await next_list()
            bad = {d.ID.split("-_-")[0] for d in upd.devices if d.health == "Unhealthy"}
            assert bad == {device_tags(devs)[1]}, bad
            mxdev.inject(0, "thermal_throttle=1", backend)
            await asyncio.sleep(0.3)
            metrics = plugin.metrics_text()
            assert 'gpushare_plugin_device_thermal_throttle{device="0"} 1' in metrics
            assert 'gpushare_plugin_device_ras_uncorrectable{device="1"} 1' in metrics
            assert plugin.devices[0].healthy  # throttled, still schedulable
            # the node is re-partitioned at run time: 2 GPUs in DPX -> 4 logical devices of 32 GiB
            mxdev.inject(0, "partition=DPX", backend)
            upd = await next_list()
            while len({d.ID.split("-_-")[0] for d in upd.devices}) != 4:
                upd = await next_list()
            assert len(upd.devices) == 4 * 32
            for _ in range(100):
                node = await c.get("nodes", "n")
                if node["metadata"]["annotations"].get(NODE_DEVICE_MEMORY_ANNOTATION) == "32,32,32,32":
                    break
                await asyncio.sleep(0.05)
            assert node["metadata"]["annotations"][NODE_DEVICE_MEMORY_ANNOTATION] == "32,32,32,32"
            inv = json.loads(node["metadata"]["annotations"]["gpushare.amd.com/devices"])
            assert [d["partition"] for d in inv] == ["DPX"] * 4
            assert plugin.stats["layout_changes"] == 1
        finally:
            stream.cancel()
            await cl.close()
            await plugin.stop()
            await plugin.client.close()
            await c.close()
            await api.stop()
    asyncio.run(go())
