"""The compute pre-flight on a real MI355X (run with ``-m gpu``): every wave of a clean launch answers what the NumPy
twin computes, every CU and SIMD is reached, and a value flipped on one physical CU (or one SIMD of it) is reported
for exactly that CU, SIMD and unit -- through the library and through ``gsx-cutest``."""
import json
import subprocess
from pathlib import Path

import pytest

torch = pytest.importorskip("torch")

from gpushare_scheduler_extender_amd.ops import cutest as ct  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
TOOL = ROOT / "gpushare_scheduler_extender_amd" / "_native" / "gsx-cutest"
SEEDS = (0, 1, 2)
NUNITS = len(ct.UNITS)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    from gpushare_scheduler_extender_amd.ops import hip as h

    assert h.SO.exists()
    return h


@pytest.fixture(scope="module")
def twin():
    return {s: [ct.expected_signature(u, s) for u in range(NUNITS)] for s in SEEDS}


@pytest.fixture(scope="module")
def clean(hip):
    """Three clean launches of 4 workgroups per CU on the whole GPU: ``(stream, blocks, {seed: records})``."""
    s = hip.Stream(0)
    blocks = 4 * hip.device_info(0)["cu_count"]
    yield s, blocks, {seed: hip.cutest_launch(s, seed, blocks) for seed in SEEDS}
    s.destroy()


def _targets(clean):
    """Two physical CUs of the clean run: the third in sorted order and the last."""
    cus = sorted({r.where() for r in clean[2][SEEDS[0]]})
    return cus[2], cus[-1]


def test_clean_launch_matches_the_twin_on_every_cu(hip, clean, twin):
    s, blocks, by_seed = clean
    cu_count = hip.device_info(0)["cu_count"]
    rep = hip.CutestReport()
    for seed, recs in by_seed.items():
        assert len(recs) == 4 * blocks
        wrong = [(i, u) for i, r in enumerate(recs) for u in range(NUNITS) if r.sig[u] != twin[seed][u]]
        assert not wrong, (seed, wrong[:8], [hex(x) for x in recs[wrong[0][0]].sig], [hex(x) for x in twin[seed]])
        assert all(r.fail_mask == 0 and r.seed == seed for r in recs)
        hip.cutest_aggregate(recs, rep)
    assert rep.waves == 3 * 4 * blocks and rep.bad_waves == 0 and rep.bad_cus == 0 and rep.n_bad == 0
    assert rep.cus_seen == cu_count
    print("after 3 launches: CUs covered", rep.cus_covered, "SIMDs seen", rep.simds_seen)
    run, seconds = hip.cutest_run(s, "quick")
    print("quick:", run.launches, "launches,", f"{seconds:.3f}s; covered", run.cus_covered, "of", run.cus_expected)
    assert run.bad_waves == 0 and run.cus_seen == cu_count and run.cus_expected == cu_count
    cus = run.cus()
    assert len(cus) == cu_count and all(c.simds == 0xF for c in cus.values())
    assert run.covered == 1 and run.cus_covered == cu_count
    assert ct.SEEDS["quick"] <= run.launches <= ct.SEEDS["quick"] + ct.EXTRA_LAUNCHES


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("unit", range(NUNITS), ids=ct.UNITS)
def test_injection_is_reported_for_exactly_that_cu_and_unit(hip, clean, twin, unit, which):
    s, blocks, _ = clean
    target = _targets(clean)[which]
    seed = SEEDS[unit % len(SEEDS)]
    recs = hip.cutest_launch(s, seed, blocks, (*target, -1, unit, 0x00410000))
    rep = hip.cutest_aggregate(recs)
    cus = rep.cus()
    there = cus[target]
    assert rep.bad_cus == 1 and rep.n_bad == 1
    assert there.waves > 0 and there.bad_waves == there.waves == rep.bad_waves
    assert there.fail_mask == 1 << unit and there.bad_simds == there.simds
    assert all(c.fail_mask == 0 and c.bad_waves == 0 for where, c in cus.items() if where != target)
    (bad,) = rep.bad_entries()
    assert (bad.xcc, bad.se, bad.sh, bad.cu) == target and bad.units == 1 << unit and bad.unit == unit
    assert bad.expected == twin[seed][unit] and bad.got ^ bad.expected
    # only that unit's signature moved
    for r in recs:
        for u in range(NUNITS):
            assert (r.sig[u] != twin[seed][u]) == (r.where() == target and u == unit)


def test_injection_with_a_simd_selector_marks_only_that_simd(hip, clean):
    s, blocks, _ = clean
    target = _targets(clean)[1]
    recs = hip.cutest_launch(s, SEEDS[1], blocks, (*target, 2, ct.UNIT_IDS["MFMA_BF16_16"], 1))
    bad = [r for r in recs if r.fail_mask]
    assert bad and all(r.where() == target and r.simd == 2 for r in bad)
    assert len(bad) == sum(1 for r in recs if r.where() == target and r.simd == 2)
    rep = hip.cutest_aggregate(recs)
    assert rep.bad_cus == 1 and rep.bad_entries()[0].simds == 1 << 2 and rep.cus()[target].bad_simds == 1 << 2
    assert rep.bad_waves == len(bad) < rep.cus()[target].waves


def test_masked_stream_tests_its_64_cus(hip, clean):
    full = {r.where() for r in clean[2][SEEDS[0]]}
    m = hip.Stream(0, hip.mask_words(range(0, 64)))
    try:
        rep, _seconds = hip.cutest_run(m, "quick")
    finally:
        m.destroy()
    assert rep.cus_seen == 64 and set(rep.cus()) <= full
    assert rep.cus_expected == 64 and rep.covered == 1 and rep.cus_covered == 64
    assert rep.bad_waves == 0 and rep.bad_cus == 0


def test_full_level_is_clean_on_the_whole_gpu(hip, clean):
    """All 256 seeds of ``full``: a false positive at any of them would take a healthy GPU out of service."""
    s, _blocks, _ = clean
    cu_count = hip.device_info(0)["cu_count"]
    run, seconds = hip.cutest_run(s, "full")
    print("full:", run.launches, "launches,", f"{seconds:.3f}s; covered", run.cus_covered, "of", run.cus_expected)
    assert run.bad_waves == 0 and run.bad_cus == 0 and run.n_bad == 0
    assert run.cus_seen == run.cus_expected == cu_count
    assert run.covered == 1 and run.cus_covered == cu_count
    assert ct.SEEDS["full"] == 256 and 256 <= run.launches <= 256 + ct.EXTRA_LAUNCHES


def _tool(*argv):
    r = subprocess.run([str(TOOL), *argv], capture_output=True, text=True, timeout=120)
    return r.returncode, json.loads(r.stdout.strip().splitlines()[-1])


def test_tool_clean_run(hip):
    rc, out = _tool("--device", "0", "--expect-cus", str(hip.device_info(0)["cu_count"]))
    print(out)
    assert rc == 0 and out["error"] is None and out["covered"] is True and not out["truncated"]
    assert out["bad_waves"] == 0 and out["bad_cus"] == [] and out["units_failed"] == []
    assert out["cus_seen"] == out["cus_expected"] == hip.device_info(0)["cu_count"] and out["launches"] >= 8


def test_tool_truncated_before_its_first_launch():
    rc, out = _tool("--device", "0", "--max-seconds", "0.000001")
    assert rc == 0 and out["error"] is None, out
    assert out["truncated"] is True and out["launches"] == 0 and out["covered"] is False and out["waves"] == 0


MASK64 = "0xffffffff,0xffffffff"


def test_tool_on_a_masked_stream_expects_the_mask():
    rc, out = _tool("--device", "0", "--cu-mask", MASK64)
    assert rc == 0 and out["error"] is None and out["covered"] is True and not out["truncated"], out
    assert out["cus_expected"] == out["cus_seen"] == out["cus_covered"] == 64 and out["bad_waves"] == 0
    assert 8 <= out["launches"] <= 16


def test_tool_whose_coverage_stays_short_uses_every_extra_launch(hip):
    rc, out = _tool("--device", "0", "--cu-mask", MASK64, "--expect-cus", str(hip.device_info(0)["cu_count"]))
    assert rc == 2 and "--expect-cus" in out["error"], out
    assert out["covered"] is False and not out["truncated"] and out["bad_waves"] == 0
    assert out["launches"] == ct.SEEDS["quick"] + ct.EXTRA_LAUNCHES == 16


def test_tool_and_library_run_the_same_loop(hip, clean):
    cu_count = hip.device_info(0)["cu_count"]
    rc, out = _tool("--device", "0")
    assert rc == 0 and out["error"] is None and not out["truncated"], out
    run, _seconds = hip.cutest_run(clean[0], "quick")
    assert out["waves"] == 16 * cu_count * out["launches"] and run.waves == 16 * cu_count * run.launches
    assert out["cus_covered"] == run.cus_covered


def test_tool_names_the_injected_cu(clean):
    xcc, se, sh, cu = _targets(clean)[0]
    rc, out = _tool("--device", "0", "--inject", f"{xcc}:{se}:{sh}:{cu}:LDS:0x80")
    assert rc == 1 and out["error"] is None and out["bad_cu_count"] == 1 and out["units_failed"] == ["LDS"]
    (bad,) = out["bad_cus"]
    assert (bad["xcc"], bad["se"], bad["sh"], bad["cu"]) == (xcc, se, sh, cu) and bad["units"] == ["LDS"]
    assert bad["expected"] != bad["got"] and out["bad_waves"] > 0
