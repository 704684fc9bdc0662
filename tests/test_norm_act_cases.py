"""CPU checks for the add + RMSNorm and SwiGLU kernels (native/kernels/norm_act.hip): the interval helper of
``tests/norm_act_cases.py`` against torch, the fp32 twin of the kernels' order against the fp64 reference within the
bound derived there, that every wrong twin fails a case, that the random cases leave few elements ambiguous, every
argument the entry points refuse, and the tools' parsers and size helpers.  No GPU: the refused calls never reach the
device."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import kv_append_cases as kc  # noqa: E402
from tests import norm_act_cases as nc  # noqa: E402


@pytest.fixture(scope="module")
def hip():
    from gpushare_scheduler_extender_amd.ops import hip as h

    h.lib()
    assert hasattr(h, "add_rmsnorm") and hasattr(h, "silu_mul"), "the bindings have no add_rmsnorm / silu_mul"
    return h


# ---- number formats and the interval -----------------------------------------------------------------------------------

def test_bf16_rounding_of_fp64_is_torchs_and_rounds_once():
    rng = np.random.default_rng(0)
    x32 = np.concatenate([(rng.standard_normal(200000) * 2.0 ** rng.integers(-100, 100, 200000)).astype(np.float32),
                          kc.bf16_value(np.arange(65536, dtype=np.uint16)),
                          np.array([0.0, -0.0, 3.3895314e38, 3.3961775e38, 3.4e38, -3.4e38, 1e-40, 2.0 ** -134,
                                    2.0 ** -133], dtype=np.float32)])
    x32 = x32[~np.isnan(x32)]
    want = torch.from_numpy(x32).to(torch.bfloat16).float().numpy()
    got = nc.bf16_round64(x32.astype(np.float64))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # a midpoint between two bf16 values goes to the even one; a value just beside it, which fp32 cannot hold, to its
    # own side: rounding through fp32 first would land on the midpoint and then on the even neighbour
    mid = 1.0 + 2.0 ** -8
    for x, w in ((mid, 1.0), (mid + 2.0 ** -40, 1.0 + 2.0 ** -7), (mid - 2.0 ** -40, 1.0), (1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -6),
                 (-(mid + 2.0 ** -40), -(1.0 + 2.0 ** -7))):
        assert float(nc.bf16_round64(x)) == w, x
    assert float(np.float32(mid + 2.0 ** -40)) == mid


def test_interval_ends_are_sorted_and_hold_the_rounded_exact_value():
    rng = np.random.default_rng(1)
    exact = rng.standard_normal(100000) * 2.0 ** rng.integers(-20, 20, 100000)
    lo, hi = nc.bf16_interval(exact, 78 * nc.U32)
    mid = nc.bf16_round64(exact)
    assert bool((lo <= mid).all() and (mid <= hi).all())
    assert 0 < float((lo != hi).mean()) < 0.01
    zlo, zhi = nc.bf16_interval(np.zeros(3), 1e-3)
    assert not zlo.any() and not zhi.any()


def test_fp64_encoder_is_the_fp32_encoder_and_rounds_once():
    rng = np.random.default_rng(2)
    x = np.concatenate([rng.uniform(-500, 500, 200000).astype(np.float32), kc.e4m3_midpoints().ravel(),
                        (rng.standard_normal(100000) * 2.0 ** rng.integers(-12, 9, 100000)).astype(np.float32),
                        np.array([0.0, -0.0, np.inf, -np.inf, 1e9], dtype=np.float32)])
    assert np.array_equal(nc.e4m3_encode64(x.astype(np.float64)), kc.e4m3_encode(x))
    assert nc.e4m3_encode64(np.array([1.0625, 1.0625 + 2.0 ** -40, 1.0625 - 2.0 ** -40])).tolist() == [0x38, 0x39, 0x38]
    v = kc.e4m3_values()
    keep = ~np.isnan(v)
    assert np.array_equal(nc.e4m3_encode64(v[keep]), np.arange(256)[keep])


def test_delta_follows_the_kernels_order():
    assert [nc.chunks_per_thread(n) for n in (8, 2040, 2048, 2056, 4096, 4104, 16384, 32768)] == \
        [1, 1, 1, 2, 2, 3, 8, 16]
    assert nc.norm_delta(8) == nc.norm_delta(2048) == 22 * 2.0 ** -24
    assert nc.norm_delta(2056) == 30 * 2.0 ** -24 and nc.norm_delta(16384) == 78 * 2.0 ** -24
    assert float(nc.silu_delta(0.0)) == 4 * 2.0 ** -23 and float(nc.silu_delta(-64.0)) == 68 * 2.0 ** -23


# ---- the twins, the reference and the cases -----------------------------------------------------------------------------

@pytest.mark.parametrize("kind", nc.KINDS)
def test_norm_twin_passes_every_case_and_few_elements_are_ambiguous(kind):
    for name, p in nc.norm_random_cases():
        nc.check_norm(p, kind, nc.norm_twin(p, kind), f"{kind}, {name}")
        frac = nc.ambiguous_fraction(kind, nc.norm_reference(p), nc.norm_delta(p.h))
        assert frac <= 0.01, (name, frac)
    for h in (8, 2048, 2056, 16384):
        p = nc.norm_one_hot(h)
        nc.check_norm(p, kind, nc.norm_twin(p, kind), f"{kind}, one-hot H{h}")
    p, y, scale = nc.norm_exact(kind)
    got = nc.norm_twin(p, kind)
    assert np.array_equal(got.y, y) and (scale is None or np.array_equal(got.scale, scale))
    nc.check_norm(p, kind, got, f"{kind}, exact")


@pytest.mark.parametrize("kind", nc.KINDS)
def test_silu_twin_passes_every_case_and_few_elements_are_ambiguous(kind):
    for name, p in nc.silu_random_cases(kind):
        nc.check_silu(p, kind, nc.silu_twin(p, kind), f"{kind}, {name}")
        exact, delta = nc.silu_reference(p)
        g, _ = nc.silu_inputs(p)
        assert float(np.abs(g).max()) <= 64 and bool(np.isfinite(exact).all())
        frac = nc.ambiguous_fraction(kind, exact, delta)
        assert frac <= 0.01, (name, frac)
    p = nc.silu_one_hot(32768 if kind == "fp8" else 16384)
    nc.check_silu(p, kind, nc.silu_twin(p, kind), f"{kind}, one-hot")
    p, y, scale = nc.silu_exact(kind)
    got = nc.silu_twin(p, kind)
    assert np.array_equal(got.y, y) and (scale is None or np.array_equal(got.scale, scale))
    nc.check_silu(p, kind, got, f"{kind}, exact")


def _fails(check, p, kind, got) -> bool:
    try:
        check(p, kind, got, "a wrong twin")
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("wrong", nc.NORM_WRONG)
def test_wrong_norm_twins_fail_a_case(wrong):
    kinds = ("fp8",) if wrong == "amax of bf16" else nc.KINDS
    for kind in kinds:
        assert any(_fails(nc.check_norm, p, kind, nc.norm_twin(p, kind, wrong)) for _, p in nc.norm_random_cases()), \
            (wrong, kind)
    if wrong in ("drop a chunk", "double a chunk"):  # the one-hot rows catch both at once: inf or NaN, or sqrt 2
        p = nc.norm_one_hot(16384)
        assert _fails(nc.check_norm, p, "bf16", nc.norm_twin(p, "bf16", wrong))


@pytest.mark.parametrize("wrong", nc.SILU_WRONG)
def test_wrong_silu_twins_fail_a_case(wrong):
    kinds = ("fp8",) if wrong == "amax of bf16" else nc.KINDS
    for kind in kinds:
        assert any(_fails(nc.check_silu, p, kind, nc.silu_twin(p, kind, wrong))
                   for _, p in nc.silu_random_cases(kind)), (wrong, kind)


def test_checks_refuse_a_stray_value_a_wrong_scale_and_a_wrong_top_code():
    _, p = nc.norm_random_cases()[2]
    got = nc.norm_twin(p, "bf16")
    got.y = got.y.copy()
    got.y[5, 77] ^= 1  # one ulp, at an element whose interval holds one value
    lo, hi = nc.bf16_interval(nc.norm_reference(p), nc.norm_delta(p.h))
    assert lo[5, 77] == hi[5, 77]
    assert _fails(nc.check_norm, p, "bf16", got)
    got = nc.norm_twin(p, "fp8")
    got.scale = got.scale * np.float32(1 + 2.0 ** -17)
    assert _fails(nc.check_norm, p, "fp8", got)
    got = nc.norm_twin(p, "fp8")
    got.y = got.y.copy()
    top = np.abs(nc.norm_reference(p)[0]).argmax()
    got.y[0, top] -= 1
    assert _fails(nc.check_norm, p, "fp8", got)
    nan = nc.norm_twin(p, "bf16")
    nan.y = nan.y.copy()
    nan.y[0, 0] = 0x7FC0
    assert _fails(nc.check_norm, p, "bf16", nan)


def test_boundary_columns_cover_the_edges():
    cols = nc.boundary_columns(16384)
    chunks = {c // 8 for c in cols}
    assert {0, 2047, 63, 64, 255, 3 * 256, 3 * 256 + 255, 4 * 256, 7 * 256 + 192} <= chunks
    assert {c % 8 for c in cols} == {0, 7} and max(cols) == 16383 and min(cols) == 0
    assert nc.boundary_columns(8) == [0] and len(set(cols)) == len(cols)
    assert {0, 4095, 15 * 256, 8 * 256 + 63, 12 * 256 - 1} <= {c // 8 for c in nc.boundary_columns(32768)}


# ---- what the entry points refuse --------------------------------------------------------------------------------------

# Addresses that are never dereferenced: every call below is refused before the first device call.
X, RI, RO, W, Y, SC, GU = (0x10000000 * i for i in range(1, 8))


class _NoStream:
    """Stands in for ``hip.Stream``: the calls under test never get as far as using one."""
    handle = None


def _norm_good(kind):
    return {"x": X, "xs": 2056, "ri": RI, "ro": RO, "rs": 2064, "w": W, "y": Y, "ys": 2072,
            "sc": SC + 4 if kind == "fp8" else 0, "m": 17, "h": 2048, "eps": 1e-5}


def _norm_call(hip, kind, v, timed=False):
    args = (_NoStream, kind, v["x"], v["xs"], v["ri"], v["ro"], v["rs"], v["w"], v["y"], v["ys"], v["sc"], v["m"],
            v["h"], v["eps"])
    return hip.time_add_rmsnorm(*args, 1) if timed else hip.add_rmsnorm(*args)


def _silu_good(kind):
    return {"gu": GU, "gs": 2 * 4096 + 8, "y": Y, "ys": 4104, "sc": SC + 4 if kind == "fp8" else 0, "m": 17, "i": 4096}


def _silu_call(hip, kind, v, timed=False):
    args = (_NoStream, kind, v["gu"], v["gs"], v["y"], v["ys"], v["sc"], v["m"], v["i"])
    return hip.time_silu_mul(*args, 1) if timed else hip.silu_mul(*args)


SCALE_RULE = "scale_out must be NULL with GSX_ACT_OUT_BF16 and non-NULL with GSX_ACT_OUT_FP8_ROW"


@pytest.mark.parametrize("timed", [False, True], ids=["launch", "timed"])
@pytest.mark.parametrize("kind", nc.KINDS)
def test_add_rmsnorm_rejects_bad_arguments_by_name(hip, kind, timed):
    good = _norm_good(kind)

    def rej(text, **kw):
        with pytest.raises(hip.HipError, match=f"gsx_add_rmsnorm: {text}"):
            _norm_call(hip, kind, {**good, **kw}, timed)

    for m in (0, -1):
        rej("need M >= 1", m=m)
    rej(SCALE_RULE, sc=SC if kind == "bf16" else 0)
    for h in (0, 4, 12, 2044, 16392, 32768, -8):
        rej("need 8 <= H <= 16384 and H % 8 == 0", h=h)
    for xs in (2040, 2052):
        rej("need x_stride >= H and x_stride % 8 == 0", xs=xs)
    for rs in (2040, 2052):
        rej("need r_stride >= H and r_stride % 8 == 0", rs=rs)
        rej("need r_stride >= H and r_stride % 8 == 0", rs=rs, ri=0)
        rej("need r_stride >= H and r_stride % 8 == 0", rs=rs, ro=0)
    for ys in (2040, 2052):
        rej("need y_stride >= H and y_stride % 8 == 0", ys=ys)
    for name in ("x", "w", "y"):
        rej("X, W and Y must not be NULL", **{name: 0})
    for name in ("x", "ri", "ro", "w", "y"):
        rej("X, R_in, R_out, W and Y must be 16-B aligned", **{name: good[name] + 8})
    if kind == "fp8":
        rej("scale_out must be 4-B aligned", sc=SC + 2)
    esz = 2 if kind == "bf16" else 1
    x_bytes, r_bytes, y_bytes = (16 * 2056 + 2048) * 2, (16 * 2064 + 2048) * 2, (16 * 2072 + 2048) * esz
    for y in (X, X + x_bytes - 16, X - y_bytes + 16, RI + r_bytes - 16, W + 4080, W - y_bytes + 16):
        rej("Y must not overlap X, R_in or W", y=y)
    for ro in (X + 16, X - r_bytes + 16, W, Y + y_bytes - 16, RI + 16, RI - 16):
        rej("R_out must not overlap X, W, Y or scale_out, nor R_in unless it is R_in", ro=ro)
    if kind == "fp8":
        rej("R_out must not overlap X, W, Y or scale_out, nor R_in unless it is R_in", ro=SC - r_bytes + 16)
        for sc in (X + 4, RI + r_bytes - 4, W + 4092, Y - 17 * 4 + 4):
            rej("scale_out must not overlap X, R_in, W or Y", sc=sc)
    for eps in (-1e-6, float("inf"), float("nan")):
        rej("eps must be finite and >= 0", eps=eps)


def test_add_rmsnorm_accepts_what_lies_next_to_a_refusal(hip):
    """Buffers that only touch, R_out == R_in, and a missing R_in or R_out whose stride is then not looked at: checked
    through the one refusal that comes after the overlap rules."""
    good = _norm_good("bf16")
    x_bytes, r_bytes, y_bytes = (16 * 2056 + 2048) * 2, (16 * 2064 + 2048) * 2, (16 * 2072 + 2048) * 2
    for kw in ({"y": X + x_bytes}, {"y": X - y_bytes}, {"ro": RI}, {"ro": X + x_bytes}, {"ro": Y - r_bytes},
               {"ri": 0}, {"ro": 0}, {"ri": 0, "ro": 0, "rs": 3}):
        with pytest.raises(hip.HipError, match="gsx_add_rmsnorm: eps must be finite and >= 0"):
            _norm_call(hip, "bf16", {**good, **kw, "eps": -1.0})


@pytest.mark.parametrize("timed", [False, True], ids=["launch", "timed"])
@pytest.mark.parametrize("kind", nc.KINDS)
def test_silu_mul_rejects_bad_arguments_by_name(hip, kind, timed):
    good = _silu_good(kind)

    def rej(text, **kw):
        with pytest.raises(hip.HipError, match=f"gsx_silu_mul: {text}"):
            _silu_call(hip, kind, {**good, **kw}, timed)

    rej("need M >= 1", m=0)
    rej(SCALE_RULE, sc=SC if kind == "bf16" else 0)
    for i in (0, 4, 12, 4092, -8):
        rej("need I >= 8 and I % 8 == 0", i=i)
    if kind == "fp8":
        rej("need I <= 32768 with GSX_ACT_OUT_FP8_ROW", i=32776, gs=65552, ys=32776)
        rej("scale_out must be 4-B aligned", sc=SC + 2)
    for gs in (8184, 4096, 8196):
        rej("need gu_stride >= 2 I and gu_stride % 8 == 0", gs=gs)
    for ys in (4088, 4100):
        rej("need y_stride >= I and y_stride % 8 == 0", ys=ys)
    for name in ("gu", "y"):
        rej("GU and Y must not be NULL", **{name: 0})
        rej("GU and Y must be 16-B aligned", **{name: good[name] + 8})
    esz = 2 if kind == "bf16" else 1
    gu_bytes, y_bytes = (16 * 8200 + 8192) * 2, (16 * 4104 + 4096) * esz
    for y in (GU, GU + gu_bytes - 16, GU - y_bytes + 16):
        rej("Y must not overlap GU", y=y)
    if kind == "fp8":
        for sc in (GU + 4, Y + y_bytes - 4, Y - 17 * 4 + 4):
            rej("scale_out must not overlap GU or Y", sc=sc)
        with pytest.raises(hip.HipError, match="gsx_silu_mul: need M >= 1"):  # 32768 itself is taken
            _silu_call(hip, kind, {**good, "i": 32768, "gs": 65536, "ys": 32768, "m": 0}, timed)
    else:  # no such limit without a row reduction
        with pytest.raises(hip.HipError, match="gsx_silu_mul: need M >= 1"):
            _silu_call(hip, kind, {**good, "i": 1 << 20, "gs": 1 << 21, "ys": 1 << 20, "m": 0}, timed)


def test_unknown_out_kind_is_rejected_by_name(hip):
    L = hip.lib()
    for kind in (-1, 2, 7):
        for fn, tail in ((L.gsx_add_rmsnorm, []), (L.gsx_event_time_add_rmsnorm, [1, None])):
            rc = fn(None, kind, X, 2048, RI, RO, 2048, W, Y, 2048, None, 3, 2048, 1e-5, *tail)
            assert rc != 0 and L.gsx_last_error().decode() == f"gsx_add_rmsnorm: unknown out_kind {kind}"
        for fn, tail in ((L.gsx_silu_mul, []), (L.gsx_event_time_silu_mul, [1, None])):
            rc = fn(None, kind, GU, 8192, Y, 4096, None, 3, 4096, *tail)
            assert rc != 0 and L.gsx_last_error().decode() == f"gsx_silu_mul: unknown out_kind {kind}"
    assert hip.ACT_OUT_KINDS == {"bf16": 0, "fp8": 1}
    for timed in (False, True):
        with pytest.raises(ValueError, match="output kind 'fp4'"):
            _norm_call(hip, "fp4", _norm_good("bf16"), timed)
        with pytest.raises(ValueError, match="output kind 'fp4'"):
            _silu_call(hip, "fp4", _silu_good("bf16"), timed)


# ---- the tools -------------------------------------------------------------------------------------------------------

def test_workload_and_isolation_parsers_take_the_layer_workload():
    from gsxtools import isolation, workload

    for mod in (workload, isolation):
        ap = mod.build_parser()
        d = ap.parse_args(["--workload", "layer"])
        assert (d.workload, d.batch, d.context, d.heads, d.kv_heads, d.kv_dtype, d.page, d.ffn) == \
            ("layer", 8, 8192, 64, 8, "bf16", 16, None)
        assert ap.parse_args(["--workload", "layer", "--batch", "16", "--ffn", "28672"]).ffn == 28672
        for bad in (["--workload", "layer", "--batch", "0"], ["--workload", "layer", "--batch", "17"]):
            with pytest.raises(SystemExit):
                ap.parse_args(bad)
    a = isolation.build_parser().parse_args(["--workload", "layer", "--kv-dtype", "fp8", "--kv-gib", "2",
                                             "--weights-gib", "1", "--ffn", "1024"])
    line = isolation.layer_cmdline(a)
    got = workload.build_parser().parse_args(["--workload", "layer", *line])
    assert (got.kv_dtype, got.kv_gib, got.weights_gib, got.heads, got.ffn) == ("fp8", 2.0, 1.0, 64, 1024)
    assert "--ffn" not in isolation.layer_cmdline(isolation.build_parser().parse_args(["--workload", "layer"]))
    assert isolation.SCENARIOS_LAYER == isolation.SCENARIOS_SERVER
    with pytest.raises(SystemExit, match="--workload layer: scenario noisy is not one of"):
        isolation.main(["--workload", "layer", "--scenarios", "noisy"])
    # the server workload is as it was
    assert workload.build_parser().parse_args(["--workload", "server"]).workload == "server"


def test_layer_workload_sizes():
    from gsxtools import workload as wl

    assert [wl.default_ffn(h) for h in (1024, 4096, 8192, 5120, 128)] == [3584, 14336, 28672, 17920, 448]
    assert all(wl.default_ffn(h) % 64 == 0 for h in range(128, 16385, 128))
    # bf16 weights of one layer: the server layer's two projections, gate and up [2 ffn][hidden], down [hidden][ffn]
    assert wl.layer_weight_bytes(64, 8, 28672) == \
        wl.server_layer_weight_bytes(64, 8) + (2 * 28672 * 8192 + 8192 * 28672) * 2
    assert wl.layer_weight_bytes(8, 2, 3584) == ((8 + 4) * 128 * 1024 + 1024 * 1024 + 3 * 3584 * 1024) * 2
    # the MLP holds two thirds of a layer's weights and more
    assert wl.layer_weight_bytes(64, 8, 28672) > 3 * wl.server_layer_weight_bytes(64, 8)
