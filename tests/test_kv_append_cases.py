"""CPU checks for the RoPE + KV append (native/kernels/kv_append.hip): the e4m3 encoder of ``tests/kv_append_cases.py``
against torch, the NumPy twin against an fp64 reference within the bound derived there, the properties of the
addressing cases, that wrong twins change a case, every argument the entry points refuse and the binding's argument
handling, and the tools' parsers.  No GPU: the refused calls never reach the device."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import kv_append_cases as kc  # noqa: E402


@pytest.fixture(scope="module")
def hip():
    from gpushare_scheduler_extender_amd.ops import hip as h

    h.lib()
    assert hasattr(h, "kv_append"), "the bindings have no kv_append"
    return h


# ---- number formats --------------------------------------------------------------------------------------------------

def _torch_e4m3(x: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def test_encoder_is_torchs_up_to_448_and_saturates_above():
    """On every value of magnitude <= 448 tried (random ones, every bf16 code, all 126 midpoints between neighbouring
    codes with their fp32 neighbours on either side, both signs) the encoder is ``torch.Tensor.to(float8_e4m3fn)``.
    Above 448 the two DIFFER, and that is the point of the kernel: torch's cast gives NaN from 465 on, the contract
    saturates."""
    rng = np.random.default_rng(0)
    mids = kc.e4m3_midpoints()
    assert mids.shape == (2, 126, 3) and bool((np.abs(mids[:, :, 0]) < np.abs(mids[:, :, 1])).all())
    x = np.concatenate([rng.uniform(-448, 448, 300000).astype(np.float32),
                        (rng.standard_normal(300000) * 2.0 ** rng.integers(-12, 9, 300000)).astype(np.float32),
                        mids.ravel(), kc.bf16_value(np.arange(65536, dtype=np.uint16)),
                        np.array([0.0, -0.0, 448.0, -448.0, 2.0 ** -9, 2.0 ** -10, -2.0 ** -10], dtype=np.float32)])
    x = x[np.abs(x) <= 448]
    assert len(x) > 600000
    bad = np.nonzero(kc.e4m3_encode(x) != _torch_e4m3(x))[0]
    assert len(bad) == 0, (len(bad), x[bad[:5]])
    # a midpoint goes to the even code, its neighbours to either side
    codes = kc.e4m3_encode(mids[0])
    assert bool((codes[:, 0] + 1 == codes[:, 2]).all()) and bool((codes[:, 1] % 2 == 0).all())
    over = np.array([449, 464, 465, 1e9, np.inf, -449, -465, -np.inf], dtype=np.float32)
    assert kc.e4m3_encode(over).tolist() == [0x7E] * 5 + [0xFE] * 3
    assert (_torch_e4m3(over[2:5]) & 0x7F).tolist() == [0x7F] * 3  # torch: NaN
    nan = kc.e4m3_encode(np.array([np.nan, -np.nan], dtype=np.float32))
    assert bool(kc.same_e4m3(nan, [0x7F, 0x7F]).all())
    # the decoder of the format inverts the encoder on every code that is no NaN
    v = kc.e4m3_values()
    keep = ~np.isnan(v)
    assert np.array_equal(kc.e4m3_encode(v[keep].astype(np.float32)), np.arange(256)[keep])


def test_bf16_rounding_is_torchs():
    rng = np.random.default_rng(1)
    x = np.concatenate([(rng.standard_normal(200000) * 2.0 ** rng.integers(-30, 30, 200000)).astype(np.float32),
                        np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 0.0, -0.0, np.inf,
                                  3.3895e38], dtype=np.float32)])
    want = torch.from_numpy(x).bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(kc.bf16_bits(x), want)
    assert kc.bf16_bits(np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8], dtype=np.float32)).tolist() == [0x3F80, 0x3F82]
    assert np.array_equal(kc.bf16_bits(kc.bf16_value(np.arange(65536, dtype=np.uint16))), np.arange(65536))


# ---- the twin --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", kc.KINDS)
def test_twin_is_inside_the_bound_of_the_fp64_reference(kind):
    for name, p in kc.rotation_cases(kind) + [("cancellation", kc.cancellation_problem(kind))]:
        got = kc.twin(p)
        rot, v, mag = kc.reference64(p)
        live = [n for n, _, _ in p.live()]
        assert live, name
        # Q_out is bf16 whatever the cache
        q = kc.bf16_value(got.q_out).astype(np.float64)
        target, bound = kc.error_bound(rot[:, :p.hq], mag[:, :p.hq], "bf16")
        assert bool((np.abs(q - target)[live] <= bound[live]).all()), name
        for n, pp, slot in p.live():
            krow, vrow = got.k[kc.GUARD + pp, :, slot], got.v[kc.GUARD + pp, :, slot]
            if kind == "bf16":
                kv, vv = kc.bf16_value(krow).astype(np.float64), kc.bf16_value(vrow).astype(np.float64)
            else:
                kv, vv = kc.e4m3_values()[krow], kc.e4m3_values()[vrow]
            target, bound = kc.error_bound(rot[n, p.hq:], mag[n, p.hq:], kind, p.k_inv)
            assert bool((np.abs(kv - target) <= bound).all()), (name, n)
            target, bound = kc.error_bound(v[n], np.abs(v[n]), kind, p.v_inv, ops=0)
            assert bool((np.abs(vv - target) <= (bound if kind == "fp8" else 0)).all()), (name, n)


def _written(p, r):
    fill = kc.POISON16 if p.kind == "bf16" else kc.POISON8
    return {(int(a), int(c)) for a, _, c, _ in np.argwhere(r.k != fill)}


@pytest.mark.parametrize("kind", kc.KINDS)
def test_addressing_cases_have_the_properties_they_are_there_for(kind):
    cases = kc.addressing_cases(kind) + kc.dropped_page_cases(kind)
    assert {p.b for _, p in cases} >= {1, 2, 3, 4, 5} and {p.t for _, p in cases} >= {1, 2, 3, 17, 33, 129, 513}
    assert {(p.hq, p.hkv) for _, p in cases} == set(kc.HEADS) and {p.page for _, p in cases} == {16, 64, 256}
    assert max(p.b * p.t for _, p in cases) == 1030
    assert any(p.qkv_stride > p.rows * kc.D for _, p in cases)
    assert any(p.table_stride > -(-p.max_seq_len // p.page) for _, p in cases)
    assert any(int(s) + p.t == p.max_seq_len for _, p in cases for s in p.seq_lens)
    assert any(int(s) % p.page == p.page - 1 for _, p in cases for s in p.seq_lens)
    assert any(0 < int(s) % p.page < p.page - 1 for _, p in cases for s in p.seq_lens)
    assert {-1, -2 ** 31} <= {int(s) for _, p in cases for s in p.seq_lens}
    for name, p in cases:
        live = p.live()
        slots = [(pp, slot) for _, pp, slot in live]
        assert len(set(slots)) == len(slots), f"{name}: a slot written twice"
        assert all(0 <= pp < p.num_pages for pp, _ in slots)
        # the written slots are what the lengths say
        base = p.base()
        want = set()
        for b in range(p.b):
            for pos in range(base[b], min(base[b] + p.t, p.max_seq_len)):
                e = int(p.table[b, pos // p.page])
                if 0 <= e < p.num_pages:
                    want.add((e, pos % p.page))
        assert set(slots) == want, name
        r = kc.twin(p)
        assert _written(p, r) == {(kc.GUARD + pp, slot) for pp, slot in slots}, name
        assert r.lens_out.tolist() == [min(x + p.t, p.max_seq_len) for x in base], name
        dead = sorted(set(range(p.b * p.t)) - {n for n, _, _ in live})
        assert not r.q_out[dead].any() and bool(r.q_out[[n for n, _, _ in live]].all()), name
        # tokens on both sides of a page boundary
        positions = {(b, base[b] + t) for b in range(p.b) for t in range(p.t) if base[b] + t < p.max_seq_len}
        assert any(pos % p.page == p.page - 1 and (b, pos + 1) in positions for b, pos in positions) or \
            {pos % p.page for _, pos in positions} >= {0, p.page - 1}, name
        # every table entry the case can reach with a wrong slot or sequence still lies inside the guard pages
        assert int(p.table.min()) >= -kc.GUARD and int(p.table.max()) < p.num_pages + kc.GUARD
    past = dict(cases)["B 4, T 17, 21/3 heads, page 16, past max_seq_len"]
    assert kc.twin(past).lens_out.tolist() == [57, 64, 64, 64] and len(past.live()) == 17 + 0 + 14
    for name, p in kc.dropped_page_cases(kind):
        entries = {int(e) for e in p.table[:p.b].ravel()}
        assert {-3, -2, -1, p.num_pages, p.num_pages + 1, p.num_pages + 2} <= entries, name


@pytest.mark.parametrize("kind", kc.KINDS)
def test_a_wrong_twin_changes_a_case(kind):
    """An FMA in the rotation changes the cancellation case (about 940 of its 4096 rotated elements), whichever
    product it swallows; a dropped token, a token one slot late and a clamped page index each change an addressing or
    a dropped-page case."""
    c = kc.cancellation_problem(kind)
    right = kc.twin(c)
    for wrong in ("fuse x1c", "fuse x2s"):
        got = kc.twin(c, wrong)
        changed = int((got.q_out != right.q_out).sum())
        print(f"{kind}, {wrong}: {changed} of {right.q_out.size} elements of Q_out change")
        assert changed >= 1 and (kind == "fp8" or int((got.k != right.k).sum()) >= 1)
        assert np.array_equal(got.v, right.v) and np.array_equal(got.lens_out, right.lens_out)
    for name, p in kc.addressing_cases(kind):
        right = kc.twin(p)
        for wrong in ("drop a token", "a slot late"):
            got = kc.twin(p, wrong)
            assert not (np.array_equal(got.k, right.k) and np.array_equal(got.v, right.v)), (name, wrong)
    for name, p in kc.dropped_page_cases(kind):
        right, got = kc.twin(p), kc.twin(p, "clamp")
        assert not np.array_equal(got.k, right.k) and not np.array_equal(got.q_out, right.q_out), name


def test_sweeps_hold_every_bf16_code():
    assert sorted(kc.all_codes().ravel().tolist()) == list(range(65536))
    v = kc.sweep_problem("fp8", "v", 1.0)
    assert np.array_equal(np.sort(v.qkv.reshape(512, 3, kc.D)[:, 2].ravel()), np.arange(65536))
    seen = []
    for through in ("k0", "k1"):
        p = kc.sweep_problem("fp8", through, 0.5)
        k = p.qkv.reshape(512, 3, kc.D)[:, 1]
        assert not k[:256, kc.HALF:].any() and not k[256:, :kc.HALF].any()
        seen += [k[:256, :kc.HALF].ravel(), k[256:, kc.HALF:].ravel()]
        assert len(p.live()) == 512
    assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(65536))
    # through V with scale 1.0 every finite code up to 448 comes out as torch's cast has it
    r = kc.twin(v)
    codes = kc.all_codes()
    for n, pp, slot in v.live():
        x = kc.bf16_value(codes[n])
        ok = np.abs(x) <= 448
        assert np.array_equal(r.v[kc.GUARD + pp, 0, slot][ok], _torch_e4m3(x[ok]))


def test_chain_crosses_the_tile_and_ends_clamped():
    problems, lens = kc.chain_problem("bf16")
    assert len(problems) == 33 and problems[0].seq_lens.tolist() == [0, 20, 40] and lens == [33, 53, 70]
    assert all(p.t == 1 and p.page == 16 for p in problems)
    r = kc.chain_twin(problems)
    assert r.lens_out.tolist() == lens
    assert problems[0].max_seq_len == 70 and [len(p.live()) for p in problems[-4:]] == [3, 2, 2, 2]
    assert len(_written(problems[0], r)) == 33 + 33 + 30 and not r.q_out[2].any() and bool(r.q_out[:2].all())


# ---- what the entry points refuse --------------------------------------------------------------------------------------

# Addresses that are never dereferenced: every call below is refused before the first device call.
QKV, QO, K, V, BT, SL, LO, COS, SIN = (0x100000 * i for i in range(1, 10))


class _NoStream:
    """Stands in for ``hip.Stream``: the calls under test never get as far as using one."""
    handle = None


def _good(kind):
    inv = (1.0, 1.0) if kind == "bf16" else (2.0, 0.5)
    return {"qkv": QKV, "stride": 20 * 128 + 8, "qo": QO, "k": K, "v": V, "bt": BT + 4, "sl": SL + 4, "lo": LO + 4,
            "cos": COS, "sin": SIN, "rope_len": 320, "b": 3, "t": 5, "hq": 16, "hkv": 2, "d": 128, "page": 32,
            "num_pages": 40, "tstride": 10, "n": 320, "ki": inv[0], "vi": inv[1]}


def _call(hip, kind, v, timed=False):
    args = (_NoStream, kind, v["qkv"], v["stride"], v["qo"], v["k"], v["v"], v["bt"], v["sl"], v["lo"], v["cos"],
            v["sin"], v["rope_len"], v["b"], v["t"], v["hq"], v["hkv"], v["d"], v["page"], v["num_pages"], v["tstride"],
            v["n"])
    if timed:
        return hip.time_kv_append(*args, 1, v["ki"], v["vi"])
    return hip.kv_append(*args, v["ki"], v["vi"])


@pytest.mark.parametrize("timed", [False, True], ids=["launch", "timed"])
@pytest.mark.parametrize("kind", kc.KINDS)
def test_kv_append_rejects_bad_arguments_by_name(hip, kind, timed):
    def rej(text, **kw):
        with pytest.raises(hip.HipError, match=f"gsx_kv_append: {text}"):
            _call(hip, kind, {**_good(kind), **kw}, timed)

    for d in (0, 64, 127, 256):
        rej("need D == 128", d=d)
    rej("need 1 <= Hq", hq=0)
    for hq, hkv in ((16, 3), (16, 0), (34, 2), (17, 1), (8, 16)):
        rej("need Hq % Hkv == 0 and Hq / Hkv <= 16", hq=hq, hkv=hkv)
    for page in (0, 8, 24, 272, 512, -16):
        rej("need page % 16 == 0 and 16 <= page <= 256", page=page)
    rej("need B >= 1 and T >= 1", b=0)
    rej("need B >= 1 and T >= 1", t=0)
    rej("need B >= 1 and T >= 1", t=-1)
    rej("B \\* T must stay below 2\\^31", b=1 << 16, t=1 << 15)
    rej("need num_pages >= 1", num_pages=0)
    rej("need table_stride >= 1", tstride=0)
    rej("need max_seq_len >= 1", n=0)
    rej("need max_seq_len <= table_stride \\* page", n=321, rope_len=400)
    rej("need rope_len >= max_seq_len", rope_len=319)
    rej("need qkv_stride >= \\(Hq \\+ 2 Hkv\\) \\* D and qkv_stride % 8 == 0", stride=20 * 128 - 8)
    rej("need qkv_stride >= \\(Hq \\+ 2 Hkv\\) \\* D and qkv_stride % 8 == 0", stride=20 * 128 + 4)
    for name in ("qkv", "qo", "k", "v", "bt", "sl", "cos", "sin"):
        rej("QKV, Q_out, K_cache, V_cache, block_table, seq_lens, rope_cos and rope_sin must not be NULL", **{name: 0})
    for name in ("qkv", "qo", "k", "v", "cos", "sin"):
        rej("QKV, Q_out, K_cache, V_cache, rope_cos and rope_sin must be 16-B aligned", **{name: _good(kind)[name] + 8})
    for name in ("bt", "sl", "lo"):
        rej("block_table, seq_lens and lens_out must be 4-B aligned", **{name: BT + 2})
    qkv_bytes = (14 * (20 * 128 + 8) + 20 * 128) * 2
    for qo in (QKV, QKV + qkv_bytes - 16, QKV - 15 * 16 * 256 + 16):
        rej("Q_out must not overlap QKV", qo=qo)
    for lo in (SL + 4, SL + 12, SL - 4):
        rej("lens_out must not overlap seq_lens", lo=lo)
    if kind == "bf16":
        rej("a bf16 cache takes no scales: k_inv_scale and v_inv_scale must be 1.0", ki=0.5)
        rej("a bf16 cache takes no scales: k_inv_scale and v_inv_scale must be 1.0", vi=2.0)
    else:
        for name in ("ki", "vi"):
            for bad in (0.0, -1.0, float("inf"), float("nan")):
                rej("k_inv_scale and v_inv_scale must be finite and > 0", **{name: bad})


def test_kv_append_accepts_what_lies_next_to_a_refusal(hip):
    """The overlap rules refuse nothing that only touches: checked through the one refusal that comes after them."""
    g = _good("bf16")
    qkv_bytes = (14 * (20 * 128 + 8) + 20 * 128) * 2
    for kw in ({"qo": QKV + qkv_bytes}, {"qo": QKV - 15 * 16 * 256}, {"lo": SL + 4 + 12}, {"lo": SL + 4 - 12},
               {"lo": 0}):
        with pytest.raises(hip.HipError, match="a bf16 cache takes no scales"):
            _call(hip, "bf16", {**g, **kw, "ki": 0.5})


def test_kv_append_unknown_kind_is_rejected_by_name(hip):
    L = hip.lib()
    for kind in (-1, 2, 7):
        for fn, tail in ((L.gsx_kv_append, []), (L.gsx_event_time_kv_append, [1, None])):
            rc = fn(None, kind, QKV, 2560, QO, K, V, BT, SL, LO, COS, SIN, 320, 3, 5, 16, 2, 128, 32, 40, 10, 320, 1.0,
                    1.0, *tail)
            assert rc != 0 and L.gsx_last_error().decode() == f"gsx_kv_append: unknown kind {kind}"
    for timed in (False, True):
        with pytest.raises(ValueError, match="KV cache kind 'fp4'"):
            _call(hip, "fp4", _good("bf16"), timed)


# ---- the tools -------------------------------------------------------------------------------------------------------

def test_workload_and_isolation_parsers_take_the_server_workload():
    from gsxtools import isolation, workload

    for mod in (workload, isolation):
        ap = mod.build_parser()
        d = ap.parse_args(["--workload", "server"])
        assert (d.workload, d.batch, d.context, d.heads, d.kv_heads, d.kv_dtype, d.page) == \
            ("server", 8, 8192, 64, 8, "bf16", 16)
        assert ap.parse_args(["--workload", "server", "--batch", "16", "--kv-dtype", "fp8"]).kv_dtype == "fp8"
        for bad in (["--workload", "server", "--batch", "0"], ["--workload", "server", "--batch", "17"]):
            with pytest.raises(SystemExit):
                ap.parse_args(bad)
    a = isolation.build_parser().parse_args(["--workload", "server", "--kv-dtype", "fp8", "--kv-gib", "2",
                                             "--weights-gib", "1"])
    line = isolation.server_cmdline(a)
    got = workload.build_parser().parse_args(["--workload", "server", *line])
    assert (got.kv_dtype, got.kv_gib, got.weights_gib, got.heads) == ("fp8", 2.0, 1.0, 64)


def test_server_workload_sizes():
    from gsxtools import workload as wl

    # bf16 weights of one layer: the QKV projection [(Hq + 2 Hkv) 128][hidden] and the output projection [hidden]^2
    assert wl.server_layer_weight_bytes(64, 8) == ((64 + 16) * 128 * 8192 + 8192 * 8192) * 2
    assert [wl.server_window(n) for n in (1, 3, 64, 65, 8192)] == [1, 3, 64, 64, 64]
