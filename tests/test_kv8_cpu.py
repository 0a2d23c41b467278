"""The GPU-free part of the FP8 paged-KV cache: THE QUANTISATION RULE's CPU reference on literal vectors, the
"rope_append_kv8" / "attn_kv8" / "attn_split_kv8" op kinds and the LLM_KV8 table written out literally, the executor's
rows, and every error of the two wrappers' new arguments, which must fire before the native module is touched."""
import pytest
import torch

from k8s_gpu_scheduler_amd import _native
from k8s_gpu_scheduler_amd.models import workloads as W
from k8s_gpu_scheduler_amd.ops import loadgen
from k8s_gpu_scheduler_amd.parallel import executor

BF, FP8, U8 = torch.bfloat16, loadgen.FP8, torch.uint8
INF, NAN = float("inf"), float("nan")


# ------------------------------------------------------------------------------------------------
# the e4m3fn table, written from the format's definition (not from torch)
# ------------------------------------------------------------------------------------------------
def e4m3(code: int) -> float:
    e, m = (code >> 3) & 0xF, code & 7
    if code & 0x7F == 0x7F:
        return NAN
    v = m * 2.0 ** -9 if e == 0 else (8 + m) * 2.0 ** (e - 10)
    return -v if code & 0x80 else v


POS = [e4m3(c) for c in range(0x7F)]                                  # 0 .. 448, ascending


def q(values):
    return loadgen.quantize_kv8_reference(torch.tensor(values, dtype=torch.float32)).tolist()


def test_the_table_is_e4m3fn():
    assert POS[0] == 0.0 and POS[1] == 2.0 ** -9 and POS[8] == 2.0 ** -6 and POS[0x38] == 1.0 and POS[0x40] == 2.0
    assert POS[0x7E] == 448.0 and all(a < b for a, b in zip(POS, POS[1:]))
    t = torch.arange(256, dtype=U8).view(FP8).float()
    assert t[:0x7F].tolist() == POS and bool(t[0x7F].isnan()) and bool(t[0xFF].isnan())
    assert t[0x80:0xFF].tolist() == [-v for v in POS]


def test_every_value_round_trips():
    assert q(POS) == list(range(0x7F))
    assert q([-v for v in POS]) == [c | 0x80 for c in range(0x7F)]


def test_every_midpoint_goes_to_the_even_code():
    mids = [(a + b) / 2 for a, b in zip(POS, POS[1:])]
    assert all(torch.tensor(m, dtype=torch.float32).item() == m for m in mids)          # exact in fp32
    want = [c if c % 2 == 0 else c + 1 for c in range(0x7E)]
    assert q(mids) == want and q([-m for m in mids]) == [c | 0x80 for c in want]
    # one fp32 ulp to either side decides
    t = torch.tensor(mids, dtype=torch.float32)
    up, down = torch.nextafter(t, torch.tensor(INF)), torch.nextafter(t, torch.tensor(0.0))
    assert loadgen.quantize_kv8_reference(up).tolist() == list(range(1, 0x7F))
    assert loadgen.quantize_kv8_reference(down).tolist() == list(range(0x7E))


def test_saturation_nan_signed_zero_and_subnormals():
    assert q([464.0, 465.0, 480.0, 1e30, INF, -INF]) == [0x7E, 0x7E, 0x7E, 0x7E, 0x7E, 0xFE]
    assert q([-464.0, -465.0]) == [0xFE, 0xFE]
    nans = torch.tensor([0x7FC00000, 0xFFC00000 - (1 << 32), 0x7F800001, 0xFF812345 - (1 << 32)], dtype=torch.int32).view(torch.float32)
    assert loadgen.quantize_kv8_reference(nans).tolist() == [0x7F, 0xFF, 0x7F, 0xFF]
    assert q([0.0, -0.0, -2.0 ** -11, 2.0 ** -11, 2.0 ** -10, -2.0 ** -10, 1.5 * 2.0 ** -10]) == [0, 0x80, 0x80, 0, 0, 0x80, 1]
    assert q([3 * 2.0 ** -10, 2.5 * 2.0 ** -9, 7.5 * 2.0 ** -9, 7.75 * 2.0 ** -9]) == [2, 2, 8, 8]      # ties to even, the carry into the normals
    assert q([1e-45, -1e-45, 1e-38]) == [0, 0x80, 0]                                                     # fp32 subnormals
    with pytest.raises(ValueError):
        loadgen.quantize_kv8_reference(torch.zeros(3, dtype=BF))


def test_agrees_with_torch_up_to_448_and_not_beyond():
    g = torch.Generator().manual_seed(8)
    z = torch.cat([torch.randn(200000, generator=g) * s for s in (1e-3, 0.02, 1.0, 30.0, 200.0)]).clamp(-448, 448)
    bits = torch.randint(-2 ** 31, 2 ** 31, (400000,), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
    z = torch.cat([z, bits[bits.abs() <= 448]])
    assert torch.equal(loadgen.quantize_kv8_reference(z), z.to(FP8).view(U8))
    assert torch.tensor([500.0]).to(FP8).view(U8).item() == 0x7F and q([500.0]) == [0x7E]        # torch does not saturate


def test_dequantize_reference():
    codes = torch.arange(256, dtype=U8)
    d = loadgen.dequantize_kv8_reference(codes, 1.0)
    assert d.dtype == torch.float64 and d[:0x7F].tolist() == POS and bool(d[0x7F].isnan()) and bool(d[0xFF].isnan())
    assert torch.equal(loadgen.dequantize_kv8_reference(codes.view(FP8), 0.75).nan_to_num(9.0), (d * 0.75).nan_to_num(9.0))
    cache = torch.full((2, 2, 32, 128), 0x38, dtype=U8)                                          # 1.0
    per_head = loadgen.dequantize_kv8_reference(cache, torch.tensor([0.5, 4.0]).view(1, 2, 1, 1))
    assert bool((per_head[:, 0] == 0.5).all()) and bool((per_head[:, 1] == 4.0).all())
    # every finite code is exact in bf16: the kernels convert without loss
    assert torch.equal(d[~d.isnan()].to(BF).double(), d[~d.isnan()])
    with pytest.raises(ValueError):
        loadgen.dequantize_kv8_reference(torch.zeros(3, dtype=torch.int32), 1.0)


def test_rope_append_reference_composes_rotation_and_division():
    g = torch.Generator().manual_seed(9)
    Hq, Hkv = 4, 2
    qkv = (torch.randint(-127, 128, (7, Hq + 2 * Hkv, 128), generator=g).float() / 64).to(BF)
    cs = torch.randint(-8, 9, (40, 128), generator=g).float() / 8
    ctx, q_start = torch.tensor([35, 3], dtype=torch.int32), torch.tensor([1, 4, 6], dtype=torch.int32)
    ks, vs = torch.tensor([0.125, 4.0]), torch.tensor([1.0, 0.75])
    kb, vb = loadgen.rope_append_kv8_reference(qkv, cs, ctx, q_start, ks, vs)
    assert kb.dtype == U8 and tuple(kb.shape) == tuple(vb.shape) == (7, Hkv, 128)
    assert not kb[0].any() and not kb[6].any() and not vb[0].any()                # rows of no chunk
    row, pos = 2, 33                                                             # second row of sequence 0: 35 - 3 + 1
    x = qkv[row, Hq + 1].double()
    c, s = cs[pos, :64].double(), cs[pos, 64:].double()
    y = torch.cat([x[:64] * c - x[64:] * s, x[64:] * c + x[:64] * s])
    assert torch.equal(kb[row, 1], loadgen.quantize_kv8_reference((y / 4.0).float()))
    assert torch.equal(vb[row, 1], loadgen.quantize_kv8_reference(qkv[row, Hq + Hkv + 1].float() / 0.75))
    assert torch.equal(vb[5, 0], loadgen.quantize_kv8_reference(qkv[5, Hq + Hkv].float()))


# ------------------------------------------------------------------------------------------------
# Op accounting and the table
# ------------------------------------------------------------------------------------------------
def test_op_accounting_written_out():
    a = W.Op("attn_kv8", 256, 32, 1024, rows=8)
    assert a.flops == 4.0 * 256 * 32 * 1024 * 128 == W.Op("attn", 256, 32, 1024, rows=8).flops
    assert a.bytes == 2 * 256 * 8 * 1024 * 128 + 4 * 256 * 32 * 128 + 4 * 256 * 32 + 4 * 256 + 8 * 8
    assert a.workgroups(0) == a.workgroups(64) == 2048 and not a.on_mfma and not a.is_gemm and a.mfma_rate() == 1.0
    sp = W.Op("attn_split_kv8", 8, 32, 32768, rows=8, splits=4)
    assert sp.flops == 4.0 * 8 * 32 * 32768 * 128
    assert sp.bytes == 2 * 8 * 8 * 32768 * 128 + 4 * 8 * 32 * 128 + 4 * 8 * 1024 + 4 * 8 + 8 * 8 + 2 * 4 * 8 * 32 * 4 * 132
    assert sp.workgroups(0) == 256 and not sp.on_mfma
    r = W.Op("rope_append_kv8", 256, 32, 1024, rows=8, q=1)
    assert r.flops == 3.0 * 128 * 40 * 256 == W.Op("rope_append", 256, 32, 1024, rows=8, q=1).flops
    assert r.bytes == (2 * 256 * 48 * 128 + 2 * 256 * 32 * 128 + 256 * 16 * 128 + 512 * 256 + 4 * 256 + 4 * 257 + 4 * 256 + 8 * 8)
    assert r.workgroups(0) == 2048
    r8 = W.Op("rope_append_kv8", 8, 32, 32768, rows=8, q=1)
    assert r8.bytes == 2 * 8 * 48 * 128 + 2 * 8 * 32 * 128 + 8 * 16 * 128 + 512 * 8 + 4 * 8 + 4 * 9 + 4 * 8 + 8 * 8
    assert r8.workgroups(0) == 64
    # half the cache bytes of the bf16 kinds, and they are unchanged
    b16 = W.Op("attn", 256, 32, 1024, rows=8)
    assert b16.bytes == 4 * 256 * 8 * 1024 * 128 + 4 * 256 * 32 * 128 + 4 * 256 * 32 + 4 * 256
    assert b16.bytes - a.bytes == 2 * 256 * 8 * 1024 * 128 - 64
    assert W.Op("rope_append", 256, 32, 1024, rows=8, q=1).bytes == r.bytes + 256 * 16 * 128 - 64


def test_llm_kv8_table_written_out():
    dec = W.Workload("llm_kv8_layer_decode_256", "llm_kv8_layer_decode", "hip", 256,
                     (W.Op("gemm", 256, 6144, 4096), W.Op("rope_append_kv8", 256, 32, 1024, rows=8, q=1),
                      W.Op("attn_kv8", 256, 32, 1024, rows=8), W.Op("gemm", 256, 4096, 4096)), 1.25)
    lng = W.Workload("llm_kv8_decode_long_8", "llm_kv8_decode_long", "hip", 8,
                     (W.Op("gemm", 64, 6144, 4096), W.Op("rope_append_kv8", 8, 32, 32768, rows=8, q=1),
                      W.Op("attn_split_kv8", 8, 32, 32768, rows=8, splits=4), W.Op("gemm", 64, 4096, 4096)), 1.25)
    assert W.LLM_KV8 == {"llm_kv8_layer_decode_256": dec, "llm_kv8_decode_long_8": lng}
    # llm_layer_decode_256 with the two kv8 kinds
    want = tuple(W.Op(o.kind + "_kv8", o.M, o.N, o.K, rows=o.rows, q=o.q) if o.kind in ("rope_append", "attn") else o
                 for o in W.LLM_LAYER["llm_layer_decode_256"].ops)
    assert dec.ops == want
    assert not set(W.LLM_KV8) & (set(W.CATALOG) | set(W.EXTRA))
    for w in W.LLM_KV8.values():
        assert W.get(w.name) is w
        assert W.workload_for_pod(f"pod-{w.name.replace('_', '-')}-17") is w
        assert W.roofline_seconds(w, 1.0) > 0 and 0 < W.cu_fill(w) <= 1
        assert W.roofline_split(w.name)[1] > 0


def _declared_bytes(w: W.Workload) -> float:
    """What executor._Buffers allocates for the workload, from the operand layouts of its OP_KINDS rows."""
    total = 0.0
    for o in w.ops:
        if o.kind == "gemm":
            total += 2 * (o.M * o.K + o.N * o.K + o.M * o.N) + 4 * o.N
        elif o.kind in ("attn_kv8", "attn_split_kv8", "rope_append_kv8"):
            rows = o.M * (o.q or 1)
            total += 2 * o.M * o.K * o.rows * 128 + 2 * 2 * rows * o.N * 128 + 8 * o.rows        # 1-byte caches, q / out, scales
            total += 4 * o.M * o.K // 32 + 4 * o.M                                              # table, ctx
            if o.kind == "rope_append_kv8":
                total += 2 * rows * 2 * o.rows * 128 + 4 * 128 * o.K + 4 * (o.M + 1)             # the K / V part of qkv, cos_sin
            if o.kind == "attn_split_kv8":
                total += 4 * W.decode_split_workspace_floats(o.M, o.N, o.splits)
        else:
            raise AssertionError(o)
    return total


def test_llm_kv8_declared_footprints_cover_the_operands():
    for w in W.LLM_KV8.values():
        caches = sum(2 * o.M * o.K * o.rows * 128 for o in w.ops if o.kind.endswith("_kv8"))
        assert caches == 2 * 512 * 2 ** 20                                                       # two 512 MiB caches (K + V) each
        gib = _declared_bytes(w) / 2 ** 30
        assert gib <= w.hbm_gib < gib + 0.25, (w.name, gib)


def test_new_names_change_no_existing_lookup():
    tables = (W.CATALOG, W.EXTRA, W.STAGED, W.LONG_CONTEXT, W.LLM_LAYER, W.LLM_BLOCK, W.LLM_HEAD, W.LLM_MOE, W.LLM_MX)
    old = [n for t in tables for n in t]
    for new in W.LLM_KV8:
        assert not any(o in new for o in old), new                      # an older name would win the lookup of a new pod
        assert not any(new in o for o in old), new
    assert not any(a != b and a in b for a in W.LLM_KV8 for b in W.LLM_KV8)
    for t in tables:
        for n, w in t.items():
            assert W.workload_for_pod(f"x-{n.replace('_', '-')}-0").name in (n, W.workload_for_pod(n).name)
            assert W.get(n) is w


# ------------------------------------------------------------------------------------------------
# the executor's rows
# ------------------------------------------------------------------------------------------------
def test_op_kinds_rows_build_operands_on_the_cpu():
    assert all(executor.OP_KINDS[k][2] == 0 for k in ("attn_kv8", "attn_split_kv8", "rope_append_kv8"))
    assert {o.kind for w in W.LLM_KV8.values() for o in w.ops} <= set(executor.OP_KINDS)
    ops = (W.Op("rope_append_kv8", 3, 4, 64, rows=2, q=5), W.Op("attn_kv8", 3, 4, 64, rows=2),
           W.Op("attn_split_kv8", 2, 8, 3 * 32 * 40, rows=2, splits=3))
    w = W.Workload("kv8_rows", "pin", "hip", 3, ops, 0.1)
    bufs, again = executor._Buffers(w, torch.device("cpu")), executor._Buffers(w, torch.device("cpu"))
    (o0, t0), (o1, t1), (o2, t2) = bufs.ops
    q_out, qkv, cos_sin, kc, vc, table, ctx, q_start, ks, vs = t0
    assert executor.op_output(o0, t0) is q_out and tuple(q_out.shape) == (15, 4, 128) and tuple(qkv.shape) == (15, 8, 128)
    assert kc.dtype == vc.dtype == FP8 and tuple(kc.shape) == (6, 2, 32, 128) and tuple(vc.shape) == (6, 2, 128, 32)
    assert not kc.view(U8).any() and not vc.view(U8).any()                                      # the append's caches start as zeros
    assert tuple(cos_sin.shape) == (64, 128) and q_start.tolist() == [0, 5, 10, 15] and ctx.tolist() == [64] * 3
    assert sorted(table.flatten().tolist()) == list(range(6))
    for t, n_ops in ((t0, 10), (t1, 8), (t2, 9)):
        assert len(t) == n_ops
        k_scale, v_scale = t[-2:]
        assert k_scale.dtype == v_scale.dtype == torch.float32 and tuple(k_scale.shape) == tuple(v_scale.shape) == (2,)
        assert k_scale.tolist() == [executor.KV8_K_SCALE] * 2 and v_scale.tolist() == [executor.KV8_V_SCALE] * 2
        assert k_scale.is_contiguous() and executor.KV8_K_SCALE > 0 and executor.KV8_V_SCALE > 0
    for (o, t), (_, u) in zip(bufs.ops[1:], again.ops[1:]):
        out, qq, kc, vc, table, ctx = t[:6]
        nb = o.M * o.K // 32
        assert executor.op_output(o, t) is out and out.dtype == BF and tuple(out.shape) == tuple(qq.shape) == (o.M, o.N, 128)
        assert kc.dtype == vc.dtype == FP8 and tuple(kc.shape) == (nb, 2, 32, 128) and tuple(vc.shape) == (nb, 2, 128, 32)
        for c in (kc, vc):
            d = loadgen.dequantize_kv8_reference(c, 1.0)
            assert bool(d.isfinite().all()) and float(d.abs().max()) == 2.0 and float(d.min()) == -2.0
            assert len(c.view(U8).unique()) > 100
        assert sorted(table.flatten().tolist()) == list(range(nb)) and ctx.tolist() == [o.K] * o.M
        assert all(torch.equal(a.view(U8) if a.dtype == FP8 else a, b.view(U8) if b.dtype == FP8 else b)
                   for a, b in zip(t[1:6], u[1:6]))                                            # seeded
    ws = t2[6]
    assert ws.dtype == torch.float32 and ws.numel() == W.decode_split_workspace_floats(2, 8, 3)
    big = t2[2].view(U8)                                                                         # 240 blocks repeat a pattern of 64
    assert torch.equal(big[64:128], big[:64]) and torch.equal(big[192:240], big[:48])

    calls = []
    saved = loadgen.rope_append, loadgen.paged_decode_attention_kv8, loadgen.paged_decode_attention

    def no_bf16_call(*a, **kw):
        raise AssertionError("a kv8 kind called the bf16 wrapper")
    loadgen.rope_append = lambda *a, **kw: calls.append(("append", len(a), a[2].dtype, kw["max_q_len"], kw["check"], sorted(kw)))
    loadgen.paged_decode_attention_kv8 = lambda *a, **kw: calls.append(("attn", len(a), a[1].dtype, a[5].dtype, a[6].dtype, kw.get("kv_splits", 1), kw["check"], sorted(kw)))
    loadgen.paged_decode_attention = no_bf16_call
    try:
        executor.enqueue_ops(bufs, 1, "st", 64)
    finally:
        loadgen.rope_append, loadgen.paged_decode_attention_kv8, loadgen.paged_decode_attention = saved
    F32 = torch.float32
    assert calls == [("append", 7, FP8, 5, False, ["check", "k_scale", "max_q_len", "q_out", "stream", "v_scale"]),
                     ("attn", 7, FP8, F32, F32, 1, False, ["check", "out", "stream"]),
                     ("attn", 7, FP8, F32, F32, 3, False, ["check", "kv_splits", "out", "stream", "workspace"])]


def test_bf16_rows_make_the_calls_they_made():
    """The bf16 kinds' recorded loadgen calls carry no scale keyword."""
    ops = (W.Op("rope_append", 3, 4, 64, rows=2, q=5), W.Op("attn", 3, 4, 64, rows=2), W.Op("attn_split", 2, 8, 96, rows=2, splits=3))
    bufs = executor._Buffers(W.Workload("bf16_rows", "pin", "hip", 3, ops, 0.1), torch.device("cpu"))
    assert [len(t) for _, t in bufs.ops] == [8, 6, 7] and bufs.ops[0][1][3].dtype == BF
    calls = []
    saved = loadgen.rope_append, loadgen.paged_decode_attention
    loadgen.rope_append = lambda *a, **kw: calls.append(sorted(kw))
    loadgen.paged_decode_attention = lambda *a, **kw: calls.append(sorted(kw))
    try:
        executor.enqueue_ops(bufs, 1, "st", 64)
    finally:
        loadgen.rope_append, loadgen.paged_decode_attention = saved
    assert calls == [["check", "max_q_len", "q_out", "stream"], ["check", "out", "stream"],
                     ["check", "kv_splits", "out", "stream", "workspace"]]


# ------------------------------------------------------------------------------------------------
# host wrappers: every rejection happens before the native module is asked for
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def host_operands_pass(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the native module was touched")
    monkeypatch.setattr(_native, "hip", boom)
    monkeypatch.setattr(loadgen, "_check_devices", lambda name, *ts: torch.device("cpu"))


def _decode(S=2, Hq=4, Hkv=2, NB=3, MB=2, dtype=FP8):
    q_ = torch.zeros(S, Hq, 128, dtype=BF)
    kc = torch.zeros(NB, Hkv, 32, 128, dtype=U8).view(dtype) if dtype == FP8 else torch.zeros(NB, Hkv, 32, 128, dtype=dtype)
    vc = torch.zeros(NB, Hkv, 128, 32, dtype=U8).view(dtype) if dtype == FP8 else torch.zeros(NB, Hkv, 128, 32, dtype=dtype)
    return q_, kc, vc, torch.zeros(S, MB, dtype=torch.int32), torch.ones(S, dtype=torch.int32)


def _append(Hq=4, Hkv=2, dtype=FP8):
    q_, kc, vc, table, ctx = _decode(Hq=Hq, Hkv=Hkv, dtype=dtype)
    qkv = torch.zeros(2, Hq + 2 * Hkv, 128, dtype=BF)
    return qkv, torch.zeros(64, 128), kc, vc, table, ctx, torch.tensor([0, 1, 2], dtype=torch.int32)


SCALES = lambda n=2: (torch.ones(n), torch.ones(n))              # noqa: E731


def _both(call_decode, call_append):
    return ((loadgen.paged_decode_attention_kv8, call_decode), (loadgen.rope_append, call_append))


def test_wrappers_reject_scales_with_bf16_caches(host_operands_pass):
    ks, vs = SCALES()
    for fn, args in _both(_decode(dtype=BF), _append(dtype=BF)):
        for kw in (dict(k_scale=ks, v_scale=vs), dict(k_scale=ks), dict(v_scale=vs)):
            with pytest.raises(ValueError, match="scale"):
                fn(*args, **kw)


def test_wrappers_need_both_scales_with_fp8_caches(host_operands_pass):
    ks, vs = SCALES()
    for fn, args in _both(_decode(), _append()):
        for kw in ({}, dict(k_scale=ks), dict(v_scale=vs)):
            with pytest.raises(ValueError, match="need k_scale and v_scale"):
                fn(*args, **kw)


def test_wrappers_reject_bad_scale_tensors(host_operands_pass):
    ks, vs = SCALES()
    for fn, args in _both(_decode(), _append()):
        with pytest.raises(TypeError, match="fp32 k_scale"):
            fn(*args, k_scale=ks.double(), v_scale=vs)
        with pytest.raises(TypeError, match="fp32 v_scale"):
            fn(*args, k_scale=ks, v_scale=vs.to(BF))
        for bad in (torch.ones(3), torch.ones(1), torch.ones(2, 1), torch.ones(4)[::2], torch.tensor(1.0)):
            with pytest.raises(ValueError, match=r"contiguous \[2\] vector"):
                fn(*args, k_scale=bad, v_scale=vs)
            with pytest.raises(ValueError, match=r"contiguous \[2\] vector"):
                fn(*args, k_scale=ks, v_scale=bad)


def test_wrappers_reject_mixed_and_other_cache_dtypes(host_operands_pass):
    ks, vs = SCALES()
    q_, kc8, vc8, table, ctx = _decode()
    _, kc16, vc16, _, _ = _decode(dtype=BF)
    for kc, vc in ((kc8, vc16), (kc16, vc8)):
        with pytest.raises(TypeError, match="one cache dtype"):
            loadgen.paged_decode_attention_kv8(q_, kc, vc, table, ctx, k_scale=ks, v_scale=vs)
        a = _append()
        with pytest.raises(TypeError, match="one cache dtype"):
            loadgen.rope_append(a[0], a[1], kc, vc, *a[4:], k_scale=ks, v_scale=vs)
    for other in (torch.float16, torch.float32, U8, torch.float8_e5m2):
        _, kc, vc, _, _ = _decode(dtype=other)
        for pair in ((kc, vc), (kc, vc16), (kc8, vc)):
            with pytest.raises(TypeError, match="bf16"):
                loadgen.paged_decode_attention(q_, *pair, table, ctx)
            a = _append()
            with pytest.raises(TypeError, match="bf16"):
                loadgen.rope_append(a[0], a[1], *pair, *a[4:])
    with pytest.raises(TypeError, match="bf16"):                                     # q stays bf16
        loadgen.paged_decode_attention_kv8(q_.float(), kc8, vc8, table, ctx, k_scale=ks, v_scale=vs)


def test_each_decode_wrapper_reads_one_cache_dtype(host_operands_pass):
    """paged_decode_attention keeps its parameter list and reads bf16 caches only; paged_decode_attention_kv8 reads
    FP8 caches only."""
    import inspect
    ks, vs = SCALES()
    names = list(inspect.signature(loadgen.paged_decode_attention_kv8).parameters)
    assert names == ["q", "k_cache", "v_cache", "block_table", "ctx_lens", "k_scale", "v_scale", "out", "scale", "stream",
                     "check", "kv_splits", "workspace"]
    assert "k_scale" not in inspect.signature(loadgen.paged_decode_attention).parameters
    with pytest.raises(TypeError, match="bf16"):
        loadgen.paged_decode_attention(*_decode())
    with pytest.raises(TypeError):
        loadgen.paged_decode_attention(*_decode(), k_scale=ks, v_scale=vs)
    with pytest.raises(ValueError, match="these are bf16"):
        loadgen.paged_decode_attention_kv8(*_decode(dtype=BF))
    with pytest.raises(ValueError, match="these are bf16"):
        loadgen.paged_decode_attention_kv8(*_decode(dtype=BF), ks, vs)
    assert tuple(loadgen.paged_decode_attention_kv8(*_decode(S=0), ks, vs).shape) == (0, 4, 128)       # positional scales


def test_prefill_keeps_rejecting_fp8_caches(host_operands_pass):
    q_, kc, vc, table, ctx = _decode()
    with pytest.raises(TypeError, match="bf16"):
        loadgen.paged_prefill_attention(q_, kc, vc, table, ctx, torch.tensor([0, 1, 2], dtype=torch.int32), max_q_len=1)
    assert "k_scale" not in loadgen.paged_prefill_attention.__code__.co_varnames


def test_the_other_checks_hold_for_fp8_caches(host_operands_pass):
    """The layout, group and workspace rules are checked on FP8 caches as on bf16 ones."""
    ks, vs = SCALES()
    q_, kc, vc, table, ctx = _decode()
    with pytest.raises(ValueError, match="contiguous caches"):
        loadgen.paged_decode_attention_kv8(q_, torch.zeros(6, 2, 32, 128, dtype=U8).view(FP8)[::2], vc, table, ctx, k_scale=ks, v_scale=vs)
    off = torch.zeros(3 * 2 * 32 * 128 + 16, dtype=U8)[8:-8].view(FP8)
    with pytest.raises(ValueError, match="16-byte"):
        loadgen.paged_decode_attention_kv8(q_, off.view(3, 2, 32, 128), vc, table, ctx, k_scale=ks, v_scale=vs)
    with pytest.raises(ValueError, match="Hq / Hkv"):
        loadgen.paged_decode_attention_kv8(*_decode(Hq=6, Hkv=2), k_scale=ks, v_scale=vs)
    with pytest.raises(ValueError, match="kv_splits"):
        loadgen.paged_decode_attention_kv8(q_, kc, vc, table, ctx, k_scale=ks, v_scale=vs, kv_splits=33)
    with pytest.raises(ValueError, match="workspace of"):
        loadgen.paged_decode_attention_kv8(q_, kc, vc, table, ctx, k_scale=ks, v_scale=vs, kv_splits=2, workspace=torch.zeros(8))
    a = _append()
    with pytest.raises(ValueError, match="check=False needs max_q_len"):
        loadgen.rope_append(*a, k_scale=ks, v_scale=vs, check=False)
    with pytest.raises(ValueError, match="overlaps"):
        loadgen.rope_append(*a, k_scale=ks, v_scale=vs, q_out=a[0][:, :4])


def test_empty_launches_return_without_the_native_module(host_operands_pass):
    ks, vs = SCALES()
    out = loadgen.paged_decode_attention_kv8(*_decode(S=0), k_scale=ks, v_scale=vs)
    assert tuple(out.shape) == (0, 4, 128)
    a = _append()
    assert tuple(loadgen.rope_append(*a, max_q_len=0, k_scale=ks, v_scale=vs).shape) == (2, 4, 128)


@pytest.mark.skipif(_native.hip(required=False) is None, reason="HIP extension not built")
def test_native_entry_points_throw_on_bad_operands():
    h = _native.hip()
    for fn in ("rope_append_kv8", "paged_decode_kv8", "paged_decode_split_kv8"):
        assert hasattr(h, fn)
    A = 4096                                                                         # an aligned non-null address: nothing launches
    with pytest.raises(RuntimeError, match="k_scale and v_scale are needed"):
        h.paged_decode_kv8(A, A, A, 0, A, A, A, A, 1, 4, 2, 512, 512, 1, 1.0, 0)
    with pytest.raises(RuntimeError, match="4-byte aligned"):
        h.paged_decode_kv8(A, A, A, A + 2, A, A, A, A, 1, 4, 2, 512, 512, 1, 1.0, 0)
    with pytest.raises(RuntimeError, match="Hq / Hkv"):
        h.paged_decode_kv8(A, A, A, A, A, A, A, A, 1, 6, 2, 768, 768, 1, 1.0, 0)
    with pytest.raises(RuntimeError, match="kv_splits"):
        h.paged_decode_split_kv8(A, A, A, A, A, A, A, A, A, 1, 4, 2, 33, 512, 512, 1, 1.0, 0)
    with pytest.raises(RuntimeError, match="k_scale and v_scale are needed"):
        h.paged_decode_split_kv8(A, A, A, A, 0, A, A, A, A, 1, 4, 2, 2, 512, 512, 1, 1.0, 0)
    with pytest.raises(RuntimeError, match="4-byte aligned"):
        h.rope_append_kv8(A, A, A, A, A, A + 1, A, A, A, A, 1, 4, 2, 1, 8, 1024, 512, 1, 0)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        h.rope_append_kv8(A, A, A + 8, A, A, A, A, A, A, A, 1, 4, 2, 1, 8, 1024, 512, 1, 0)
    # S == 0 launches nothing and needs no GPU
    h.paged_decode_kv8(A, A, A, A, A, A, A, A, 0, 4, 2, 512, 512, 1, 1.0, 0)
    h.paged_decode_split_kv8(A, A, A, A, A, A, A, 0, A, 0, 4, 2, 2, 512, 512, 1, 1.0, 0)
    h.rope_append_kv8(A, A, A, A, A, A, A, A, A, A, 0, 4, 2, 1, 8, 1024, 512, 1, 0)
