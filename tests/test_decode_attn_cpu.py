"""The paged-KV decode attention without a GPU: the workload model's attn op and the llm_decode_256
workload, the pure-Python grid rule, the host wrapper's validation (which must fire before the
native module is touched), the profiler's kernel classification, the executor's op dispatch and the
float64 reference of the GPU tests.  The kernel itself is pinned on the GPU by
test_gpu_decode_attn_exact.py."""
import math

import pytest
import torch

from k8s_gpu_scheduler_amd import _native
from k8s_gpu_scheduler_amd.models import workloads as W
from k8s_gpu_scheduler_amd.ops import loadgen


# ------------------------------------------------------------------------------------------------
# workload model
# ------------------------------------------------------------------------------------------------
def test_attn_op_bytes_flops():
    o = W.Op("attn", M=3, N=8, K=64, rows=2)
    assert W.ATTN_HEAD_DIM == 128 and W.ATTN_BLOCK_TOKENS == 32
    assert not o.is_gemm
    assert o.flops == 4 * 3 * 8 * 64 * 128
    assert o.bytes == 4 * 3 * 2 * 64 * 128 + 4 * 3 * 8 * 128 + 4 * 3 * 64 / 32 + 4 * 3
    assert o.mfma_rate() == 1.0


def _old_flops(o):
    if o.kind == "gather":
        return 1.0 * o.M * o.K * o.N
    return 2.0 * o.M * o.N * o.K if o.kind in ("gemm", "gemm8") else 2.0 * o.n_floats


def _old_bytes(o):
    if o.kind == "gemm":
        return 2.0 * (o.M * o.K + o.N * o.K + o.M * o.N)
    if o.kind == "gemm8":
        return 1.0 * (o.M * o.K + o.N * o.K) + 2.0 * o.M * o.N
    if o.kind == "gather":
        return 2.0 * o.M * o.K * o.N + 4.0 * o.M * o.K + 4.0 * (o.M + 1) + 2.0 * o.M * o.N
    return 12.0 * o.n_floats


def _old_roofline(w, share, peak_tflops=1100.0, hbm_tbps=5.5, share_bw_exp=0.6):
    t = 0.0
    for o in w.ops:
        if o.kind in ("gemm", "gemm8"):
            rate = 2.0 if o.kind == "gemm8" else 1.0
            t += max(_old_flops(o) / (peak_tflops * rate * 1e12 * share),
                     _old_bytes(o) / (hbm_tbps * 1e12 * share ** share_bw_exp))
        else:
            t += _old_bytes(o) / (hbm_tbps * 1e12 * share ** share_bw_exp)
    return t


def _old_cu_fill(w, cu_budget=W.POD_CU_BUDGET):
    t = f = 0.0
    for o in w.ops:
        dt = _old_roofline(W.Workload(w.name, w.family, w.framework, w.batch, (o,), 0.0), 1.0)
        if o.kind in ("gemm", "gemm8"):
            fo = min(1.0, W.default_gemm_workgroups(o.M, o.N, o.K, cu_budget, o.kind == "gemm8") / W.CUS)
        elif o.kind == "gather":
            fo = min(1.0, W.default_gather_workgroups(o.M) / W.CUS)
        else:
            fo = 1.0
        t += dt
        f += dt * fo
    return f / t


def test_existing_workloads_keep_their_values_bit_for_bit():
    """Expected values from the formulas as they stood before the attn op (copied above)."""
    assert len(W.CATALOG) == 18 and set(W.EXTRA) == {"fp8_llm_2048", "triad_only_2048", "dlrm_2048", "llm_decode_256"}
    for w in list(W.CATALOG.values()) + [W.EXTRA[n] for n in ("fp8_llm_2048", "triad_only_2048", "dlrm_2048")]:
        assert all(o.kind in ("gemm", "gemm8", "triad", "gather") for o in w.ops)
        assert w.flops == sum(_old_flops(o) for o in w.ops)
        assert w.bytes == sum(_old_bytes(o) for o in w.ops)
        for share in (1.0, 0.5, 0.25, 0.125):
            assert W.roofline_seconds(w, share) == _old_roofline(w, share)
        for budget in (W.POD_CU_BUDGET, 0, 128):
            assert W.cu_fill(w, budget) == _old_cu_fill(w, budget)


def test_llm_decode_workload():
    w = W.get("llm_decode_256")
    assert W.workload_for_pod("llm-decode-256-x") is w
    assert (w.family, w.framework, w.batch, w.hbm_gib) == ("llm_decode", "hip", 256, 1.25)
    qkv, a, proj = w.ops
    assert a.kind == "attn" and (a.M, a.N, a.K, a.rows) == (256, 32, 1024, 8)
    cache_bytes = 2 * a.M * a.K * a.rows * W.ATTN_HEAD_DIM * 2                       # K and V, bf16
    assert cache_bytes == 1 << 30 and w.hbm_gib * (1 << 30) >= cache_bytes
    assert a.K % W.ATTN_BLOCK_TOKENS == 0 and a.N % a.rows == 0 and a.N // a.rows in loadgen.ATTN_GROUPS
    assert [(o.kind, o.M, o.N, o.K) for o in (qkv, proj)] == [("gemm", 256, 6144, 4096), ("gemm", 256, 4096, 4096)]
    assert all(d % 64 == 0 for o in (qkv, proj) for d in (o.M, o.N, o.K))
    assert qkv.N == (a.N + 2 * a.rows) * W.ATTN_HEAD_DIM and proj.K == a.N * W.ATTN_HEAD_DIM
    t = W.roofline_seconds(w, 1.0)
    assert math.isfinite(t) and t > 0
    assert t == pytest.approx(a.bytes / 5.5e12 + sum(max(o.flops / 1100e12, o.bytes / 5.5e12) for o in (qkv, proj)))
    m, h = W.roofline_split("llm-decode-256-x", tflops=1.0e3, tbps=6.0)
    assert h == pytest.approx(a.bytes / 6.0e12) and m == pytest.approx((qkv.flops + proj.flops) / 1.0e15)
    assert h > m                                                                     # the attention dominates
    assert 0.0 < W.cu_fill(w) <= 1.0


def test_attn_cu_fill_counts_workgroups():
    one = W.Workload("a", "llm_decode", "hip", 1, (W.Op("attn", 16, 32, 1024, rows=8),), 0.0)
    assert W.cu_fill(one) == pytest.approx(128 / W.CUS)             # 16 sequences x 8 KV heads
    assert W.cu_fill(W.Workload("a", "llm_decode", "hip", 1, (W.Op("attn", 256, 32, 1024, rows=8),), 0.0)) == 1.0


def test_default_attn_workgroups():
    assert [W.default_attn_workgroups(s, g) for s, g in ((1, 1), (8, 2), (256, 8), (0, 8))] == [1, 16, 2048, 0]


@pytest.mark.skipif(_native.hip(required=False) is None, reason="HIP extension not built")
def test_default_attn_workgroups_match_the_native_rule():
    h = _native.hip()
    for s in (0, 1, 7, 256, 2048, 65536):
        for g in (1, 2, 8, 16):
            assert h.paged_decode_workgroups(s, g) == W.default_attn_workgroups(s, g), (s, g)


# ------------------------------------------------------------------------------------------------
# host wrapper: every rejection happens before the native module is asked for
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def no_native(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the native module was touched")
    monkeypatch.setattr(_native, "hip", boom)


def _operands(S=2, Hq=4, Hkv=2, NB=3, MB=2, D=128, T=32):
    q = torch.zeros(S, Hq, D, dtype=torch.bfloat16)
    kc = torch.zeros(NB, Hkv, T, D, dtype=torch.bfloat16)
    vc = torch.zeros(NB, Hkv, D, T, dtype=torch.bfloat16)
    table = torch.zeros(S, MB, dtype=torch.int32)
    ctx = torch.ones(S, dtype=torch.int32)
    return q, kc, vc, table, ctx


def test_wrapper_rejects_cpu_tensors(no_native):
    q, kc, vc, table, ctx = _operands()
    with pytest.raises(ValueError, match="device tensors"):
        loadgen.paged_decode_attention(q, kc, vc, table, ctx)
    with pytest.raises(ValueError, match="device tensors"):          # before any dtype complaint
        loadgen.paged_decode_attention(q.float(), kc, vc, table.long(), ctx)


@pytest.fixture
def host_operands_pass(monkeypatch, no_native):
    """The remaining checks need tensors that pass the device check; without a GPU the check is
    stubbed out, and everything after it up to the native call runs on host tensors."""
    monkeypatch.setattr(loadgen, "_check_devices", lambda name, *ts: torch.device("cpu"))


def test_wrapper_rejects_dtypes(host_operands_pass):
    q, kc, vc, table, ctx = _operands()
    for bad in ((q.float(), kc, vc), (q, kc.half(), vc), (q, kc, vc.float())):
        with pytest.raises(TypeError, match="bf16"):
            loadgen.paged_decode_attention(*bad, table, ctx)
    with pytest.raises(TypeError, match="int32"):
        loadgen.paged_decode_attention(q, kc, vc, table.long(), ctx)
    with pytest.raises(TypeError, match="int32"):
        loadgen.paged_decode_attention(q, kc, vc, table, ctx.long())


def test_wrapper_rejects_head_dim_block_size_and_ranks(host_operands_pass):
    for D in (64, 256):
        with pytest.raises(ValueError, match="head dim"):
            loadgen.paged_decode_attention(*_operands(D=D))
    for T in (16, 64):
        with pytest.raises(ValueError, match="block size"):
            loadgen.paged_decode_attention(*_operands(T=T))
    q, kc, vc, table, ctx = _operands()
    with pytest.raises(ValueError, match="head dim"):                # a V cache in K's layout
        loadgen.paged_decode_attention(q, kc, kc.clone(), table, ctx)
    with pytest.raises(ValueError, match="expects q"):
        loadgen.paged_decode_attention(q[0], kc, vc, table, ctx)
    with pytest.raises(ValueError, match="expects q"):
        loadgen.paged_decode_attention(q, kc, vc, table.flatten(), ctx)


@pytest.mark.parametrize("Hq,Hkv", [(3, 2), (6, 2), (32, 1), (12, 4)])
def test_wrapper_rejects_head_ratios(host_operands_pass, Hq, Hkv):
    with pytest.raises(ValueError, match="Hq / Hkv"):
        loadgen.paged_decode_attention(*_operands(Hq=Hq, Hkv=Hkv))


def test_wrapper_rejects_cache_layouts(host_operands_pass):
    q, kc, vc, table, ctx = _operands()
    with pytest.raises(ValueError, match="contiguous caches"):
        loadgen.paged_decode_attention(q, torch.zeros(6, 2, 32, 128, dtype=torch.bfloat16)[::2], vc, table, ctx)
    with pytest.raises(ValueError, match="contiguous caches"):
        loadgen.paged_decode_attention(q, kc, torch.zeros(3, 2, 32, 128, dtype=torch.bfloat16).transpose(2, 3), table, ctx)
    off = torch.zeros(3 * 2 * 32 * 128 + 8, dtype=torch.bfloat16)[4:-4]
    with pytest.raises(ValueError, match="16-byte"):
        loadgen.paged_decode_attention(q, off.view(3, 2, 32, 128), vc, table, ctx)
    with pytest.raises(ValueError, match="disagree"):
        loadgen.paged_decode_attention(q, kc, torch.zeros(4, 2, 128, 32, dtype=torch.bfloat16), table, ctx)
    with pytest.raises(ValueError, match="disagree"):
        loadgen.paged_decode_attention(q, kc, torch.zeros(3, 1, 128, 32, dtype=torch.bfloat16), table, ctx)


def test_wrapper_rejects_strides_and_alignment(host_operands_pass):
    q, kc, vc, table, ctx = _operands()
    W4 = 4 * 128
    short = torch.zeros(2 * W4 - 128, dtype=torch.bfloat16).as_strided((2, 4, 128), (W4 - 128, 128, 1))
    with pytest.raises(ValueError, match="sequence stride"):        # sequences overlap
        loadgen.paged_decode_attention(short, kc, vc, table, ctx)
    odd = torch.zeros(2, W4 + 4, dtype=torch.bfloat16)[:, :W4].unflatten(1, (4, 128))
    with pytest.raises(ValueError, match="multiple of 8"):
        loadgen.paged_decode_attention(odd, kc, vc, table, ctx)
    with pytest.raises(ValueError, match="multiple of 8"):
        loadgen.paged_decode_attention(q, kc, vc, table, ctx, out=odd)
    heads = torch.zeros(2, 4, 136, dtype=torch.bfloat16)[:, :, :128]                # head stride 136
    with pytest.raises(ValueError, match="slabs"):
        loadgen.paged_decode_attention(heads, kc, vc, table, ctx)
    with pytest.raises(ValueError, match="slabs"):
        loadgen.paged_decode_attention(q, kc, vc, table, ctx, out=torch.zeros(2, 128, 4, dtype=torch.bfloat16).transpose(1, 2))
    mis = torch.zeros(2 * W4 + 8, dtype=torch.bfloat16)[4:4 + 2 * W4].view(2, 4, 128)
    with pytest.raises(ValueError, match="16-byte"):
        loadgen.paged_decode_attention(mis, kc, vc, table, ctx)
    with pytest.raises(ValueError, match="16-byte"):
        loadgen.paged_decode_attention(q, kc, vc, table, ctx, out=mis)
    with pytest.raises(ValueError, match="block_table row"):
        loadgen.paged_decode_attention(q, kc, vc, torch.zeros(2, 2, dtype=torch.int32).T, ctx)
    with pytest.raises(ValueError, match="row stride"):
        loadgen.paged_decode_attention(q, kc, vc, torch.zeros(3, dtype=torch.int32).as_strided((2, 2), (1, 1)), ctx)
    with pytest.raises(ValueError, match="contiguous ctx_lens"):
        loadgen.paged_decode_attention(q, kc, vc, table, torch.ones(4, dtype=torch.int32)[::2])


def test_wrapper_rejects_mismatched_shapes(host_operands_pass):
    q, kc, vc, table, ctx = _operands()
    with pytest.raises(ValueError, match="do not match"):
        loadgen.paged_decode_attention(q, kc, vc, table[:1], ctx)
    with pytest.raises(ValueError, match="do not match"):
        loadgen.paged_decode_attention(q, kc, vc, table, torch.ones(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="bad output"):
        loadgen.paged_decode_attention(q, kc, vc, table, ctx, out=torch.zeros(2, 2, 128, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="bad output"):
        loadgen.paged_decode_attention(q, kc, vc, table, ctx, out=torch.zeros(2, 4, 128))


def test_no_sequences_launch_nothing(host_operands_pass):
    q, kc, vc, table, ctx = _operands()
    out = loadgen.paged_decode_attention(q[:0], kc, vc, table[:0], ctx[:0])
    assert out.shape == (0, 4, 128)


# ------------------------------------------------------------------------------------------------
# profiler and executor
# ------------------------------------------------------------------------------------------------
def test_decode_kernel_is_not_an_mfma_kernel():
    """The kernel is HBM-bound: its time must not count into mfma_share, although "attn" is one of
    the profiler's markers."""
    from k8s_gpu_scheduler_amd.agent import pod_profiler
    assert "attn" in pod_profiler.MFMA_KERNEL_MARKERS
    for name in ("paged_decode_kernel",
                 "gs::(anonymous namespace)::paged_decode_kernel(__bf16 const*, __bf16 const*, __bf16 const*, "
                 "int const*, int const*, __bf16*, int, int, unsigned long, unsigned long, unsigned long, float)",
                 "_ZN2gs12_GLOBAL__N_119paged_decode_kernelEPKDF16bS2_S2_PKiS4_PDF16biimmmf"):
        assert not pod_profiler.is_mfma_kernel(name), name
    assert pod_profiler.is_mfma_kernel("gemm_bf16_kernel")
    import os
    src = os.path.join(os.path.dirname(__file__), "..", "native", "hip", "decode_attn.hip")
    assert "paged_decode_kernel(" in open(src).read()


def test_enqueue_ops_dispatches_attn_without_the_check(monkeypatch):
    from k8s_gpu_scheduler_amd.parallel import executor
    calls = []
    monkeypatch.setattr(loadgen, "paged_decode_attention", lambda *a, **k: calls.append((a, k)))

    class Stub:
        ops = [(W.Op("attn", 1, 1, 32, rows=1), ("out", "q", "kc", "vc", "table", "ctx"))]

    executor.enqueue_ops(Stub(), 2, "stream", 0)
    assert calls == [(("q", "kc", "vc", "table", "ctx"), {"out": "out", "stream": "stream", "check": False})] * 2

    class Unknown:
        ops = [(W.Op("scatter"), ())]

    with pytest.raises(ValueError, match="scatter"):
        executor.enqueue_ops(Unknown(), 1, None, 0)


# ------------------------------------------------------------------------------------------------
# the GPU tests' reference
# ------------------------------------------------------------------------------------------------
def test_reference_agrees_with_sdpa_on_a_ragged_gqa_case():
    from test_gpu_decode_attn_exact import reference
    g = torch.Generator().manual_seed(5)
    Hq, Hkv, ctxs = 8, 2, [1, 31, 32, 33, 100, 0]
    S, need = len(ctxs), [-(-c // 32) for c in ctxs]
    NB = sum(need) + 2
    q = torch.randn(S, Hq, 128, generator=g, dtype=torch.float64)
    kc = torch.randn(NB, Hkv, 32, 128, generator=g, dtype=torch.float64)
    vc = torch.randn(NB, Hkv, 128, 32, generator=g, dtype=torch.float64)
    ids = torch.randperm(NB, generator=g).tolist()
    table = torch.full((S, max(need) + 1), -7, dtype=torch.int32)
    for s in range(S):
        table[s, :need[s]] = torch.tensor([ids.pop() for _ in range(need[s])], dtype=torch.int32)
    scale = 0.11
    out = reference(q, kc, vc, table, torch.tensor(ctxs, dtype=torch.int32), scale)
    assert out.dtype == torch.float64 and out.shape == (S, Hq, 128)
    for s, ctx in enumerate(ctxs):
        if ctx == 0:
            assert not out[s].any()
            continue
        # token by token, with none of the reference's indexing
        k = torch.stack([kc[int(table[s, t // 32]), :, t % 32, :] for t in range(ctx)], 1)          # [Hkv, ctx, D]
        v = torch.stack([vc[int(table[s, t // 32]), :, :, t % 32] for t in range(ctx)], 1)
        k, v = k.repeat_interleave(Hq // Hkv, 0), v.repeat_interleave(Hq // Hkv, 0)             # [Hq, ctx, D]
        ref = torch.nn.functional.scaled_dot_product_attention(q[s][:, None, :], k, v, scale=scale)[:, 0]
        assert (out[s] - ref).abs().max().item() <= 1e-12
