"""The paged-KV prefill attention without a GPU: the workload model's prefill op and the
llm_prefill_2048 workload, the pure-Python grid rule, the host wrapper's validation (which must fire
before the native module is touched), the profiler's kernel classification, the executor's op
dispatch and operands, and the float64 reference of the GPU tests.  The kernel itself is pinned on
the GPU by test_gpu_prefill_attn_exact.py."""
import os

import pytest
import torch

from k8s_gpu_scheduler_amd import _native
from k8s_gpu_scheduler_amd.models import workloads as W
from k8s_gpu_scheduler_amd.ops import loadgen


# ------------------------------------------------------------------------------------------------
# workload model
# ------------------------------------------------------------------------------------------------
def test_prefill_op_bytes_flops():
    o = W.Op("prefill", M=3, N=8, K=96, rows=2, q=40)
    assert not o.is_gemm and o.on_mfma and o.mfma_rate() == 1.0
    pairs = 40 * 56 + 40 * 41 / 2                       # every query sees the 56-token prefix; the triangle with its diagonal
    assert pairs == sum(56 + i + 1 for i in range(40))
    assert o.flops == 4 * 128 * 3 * 8 * pairs
    assert o.bytes == (4 * 3 * 2 * 96 * 128             # K and V, bf16, read once
                       + 4 * 3 * 40 * 8 * 128           # q and out
                       + 4 * 3 * 96 / 32 + 4 * 3 + 4 * 4)      # table entries, ctx_lens, q_start
    assert W.Op("gemm", 64, 64, 64).q == 0 and W.Op("gemm", 64, 64, 64, True, 0, 0) == W.Op("gemm", 64, 64, 64)
    assert [W.Op(k).on_mfma for k in ("gemm", "gemm8", "triad", "gather", "attn", "prefill")] == [True, True, False, False, False, True]
    one = W.Op("prefill", 1, 1, 1, rows=1, q=1)         # a single query on a single token: one pair
    assert one.flops == 4 * 128


def test_llm_prefill_workload_and_where_it_is_registered():
    w = W.get("llm_prefill_2048")
    assert W.workload_for_pod("llm-prefill-2048-x") is w and W.STAGED == {"llm_prefill_2048": w}
    assert len(W.CATALOG) == 18 and set(W.EXTRA) == {"fp8_llm_2048", "triad_only_2048", "dlrm_2048", "llm_decode_256"}
    assert W.workload_for_pod("llm-decode-256-x") is W.EXTRA["llm_decode_256"]
    assert (w.family, w.framework, w.batch, w.hbm_gib) == ("llm_prefill", "hip", 2048, 0.25)
    qkv, a, proj = w.ops
    assert a == W.Op("prefill", 2, 32, 4096, rows=8, q=1024)
    assert [(o.kind, o.M, o.N, o.K) for o in (qkv, proj)] == [("gemm", 2048, 6144, 4096), ("gemm", 2048, 4096, 4096)]
    assert qkv.M == a.M * a.q and qkv.N == (a.N + 2 * a.rows) * W.ATTN_HEAD_DIM and proj.K == a.N * W.ATTN_HEAD_DIM
    cache_bytes = 2 * a.M * a.K * a.rows * W.ATTN_HEAD_DIM * 2
    assert cache_bytes == 32 << 20 and w.hbm_gib * (1 << 30) >= cache_bytes
    assert a.K % W.ATTN_BLOCK_TOKENS == 0 and a.N // a.rows in loadgen.ATTN_GROUPS and a.q <= a.K
    assert a.flops == pytest.approx(1.2e11, rel=0.01) and qkv.flops + proj.flops == pytest.approx(1.7e11, rel=0.02)
    with pytest.raises(KeyError):
        W.get("llm_prefill")


def test_llm_prefill_roofline():
    w = W.get("llm_prefill_2048")
    qkv, a, proj = w.ops
    t = W.roofline_seconds(w, 1.0)
    assert t == pytest.approx(sum(max(o.flops / 1100e12, o.bytes / 5.5e12) for o in w.ops))
    assert a.flops / 1100e12 > a.bytes / 5.5e12                                      # the prefill is MFMA-bound
    m, h = W.roofline_split("llm-prefill-2048-x", tflops=1.0e3, tbps=6.0)
    assert h == 0.0 and m == pytest.approx((qkv.flops + a.flops + proj.flops) / 1.0e15)
    assert 0.0 < W.cu_fill(w) <= 1.0


def test_default_prefill_workgroups():
    got = [W.default_prefill_workgroups(*x) for x in ((1, 1, 1, 1), (1, 1, 1, 128), (1, 1, 1, 129), (2, 32, 8, 1024),
                                                      (8, 8, 2, 33), (3, 16, 1, 9), (5, 4, 4, 0), (0, 8, 8, 64))]
    assert got == [1, 1, 2, 512, 32, 6, 0, 0]


@pytest.mark.skipif(_native.hip(required=False) is None, reason="HIP extension not built")
def test_default_prefill_workgroups_match_the_native_rule():
    h = _native.hip()
    for s in (0, 1, 7, 256):
        for hq, hkv in ((1, 1), (8, 8), (8, 2), (32, 8), (16, 1), (128, 8)):
            for mq in (0, 1, 8, 31, 32, 33, 127, 128, 129, 1024, 100000):
                assert h.paged_prefill_workgroups(s, hq, hkv, mq) == W.default_prefill_workgroups(s, hq, hkv, mq), (s, hq, hkv, mq)


def test_prefill_cu_fill_counts_workgroups():
    one = W.Workload("a", "llm_prefill", "hip", 1, (W.Op("prefill", 2, 32, 1024, rows=8, q=256),), 0.0)
    assert W.cu_fill(one) == pytest.approx(128 / W.CUS)             # 2 sequences x 8 KV heads x 8 column tiles
    assert W.cu_fill(W.Workload("a", "llm_prefill", "hip", 1, (W.Op("prefill", 2, 32, 4096, rows=8, q=1024),), 0.0)) == 1.0


# ------------------------------------------------------------------------------------------------
# host wrapper: every rejection happens before the native module is asked for
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def no_native(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the native module was touched")
    monkeypatch.setattr(_native, "hip", boom)


def _operands(S=2, Tq=5, Hq=4, Hkv=2, NB=3, MB=2, D=128, T=32):
    q = torch.zeros(Tq, Hq, D, dtype=torch.bfloat16)
    kc = torch.zeros(NB, Hkv, T, D, dtype=torch.bfloat16)
    vc = torch.zeros(NB, Hkv, D, T, dtype=torch.bfloat16)
    table = torch.zeros(S, MB, dtype=torch.int32)
    ctx = torch.full((S,), 8, dtype=torch.int32)
    q_start = torch.linspace(0, Tq, S + 1).to(torch.int32)
    return q, kc, vc, table, ctx, q_start


def test_wrapper_rejects_cpu_tensors(no_native):
    q, kc, vc, table, ctx, qs = _operands()
    with pytest.raises(ValueError, match="device tensors"):
        loadgen.paged_prefill_attention(q, kc, vc, table, ctx, qs)
    with pytest.raises(ValueError, match="device tensors"):          # before any dtype complaint
        loadgen.paged_prefill_attention(q.float(), kc, vc, table.long(), ctx, qs.long())


@pytest.fixture
def host_operands_pass(monkeypatch, no_native):
    """The remaining checks need tensors that pass the device check; without a GPU the check is
    stubbed out, and everything after it up to the native call runs on host tensors."""
    monkeypatch.setattr(loadgen, "_check_devices", lambda name, *ts: torch.device("cpu"))


def test_wrapper_rejects_dtypes(host_operands_pass):
    q, kc, vc, table, ctx, qs = _operands()
    for bad in ((q.float(), kc, vc), (q, kc.half(), vc), (q, kc, vc.float())):
        with pytest.raises(TypeError, match="bf16"):
            loadgen.paged_prefill_attention(*bad, table, ctx, qs)
    with pytest.raises(TypeError, match="int32"):
        loadgen.paged_prefill_attention(q, kc, vc, table.long(), ctx, qs)
    with pytest.raises(TypeError, match="int32"):
        loadgen.paged_prefill_attention(q, kc, vc, table, ctx.long(), qs)
    with pytest.raises(TypeError, match="int32 q_start"):
        loadgen.paged_prefill_attention(q, kc, vc, table, ctx, qs.long())


def test_wrapper_rejects_head_dim_block_size_and_ranks(host_operands_pass):
    for D in (64, 256):
        with pytest.raises(ValueError, match="head dim"):
            loadgen.paged_prefill_attention(*_operands(D=D))
    for T in (16, 64):
        with pytest.raises(ValueError, match="block size"):
            loadgen.paged_prefill_attention(*_operands(T=T))
    q, kc, vc, table, ctx, qs = _operands()
    with pytest.raises(ValueError, match="head dim"):                # a V cache in K's layout
        loadgen.paged_prefill_attention(q, kc, kc.clone(), table, ctx, qs)
    with pytest.raises(ValueError, match=r"expects q \[Tq"):
        loadgen.paged_prefill_attention(q[0], kc, vc, table, ctx, qs)
    with pytest.raises(ValueError, match=r"expects q \[Tq"):
        loadgen.paged_prefill_attention(q, kc, vc, table.flatten(), ctx, qs)
    with pytest.raises(ValueError, match=r"expects q \[Tq"):
        loadgen.paged_prefill_attention(q, kc, vc, table, ctx[:, None], qs)


@pytest.mark.parametrize("Hq,Hkv", [(3, 2), (6, 2), (32, 1), (12, 4)])
def test_wrapper_rejects_head_ratios(host_operands_pass, Hq, Hkv):
    with pytest.raises(ValueError, match="Hq / Hkv"):
        loadgen.paged_prefill_attention(*_operands(Hq=Hq, Hkv=Hkv))


def test_wrapper_rejects_cache_layouts(host_operands_pass):
    q, kc, vc, table, ctx, qs = _operands()
    with pytest.raises(ValueError, match="contiguous caches"):
        loadgen.paged_prefill_attention(q, torch.zeros(6, 2, 32, 128, dtype=torch.bfloat16)[::2], vc, table, ctx, qs)
    with pytest.raises(ValueError, match="contiguous caches"):
        loadgen.paged_prefill_attention(q, kc, torch.zeros(3, 2, 32, 128, dtype=torch.bfloat16).transpose(2, 3), table, ctx, qs)
    off = torch.zeros(3 * 2 * 32 * 128 + 8, dtype=torch.bfloat16)[4:-4]
    with pytest.raises(ValueError, match="16-byte"):
        loadgen.paged_prefill_attention(q, off.view(3, 2, 32, 128), vc, table, ctx, qs)
    with pytest.raises(ValueError, match="disagree"):
        loadgen.paged_prefill_attention(q, kc, torch.zeros(4, 2, 128, 32, dtype=torch.bfloat16), table, ctx, qs)
    with pytest.raises(ValueError, match="disagree"):
        loadgen.paged_prefill_attention(q, kc, torch.zeros(3, 1, 128, 32, dtype=torch.bfloat16), table, ctx, qs)


def test_wrapper_rejects_strides_and_alignment(host_operands_pass):
    q, kc, vc, table, ctx, qs = _operands()
    W4 = 4 * 128
    short = torch.zeros(5 * W4, dtype=torch.bfloat16).as_strided((5, 4, 128), (W4 - 128, 128, 1))
    with pytest.raises(ValueError, match="token stride"):           # tokens overlap
        loadgen.paged_prefill_attention(short, kc, vc, table, ctx, qs)
    odd = torch.zeros(5, W4 + 4, dtype=torch.bfloat16)[:, :W4].unflatten(1, (4, 128))
    with pytest.raises(ValueError, match="multiple of 8"):
        loadgen.paged_prefill_attention(odd, kc, vc, table, ctx, qs)
    with pytest.raises(ValueError, match="multiple of 8"):
        loadgen.paged_prefill_attention(q, kc, vc, table, ctx, qs, out=odd)
    heads = torch.zeros(5, 4, 136, dtype=torch.bfloat16)[:, :, :128]                # head stride 136
    with pytest.raises(ValueError, match="slabs"):
        loadgen.paged_prefill_attention(heads, kc, vc, table, ctx, qs)
    with pytest.raises(ValueError, match="slabs"):
        loadgen.paged_prefill_attention(q, kc, vc, table, ctx, qs, out=torch.zeros(5, 128, 4, dtype=torch.bfloat16).transpose(1, 2))
    mis = torch.zeros(5 * W4 + 8, dtype=torch.bfloat16)[4:4 + 5 * W4].view(5, 4, 128)
    with pytest.raises(ValueError, match="16-byte"):
        loadgen.paged_prefill_attention(mis, kc, vc, table, ctx, qs)
    with pytest.raises(ValueError, match="16-byte"):
        loadgen.paged_prefill_attention(q, kc, vc, table, ctx, qs, out=mis)
    with pytest.raises(ValueError, match="block_table row"):
        loadgen.paged_prefill_attention(q, kc, vc, torch.zeros(2, 2, dtype=torch.int32).T, ctx, qs)
    with pytest.raises(ValueError, match="row stride"):
        loadgen.paged_prefill_attention(q, kc, vc, torch.zeros(3, dtype=torch.int32).as_strided((2, 2), (1, 1)), ctx, qs)
    with pytest.raises(ValueError, match="contiguous ctx_lens"):
        loadgen.paged_prefill_attention(q, kc, vc, table, torch.ones(4, dtype=torch.int32)[::2], qs)


def test_wrapper_rejects_q_start_and_mismatched_shapes(host_operands_pass):
    q, kc, vc, table, ctx, qs = _operands()
    with pytest.raises(ValueError, match="q_start must be 1-D"):
        loadgen.paged_prefill_attention(q, kc, vc, table, ctx, qs[None, :])
    with pytest.raises(ValueError, match="q_start must be 1-D"):
        loadgen.paged_prefill_attention(q, kc, vc, table, ctx, qs[:0])
    with pytest.raises(ValueError, match="contiguous q_start"):
        loadgen.paged_prefill_attention(q, kc, vc, table, ctx, torch.zeros(6, dtype=torch.int32)[::2])
    with pytest.raises(ValueError, match="do not match the 3 sequences of q_start"):            # one entry too many
        loadgen.paged_prefill_attention(q, kc, vc, table, ctx, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="do not match"):
        loadgen.paged_prefill_attention(q, kc, vc, table[:1], ctx, qs)
    with pytest.raises(ValueError, match="do not match"):
        loadgen.paged_prefill_attention(q, kc, vc, table, torch.ones(3, dtype=torch.int32), qs)
    with pytest.raises(ValueError, match="bad output"):
        loadgen.paged_prefill_attention(q, kc, vc, table, ctx, qs, out=torch.zeros(4, 4, 128, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="bad output"):
        loadgen.paged_prefill_attention(q, kc, vc, table, ctx, qs, out=torch.zeros(5, 4, 128))
    with pytest.raises(ValueError, match="check=False needs max_q_len"):
        loadgen.paged_prefill_attention(q, kc, vc, table, ctx, qs, check=False)
    with pytest.raises(ValueError, match="max_q_len"):
        loadgen.paged_prefill_attention(q, kc, vc, table, ctx, qs, max_q_len=-1)


def test_no_sequences_no_tokens_and_no_chunk_launch_nothing(host_operands_pass):
    q, kc, vc, table, ctx, qs = _operands()
    out = loadgen.paged_prefill_attention(q, kc, vc, table[:0], ctx[:0], qs[:1])                 # S == 0
    assert out.shape == (5, 4, 128)
    out = loadgen.paged_prefill_attention(q[:0], kc, vc, table, ctx, torch.zeros(3, dtype=torch.int32))     # Tq == 0
    assert out.shape == (0, 4, 128)
    given = torch.ones(5, 4, 128, dtype=torch.bfloat16)
    assert loadgen.paged_prefill_attention(q, kc, vc, table, ctx, qs, max_q_len=0, out=given, check=False) is given
    assert bool((given == 1).all())


# ------------------------------------------------------------------------------------------------
# profiler and executor
# ------------------------------------------------------------------------------------------------
def test_prefill_kernel_is_an_mfma_kernel():
    """The kernel is MFMA-bound: its time counts into mfma_share through the profiler's "attn" marker."""
    from k8s_gpu_scheduler_amd.agent import pod_profiler
    for name in ("paged_prefill_attn_kernel",
                 "gs::(anonymous namespace)::paged_prefill_attn_kernel(__bf16 const*, __bf16 const*, __bf16 const*, "
                 "int const*, int const*, int const*, __bf16*, int, int, int, unsigned long, unsigned long, unsigned long, float)",
                 "_ZN2gs12_GLOBAL__N_125paged_prefill_attn_kernelEPKDF16bS2_S2_PKiS4_S4_PDF16biiimmmf"):
        assert pod_profiler.is_mfma_kernel(name), name
    assert not pod_profiler.is_mfma_kernel("paged_decode_kernel")
    src = os.path.join(os.path.dirname(__file__), "..", "native", "hip", "prefill_attn.hip")
    assert "paged_prefill_attn_kernel(" in open(src).read()


def test_enqueue_ops_dispatches_prefill_without_the_check(monkeypatch):
    from k8s_gpu_scheduler_amd.parallel import executor
    calls = []
    monkeypatch.setattr(loadgen, "paged_prefill_attention", lambda *a, **k: calls.append((a, k)))

    class Stub:
        ops = [(W.Op("prefill", 1, 1, 64, rows=1, q=40), ("out", "q", "kc", "vc", "table", "ctx", "q_start"))]

    executor.enqueue_ops(Stub(), 2, "stream", 0)
    assert calls == [(("q", "kc", "vc", "table", "ctx", "q_start"),
                      {"max_q_len": 40, "out": "out", "stream": "stream", "check": False})] * 2
    assert executor.op_output(*Stub.ops[0]) == "out"


def test_buffers_build_prefill_operands_reproducibly():
    from k8s_gpu_scheduler_amd.parallel.executor import _Buffers
    o = W.Op("prefill", 3, 4, 96, rows=2, q=40)
    w = W.Workload("t_prefill", "test", "hip", 3, (o,), 0.0)
    cpu = torch.device("cpu")
    a, b = _Buffers(w, cpu), _Buffers(w, cpu)
    out, q, kc, vc, table, ctx, q_start = a.ops[0][1]
    assert out.shape == q.shape == (120, 4, 128) and out.dtype == q.dtype == torch.bfloat16
    assert kc.shape == (9, 2, 32, 128) and vc.shape == (9, 2, 128, 32)
    assert table.shape == (3, 3) and table.dtype == torch.int32 and sorted(table.flatten().tolist()) == list(range(9))
    assert ctx.tolist() == [96, 96, 96] and q_start.tolist() == [0, 40, 80, 120] and q_start.dtype == torch.int32
    assert float(kc.abs().max()) <= 127 / 64 and float(vc.abs().max()) <= 127 / 64
    for x, y in zip(a.ops[0][1][1:], b.ops[0][1][1:]):
        assert torch.equal(x.view(torch.int16) if x.dtype == torch.bfloat16 else x, y.view(torch.int16) if y.dtype == torch.bfloat16 else y)
    for bad, msg in ((W.Op("prefill", 3, 4, 100, rows=2, q=40), "workload t_bad: attention context 100 is no multiple of 32"),
                     (W.Op("prefill", 3, 4, 96, rows=2, q=97), "workload t_bad: prefill chunk 97 is longer than the context 96")):
        with pytest.raises(ValueError, match=msg):
            _Buffers(W.Workload("t_bad", "test", "hip", 3, (bad,), 0.0), cpu)


# ------------------------------------------------------------------------------------------------
# the GPU tests' reference
# ------------------------------------------------------------------------------------------------
def test_reference_agrees_with_masked_sdpa_on_a_ragged_gqa_case():
    from test_gpu_prefill_attn_exact import reference
    g = torch.Generator().manual_seed(6)
    Hq, Hkv = 8, 2
    seqs = [(1, 1), (31, 31), (100, 37), (64, 0), (33, 1), (0, 0), (70, 70)]              # (ctx, q_len)
    S, need = len(seqs), [-(-c // 32) for c, _ in seqs]
    NB, lead = sum(need) + 2, 2
    Tq = lead + sum(n for _, n in seqs) + 3
    q = torch.randn(Tq, Hq, 128, generator=g, dtype=torch.float64)
    kc = torch.randn(NB, Hkv, 32, 128, generator=g, dtype=torch.float64)
    vc = torch.randn(NB, Hkv, 128, 32, generator=g, dtype=torch.float64)
    ids = torch.randperm(NB, generator=g).tolist()
    table = torch.full((S, max(need) + 1), -7, dtype=torch.int32)
    for s in range(S):
        table[s, :need[s]] = torch.tensor([ids.pop() for _ in range(need[s])], dtype=torch.int32)
    q_start = torch.tensor([lead] + [n for _, n in seqs]).cumsum(0).to(torch.int32)
    scale = 0.11
    out = reference(q, kc, vc, table, torch.tensor([c for c, _ in seqs], dtype=torch.int32), q_start, scale)
    assert out.dtype == torch.float64 and out.shape == (Tq, Hq, 128)
    assert not out[:lead].any() and not out[int(q_start[-1]):].any()
    for s, (ctx, n) in enumerate(seqs):
        if n == 0:
            continue
        # token by token, with none of the reference's indexing, and an explicit boolean mask
        k = torch.stack([kc[int(table[s, t // 32]), :, t % 32, :] for t in range(ctx)], 1)          # [Hkv, ctx, D]
        v = torch.stack([vc[int(table[s, t // 32]), :, :, t % 32] for t in range(ctx)], 1)
        k, v = k.repeat_interleave(Hq // Hkv, 0), v.repeat_interleave(Hq // Hkv, 0)             # [Hq, ctx, D]
        mask = torch.tensor([[t <= ctx - n + i for t in range(ctx)] for i in range(n)])
        r0 = int(q_start[s])
        ref = torch.nn.functional.scaled_dot_product_attention(q[r0:r0 + n].transpose(0, 1), k, v, attn_mask=mask, scale=scale)
        assert (out[r0:r0 + n] - ref.transpose(0, 1)).abs().max().item() <= 1e-12
