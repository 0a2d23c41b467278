"""The RoPE + paged-KV append without a GPU: the workload model's rope_append op, the two LLM-layer
workloads and their table, the pure-Python grid rule, rope_table, the host wrapper's validation (which
must fire before the native module is touched), the executor's op dispatch and operands, and the float64
reference of the GPU tests.  The kernel itself is pinned on the GPU by test_gpu_rope_append_exact.py."""
import math

import pytest
import torch

from k8s_gpu_scheduler_amd import _native
from k8s_gpu_scheduler_amd.models import workloads as W
from k8s_gpu_scheduler_amd.ops import loadgen


# ------------------------------------------------------------------------------------------------
# workload model
# ------------------------------------------------------------------------------------------------
def test_rope_append_op_flops_bytes_workgroups():
    o = W.Op("rope_append", M=3, N=8, K=70, rows=2, q=40)           # tokens 30 .. 69 of each sequence: blocks 0 .. 2
    assert not o.is_gemm and not o.on_mfma and o.mfma_rate() == 1.0
    assert o.flops == 3 * 128 * (8 + 2) * 3 * 40 == 460800
    assert o.bytes == (2 * 120 * 12 * 128            # qkv read
                       + 2 * 120 * 8 * 128           # q_out written
                       + 2 * 120 * 2 * 2 * 128       # K and V written
                       + 512 * 120                   # a cos / sin row per token
                       + 4 * 3 + 4 * 4 + 4 * 3 * 3)  # ctx_lens, q_start, three touched table entries per sequence
    assert o.bytes == 798784
    assert o.workgroups(0) == o.workgroups(64) == 3 * 2 * 3 == 18   # (40 + 30) // 32 + 1 = 3 blocks a chunk can touch
    d = W.Op("rope_append", M=5, N=4, K=33, rows=4, q=1)            # decode: token 32, slot 0 of block 1
    assert d.flops == 3 * 128 * 8 * 5 == 15360
    assert d.bytes == 2 * 5 * 12 * 128 + 2 * 5 * 4 * 128 + 2 * 5 * 8 * 128 + 512 * 5 + 20 + 24 + 20 == 33344
    assert d.workgroups(0) == 5 * 4                                  # one per (sequence, KV head)
    assert W.Op("rope_append", 2, 4, 64, rows=4, q=0).bytes == 4 * 2 + 4 * 3 and W.Op("rope_append", 2, 4, 64, rows=4, q=0).flops == 0


def test_default_rope_append_workgroups():
    got = [W.default_rope_append_workgroups(*x) for x in ((1, 1, 1), (1, 1, 2), (1, 1, 33), (1, 1, 34), (2, 8, 1024),
                                                          (256, 8, 1), (8, 2, 257), (5, 4, 0), (0, 8, 64))]
    assert got == [1, 2, 2, 3, 528, 2048, 144, 0, 0]
    # the rule is the most blocks a chunk of L tokens can touch, reached from slot 31
    for L in (1, 2, 31, 32, 33, 34, 64, 65, 66, 257):
        most = max((s + L - 1) // 32 + 1 for s in range(32))
        assert W.default_rope_append_workgroups(1, 1, L) == most == (31 + L - 1) // 32 + 1


@pytest.mark.skipif(_native.hip(required=False) is None, reason="HIP extension not built")
def test_default_rope_append_workgroups_match_the_native_rule():
    h = _native.hip()
    for s in (0, 1, 7, 256):
        for hkv in (1, 2, 8):
            for mq in (0, 1, 2, 3, 31, 32, 33, 34, 35, 1024, 100000):
                assert h.rope_append_workgroups(s, hkv, mq) == W.default_rope_append_workgroups(s, hkv, mq), (s, hkv, mq)


def test_llm_layer_workloads_and_their_table():
    dec, pre = W.get("llm_layer_decode_256"), W.get("llm_layer_prefill_2048")
    assert W.LLM_LAYER == {"llm_layer_decode_256": dec, "llm_layer_prefill_2048": pre}
    assert dec.ops == (W.Op("gemm", 256, 6144, 4096), W.Op("rope_append", 256, 32, 1024, rows=8, q=1),
                       W.Op("attn", 256, 32, 1024, rows=8), W.Op("gemm", 256, 4096, 4096))
    assert pre.ops == (W.Op("gemm", 2048, 6144, 4096), W.Op("rope_append", 2, 32, 4096, rows=8, q=1024),
                       W.Op("prefill", 2, 32, 4096, rows=8, q=1024), W.Op("gemm", 2048, 4096, 4096))
    assert (dec.family, dec.framework, dec.batch, dec.hbm_gib) == ("llm_layer_decode", "hip", 256, 2.25)
    assert (pre.family, pre.framework, pre.batch, pre.hbm_gib) == ("llm_layer_prefill", "hip", 2048, 0.5)
    for w in (dec, pre):
        qkv, a, att, proj = w.ops
        assert qkv.M == a.M * a.q and qkv.N == (a.N + 2 * a.rows) * W.ATTN_HEAD_DIM and proj.K == a.N * W.ATTN_HEAD_DIM
        assert (att.M, att.N, att.K, att.rows) == (a.M, a.N, a.K, a.rows) and a.N // a.rows in loadgen.ATTN_GROUPS
        caches = 2 * (2 * a.M * a.K * a.rows * W.ATTN_HEAD_DIM * 2)                 # each op keeps its own K and V
        assert w.hbm_gib * (1 << 30) >= caches and 0.0 < W.cu_fill(w) <= 1.0
        m, h = W.roofline_split(w.name.replace("_", "-") + "-0")
        assert h >= a.bytes / 6.0e12 > 0 and m > 0
    assert dec.ops[1].workgroups(64) == 2048 and pre.ops[1].workgroups(64) == 528
    # the older tables are unchanged, and hold none of the new kind
    assert len(W.CATALOG) == 18 and set(W.EXTRA) == {"fp8_llm_2048", "triad_only_2048", "dlrm_2048", "llm_decode_256"}
    assert set(W.STAGED) == {"llm_prefill_2048"} and set(W.LONG_CONTEXT) == {"llm_decode_long_8"}
    for table in (W.CATALOG, W.EXTRA, W.STAGED, W.LONG_CONTEXT):
        assert all(o.kind != "rope_append" for w in table.values() for o in w.ops)


def test_get_and_workload_for_pod():
    dec, pre = W.LLM_LAYER["llm_layer_decode_256"], W.LLM_LAYER["llm_layer_prefill_2048"]
    assert W.workload_for_pod("llm-layer-decode-256-x") is dec and W.workload_for_pod("pod-llm-layer-prefill-2048-7") is pre
    assert W.workload_for_pod("llm-decode-256-x") is W.EXTRA["llm_decode_256"]
    assert W.workload_for_pod("llm-prefill-2048-x") is W.STAGED["llm_prefill_2048"]
    assert W.workload_for_pod("llm-decode-long-8-x") is W.LONG_CONTEXT["llm_decode_long_8"]
    assert W.workload_for_pod("onnx-resnet50-1024-3") is W.CATALOG["onnx_resnet50_1024"]
    # a pod name that holds an old and a new name: the older tables are consulted first
    assert W.workload_for_pod("llm-layer-decode-256-and-llm-decode-256") is W.EXTRA["llm_decode_256"]
    names = [n for t in (W.CATALOG, W.EXTRA, W.STAGED, W.LONG_CONTEXT) for n in t]
    for new in W.LLM_LAYER:
        assert not any(old in new or new in old for old in names)
    assert W.get("llm_decode_256") is W.EXTRA["llm_decode_256"] and W.get("onnx_resnet50_1024") is W.CATALOG["onnx_resnet50_1024"]
    for bad in ("llm_layer", "llm_layer_decode", "llm-layer-decode-256"):
        with pytest.raises(KeyError):
            W.get(bad)
    with pytest.raises(KeyError):
        W.workload_for_pod("llm-layer-decode-255")


# ------------------------------------------------------------------------------------------------
# rope_table
# ------------------------------------------------------------------------------------------------
def test_rope_table():
    t = loadgen.rope_table(300)
    assert t.shape == (300, 128) and t.dtype == torch.float32 and t.device.type == "cpu" and t.is_contiguous()
    assert torch.equal(t[0], torch.cat([torch.ones(64), torch.zeros(64)]))
    for p, i in ((1, 0), (1, 63), (7, 1), (255, 0), (299, 17), (128, 32), (299, 63)):
        a = p * 500000.0 ** (-i / 64)
        assert abs(float(t[p, i]) - math.cos(a)) <= 2.0 ** -24 and abs(float(t[p, 64 + i]) - math.sin(a)) <= 2.0 ** -24, (p, i)
    b = loadgen.rope_table(5, base=10000.0)
    assert abs(float(b[3, 64 + 32]) - math.sin(3 * 10000.0 ** -0.5)) <= 2.0 ** -24
    assert loadgen.rope_table(0).shape == (0, 128)
    with pytest.raises(ValueError):
        loadgen.rope_table(-1)


# ------------------------------------------------------------------------------------------------
# host wrapper: every rejection happens before the native module is asked for
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def no_native(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the native module was touched")
    monkeypatch.setattr(_native, "hip", boom)


def _operands(S=2, Tq=5, Hq=4, Hkv=2, NB=3, MB=2, D=128, T=32, P=64):
    qkv = torch.zeros(Tq, Hq + 2 * Hkv, D, dtype=torch.bfloat16)
    cs = torch.zeros(P, 128)
    kc = torch.zeros(NB, Hkv, T, D, dtype=torch.bfloat16)
    vc = torch.zeros(NB, Hkv, D, T, dtype=torch.bfloat16)
    table = torch.zeros(S, MB, dtype=torch.int32)
    ctx = torch.full((S,), 8, dtype=torch.int32)
    q_start = torch.linspace(0, Tq, S + 1).to(torch.int32)
    return qkv, cs, kc, vc, table, ctx, q_start


def test_wrapper_rejects_cpu_tensors(no_native):
    with pytest.raises(ValueError, match="device tensors"):
        loadgen.rope_append(*_operands())
    qkv, cs, kc, vc, table, ctx, qs = _operands()
    with pytest.raises(ValueError, match="device tensors"):          # before any dtype complaint
        loadgen.rope_append(qkv.float(), cs.double(), kc, vc, table.long(), ctx, qs)


@pytest.fixture
def host_operands_pass(monkeypatch, no_native):
    """The remaining checks need tensors that pass the device check; without a GPU the check is
    stubbed out, and everything after it up to the native call runs on host tensors."""
    monkeypatch.setattr(loadgen, "_check_devices", lambda name, *ts: torch.device("cpu"))


def test_wrapper_rejects_dtypes(host_operands_pass):
    qkv, cs, kc, vc, table, ctx, qs = _operands()
    for bad in ((qkv.float(), cs, kc, vc), (qkv, cs, kc.half(), vc), (qkv, cs, kc, vc.float())):
        with pytest.raises(TypeError, match="bf16"):
            loadgen.rope_append(*bad, table, ctx, qs)
    for bad in (cs.double(), cs.to(torch.bfloat16)):
        with pytest.raises(TypeError, match="fp32 cos_sin"):
            loadgen.rope_append(qkv, bad, kc, vc, table, ctx, qs)
    with pytest.raises(TypeError, match="int32"):
        loadgen.rope_append(qkv, cs, kc, vc, table.long(), ctx, qs)
    with pytest.raises(TypeError, match="int32"):
        loadgen.rope_append(qkv, cs, kc, vc, table, ctx.long(), qs)
    with pytest.raises(TypeError, match="int32 q_start"):
        loadgen.rope_append(qkv, cs, kc, vc, table, ctx, qs.long())


def test_wrapper_rejects_ranks_head_dim_and_block_size(host_operands_pass):
    qkv, cs, kc, vc, table, ctx, qs = _operands()
    for bad in ((qkv[0], cs, kc, vc, table, ctx), (qkv, cs[0], kc, vc, table, ctx), (qkv, cs, kc[0], vc, table, ctx),
                (qkv, cs, kc, vc[0], table, ctx), (qkv, cs, kc, vc, table.flatten(), ctx), (qkv, cs, kc, vc, table, ctx[:, None])):
        with pytest.raises(ValueError, match=r"rope_append expects qkv \[Tq, Hq \+ 2 \* Hkv, 128\], cos_sin \[max_pos, 128\]"):
            loadgen.rope_append(*bad, qs)
    for D in (64, 256):
        with pytest.raises(ValueError, match="head dim"):
            loadgen.rope_append(*_operands(D=D))
    for T in (16, 64):
        with pytest.raises(ValueError, match="block size"):
            loadgen.rope_append(*_operands(T=T))
    with pytest.raises(ValueError, match="head dim"):                # a V cache in K's layout
        loadgen.rope_append(qkv, cs, kc, kc.clone(), table, ctx, qs)
    with pytest.raises(ValueError, match="disagree"):
        loadgen.rope_append(qkv, cs, kc, torch.zeros(3, 1, 128, 32, dtype=torch.bfloat16), table, ctx, qs)


def test_wrapper_rejects_head_counts(host_operands_pass):
    qkv, cs, kc, vc, table, ctx, qs = _operands()
    for heads in (4, 3, 1):                                          # 2 * Hkv = 4 of them are K and V: no q head left
        with pytest.raises(ValueError, match=r"no Hq \+ 2 \* Hkv"):
            loadgen.rope_append(qkv[:, :heads], cs, kc, vc, table, ctx, qs)
    for Hq, Hkv in ((3, 2), (6, 2), (32, 1), (12, 4)):
        with pytest.raises(ValueError, match="Hq / Hkv"):
            loadgen.rope_append(*_operands(Hq=Hq, Hkv=Hkv))
    for Hq, Hkv in ((1, 1), (4, 2), (16, 4), (8, 1), (32, 2)):
        assert loadgen.rope_append(*_operands(Hq=Hq, Hkv=Hkv), max_q_len=0).shape == (5, Hq, 128)


def test_wrapper_rejects_cache_and_table_layouts(host_operands_pass):
    qkv, cs, kc, vc, table, ctx, qs = _operands()
    with pytest.raises(ValueError, match="contiguous caches"):
        loadgen.rope_append(qkv, cs, torch.zeros(6, 2, 32, 128, dtype=torch.bfloat16)[::2], vc, table, ctx, qs)
    off = torch.zeros(3 * 2 * 32 * 128 + 8, dtype=torch.bfloat16)[4:-4]
    with pytest.raises(ValueError, match="16-byte"):
        loadgen.rope_append(qkv, cs, off.view(3, 2, 32, 128), vc, table, ctx, qs)
    with pytest.raises(ValueError, match=r"cos_sin must be \[max_pos, 128\]"):
        loadgen.rope_append(qkv, torch.zeros(64, 64), kc, vc, table, ctx, qs)
    with pytest.raises(ValueError, match="cos_sin must be contiguous"):
        loadgen.rope_append(qkv, torch.zeros(64, 136)[:, :128], kc, vc, table, ctx, qs)
    with pytest.raises(ValueError, match="cos_sin must be contiguous and 16-byte"):
        loadgen.rope_append(qkv, torch.zeros(64 * 128 + 4)[2:-2].view(64, 128), kc, vc, table, ctx, qs)
    with pytest.raises(ValueError, match="block_table row"):
        loadgen.rope_append(qkv, cs, kc, vc, torch.zeros(2, 2, dtype=torch.int32).T, ctx, qs)
    with pytest.raises(ValueError, match="contiguous ctx_lens"):
        loadgen.rope_append(qkv, cs, kc, vc, table, torch.ones(4, dtype=torch.int32)[::2], qs)


def test_wrapper_rejects_strides_alignment_and_overlap(host_operands_pass):
    qkv, cs, kc, vc, table, ctx, qs = _operands()
    W8, W4 = 8 * 128, 4 * 128
    short = torch.zeros(5 * W8, dtype=torch.bfloat16).as_strided((5, 8, 128), (W8 - 128, 128, 1))
    with pytest.raises(ValueError, match="qkv token stride"):        # tokens overlap
        loadgen.rope_append(short, cs, kc, vc, table, ctx, qs)
    # a stride that would do for the q heads alone is too short for q | K | V
    with pytest.raises(ValueError, match="qkv token stride 512"):
        loadgen.rope_append(torch.zeros(5 * W8, dtype=torch.bfloat16).as_strided((5, 8, 128), (W4, 128, 1)), cs, kc, vc, table, ctx, qs)
    odd = torch.zeros(5, W8 + 4, dtype=torch.bfloat16)[:, :W8].unflatten(1, (8, 128))
    with pytest.raises(ValueError, match="multiple of 8"):
        loadgen.rope_append(odd, cs, kc, vc, table, ctx, qs)
    heads = torch.zeros(5, 8, 136, dtype=torch.bfloat16)[:, :, :128]
    with pytest.raises(ValueError, match="qkv must have contiguous"):
        loadgen.rope_append(heads, cs, kc, vc, table, ctx, qs)
    mis = torch.zeros(5 * W8 + 8, dtype=torch.bfloat16)[4:4 + 5 * W8].view(5, 8, 128)
    with pytest.raises(ValueError, match="16-byte"):
        loadgen.rope_append(mis, cs, kc, vc, table, ctx, qs)
    out_odd = torch.zeros(5, W4 + 4, dtype=torch.bfloat16)[:, :W4].unflatten(1, (4, 128))
    with pytest.raises(ValueError, match="out token stride"):
        loadgen.rope_append(qkv, cs, kc, vc, table, ctx, qs, q_out=out_odd)
    with pytest.raises(ValueError, match="slabs"):
        loadgen.rope_append(qkv, cs, kc, vc, table, ctx, qs, q_out=torch.zeros(5, 128, 4, dtype=torch.bfloat16).transpose(1, 2))
    with pytest.raises(ValueError, match="16-byte"):
        loadgen.rope_append(qkv, cs, kc, vc, table, ctx, qs, q_out=torch.zeros(5 * W4 + 8, dtype=torch.bfloat16)[4:4 + 5 * W4].view(5, 4, 128))
    with pytest.raises(ValueError, match="bad output"):
        loadgen.rope_append(qkv, cs, kc, vc, table, ctx, qs, q_out=torch.zeros(5, 8, 128, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="bad output"):
        loadgen.rope_append(qkv, cs, kc, vc, table, ctx, qs, q_out=torch.zeros(5, 4, 128))
    # q_out inside qkv's storage range: in place on the q heads, and in the gap a padded token stride leaves
    with pytest.raises(ValueError, match="q_out overlaps qkv"):
        loadgen.rope_append(qkv, cs, kc, vc, table, ctx, qs, q_out=qkv[:, :4])
    big = torch.zeros(5, 16, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="q_out overlaps qkv"):
        loadgen.rope_append(big[:, :8], cs, kc, vc, table, ctx, qs, q_out=big[:, 8:12])
    both = torch.zeros(2, 5, 8, 128, dtype=torch.bfloat16)           # neighbours in one allocation do not overlap
    assert loadgen.rope_append(both[0], cs, kc, vc, table, ctx, qs, q_out=both[1, :, :4], max_q_len=0).data_ptr() == both[1].data_ptr()


def test_wrapper_rejects_q_start_mismatched_shapes_and_max_q_len(host_operands_pass):
    qkv, cs, kc, vc, table, ctx, qs = _operands()
    with pytest.raises(ValueError, match="q_start must be 1-D"):
        loadgen.rope_append(qkv, cs, kc, vc, table, ctx, qs[None, :])
    with pytest.raises(ValueError, match="q_start must be 1-D"):
        loadgen.rope_append(qkv, cs, kc, vc, table, ctx, qs[:0])
    with pytest.raises(ValueError, match="contiguous q_start"):
        loadgen.rope_append(qkv, cs, kc, vc, table, ctx, torch.zeros(6, dtype=torch.int32)[::2])
    with pytest.raises(ValueError, match="do not match the 3 sequences of q_start"):
        loadgen.rope_append(qkv, cs, kc, vc, table, ctx, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="do not match"):
        loadgen.rope_append(qkv, cs, kc, vc, table[:1], ctx, qs)
    with pytest.raises(ValueError, match="do not match"):
        loadgen.rope_append(qkv, cs, kc, vc, table, torch.ones(3, dtype=torch.int32), qs)
    with pytest.raises(ValueError, match="check=False needs max_q_len"):
        loadgen.rope_append(qkv, cs, kc, vc, table, ctx, qs, check=False)
    for bad in (-1, 2 ** 31):
        with pytest.raises(ValueError, match="max_q_len"):
            loadgen.rope_append(qkv, cs, kc, vc, table, ctx, qs, max_q_len=bad)


def test_no_sequences_no_tokens_and_no_chunk_launch_nothing(host_operands_pass):
    qkv, cs, kc, vc, table, ctx, qs = _operands()
    assert loadgen.rope_append(qkv, cs, kc, vc, table[:0], ctx[:0], qs[:1]).shape == (5, 4, 128)                  # S == 0
    assert loadgen.rope_append(qkv[:0], cs, kc, vc, table, ctx, torch.zeros(3, dtype=torch.int32)).shape == (0, 4, 128)
    given = torch.ones(5, 4, 128, dtype=torch.bfloat16)
    assert loadgen.rope_append(qkv, cs, kc, vc, table, ctx, qs, max_q_len=0, q_out=given, check=False) is given
    assert bool((given == 1).all())


def test_the_existing_attention_checks_are_unchanged(host_operands_pass):
    """rope_append reuses _paged_attn_operands: its texts for the attentions stay."""
    q = torch.zeros(5, 4, 128, dtype=torch.bfloat16)
    _, _, kc, vc, table, ctx, qs = _operands()
    with pytest.raises(ValueError, match=r"paged_prefill_attention expects q \[Tq, Hq, 128\], k_cache \[NB, Hkv, 32, 128\]"):
        loadgen.paged_prefill_attention(q[0], kc, vc, table, ctx, qs)
    with pytest.raises(ValueError, match=r"paged_decode_attention: Hq / Hkv = 5 / 2 must be one of \(1, 2, 4, 8, 16\)"):
        loadgen.paged_decode_attention(torch.zeros(2, 5, 128, dtype=torch.bfloat16), kc, vc, table, ctx)


# ------------------------------------------------------------------------------------------------
# executor
# ------------------------------------------------------------------------------------------------
def test_enqueue_ops_dispatches_rope_append_without_the_check(monkeypatch):
    from k8s_gpu_scheduler_amd.parallel import executor
    calls = []
    monkeypatch.setattr(loadgen, "rope_append", lambda *a, **k: calls.append((a, k)))

    class Stub:
        ops = [(W.Op("rope_append", 1, 1, 64, rows=1, q=40), ("q_out", "qkv", "cos_sin", "kc", "vc", "table", "ctx", "q_start"))]

    executor.enqueue_ops(Stub(), 2, "stream", 0)
    assert calls == [(("qkv", "cos_sin", "kc", "vc", "table", "ctx", "q_start"),
                      {"max_q_len": 40, "q_out": "q_out", "stream": "stream", "check": False})] * 2
    assert executor.op_output(*Stub.ops[0]) == "q_out"
    assert executor.OP_KINDS["rope_append"][2] == 0


def test_buffers_build_rope_append_operands_reproducibly():
    from k8s_gpu_scheduler_amd.parallel.executor import _Buffers
    o = W.Op("rope_append", 3, 4, 96, rows=2, q=40)
    w = W.Workload("t_rope_append", "test", "hip", 3, (o,), 0.0)
    cpu = torch.device("cpu")
    a, b = _Buffers(w, cpu), _Buffers(w, cpu)
    q_out, qkv, cs, kc, vc, table, ctx, q_start = a.ops[0][1]
    assert qkv.shape == (120, 8, 128) and q_out.shape == (120, 4, 128) and qkv.dtype == q_out.dtype == torch.bfloat16
    assert torch.equal(cs, loadgen.rope_table(96))
    assert kc.shape == (9, 2, 32, 128) and vc.shape == (9, 2, 128, 32) and kc.dtype == vc.dtype == torch.bfloat16
    assert table.shape == (3, 3) and table.dtype == torch.int32 and sorted(table.flatten().tolist()) == list(range(9))
    assert ctx.tolist() == [96, 96, 96] and q_start.tolist() == [0, 40, 80, 120] and q_start.dtype == torch.int32
    assert torch.equal(qkv.view(torch.int16), b.ops[0][1][1].view(torch.int16)) and torch.equal(table, b.ops[0][1][5])
    for bad, msg in ((W.Op("rope_append", 3, 4, 100, rows=2, q=40), "workload t_bad: attention context 100 is no multiple of 32"),
                     (W.Op("rope_append", 3, 4, 96, rows=2, q=97), "workload t_bad: append chunk 97 is longer than the context 96")):
        with pytest.raises(ValueError, match=msg):
            _Buffers(W.Workload("t_bad", "test", "hip", 3, (bad,), 0.0), cpu)


# ------------------------------------------------------------------------------------------------
# the GPU tests' reference
# ------------------------------------------------------------------------------------------------
def test_reference_agrees_with_the_direct_formula():
    from test_gpu_rope_append_exact import expected_caches, quarter_table, reference
    g = torch.Generator().manual_seed(3)
    Hq, Hkv, lead = 4, 2, 2
    seqs = [(5, 2), (40, 40), (33, 0), (70, 3)]                                               # (ctx, q_len)
    Tq = lead + sum(n for _, n in seqs) + 1
    qkv = torch.randn(Tq, Hq + 2 * Hkv, 128, generator=g, dtype=torch.float64)
    cs = torch.randn(70, 128, generator=g, dtype=torch.float64)
    ctx = torch.tensor([c for c, _ in seqs], dtype=torch.int32)
    q_start = torch.tensor([lead] + [n for _, n in seqs]).cumsum(0).to(torch.int32)
    ref_q, ref_k, pos, seq = reference(qkv, cs, ctx, q_start, Hkv)
    assert ref_q.shape == (Tq, Hq, 128) and ref_k.shape == (Tq, Hkv, 128) and ref_q.dtype == ref_k.dtype == torch.float64
    assert not ref_q[:lead].any() and not ref_q[-1].any() and pos[:lead].tolist() == [-1] * lead and int(pos[-1]) == -1
    for s, (c, n) in enumerate(seqs):
        for j in range(n):
            row, p = int(q_start[s]) + j, c - n + j
            assert (int(pos[row]), int(seq[row])) == (p, s)
            for h in range(Hq + Hkv):
                got = ref_q[row, h] if h < Hq else ref_k[row, h - Hq]
                for i in (0, 1, 31, 63):
                    x1, x2, co, si = (float(v) for v in (qkv[row, h, i], qkv[row, h, i + 64], cs[p, i], cs[p, 64 + i]))
                    assert float(got[i]) == x1 * co - x2 * si and float(got[i + 64]) == x2 * co + x1 * si
    # the cache expectation, slot by slot
    table = torch.tensor([[7, -1, -1], [3, 0, -1], [-1, -1, -1], [5, 2, 6]], dtype=torch.int32)
    kb = torch.randint(-9, 9, (Tq, Hkv, 128), generator=g).to(torch.int16)
    vb = torch.randint(-9, 9, (Tq, Hkv, 128), generator=g).to(torch.int16)
    kc, vc, blk, slot = expected_caches(9, Hkv, kb, vb, pos, seq, table)
    assert kc.shape == (9, Hkv, 32, 128) and vc.shape == (9, Hkv, 128, 32)
    seen = set()
    for row in range(Tq):
        if int(pos[row]) < 0:
            continue
        b, sl = int(table[int(seq[row]), int(pos[row]) // 32]), int(pos[row]) % 32
        seen.add((b, sl))
        assert torch.equal(kc[b, :, sl, :], kb[row]) and torch.equal(vc[b, :, :, sl], vb[row])
    assert len(seen) == 45 and int((kc != 0x5A5A).sum()) <= 45 * Hkv * 128
    assert all(bool((kc[b, :, sl] == 0x5A5A).all()) for b in range(9) for sl in range(32) if (b, sl) not in seen)
    qt = quarter_table(6)
    assert qt[0, :4].tolist() == [1, 0, -1, 0] and qt[0, 64:68].tolist() == [0, 1, 0, -1] and qt[1, :3].tolist() == [0, -1, 0]
