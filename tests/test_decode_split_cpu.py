"""The split-KV paged decode attention without a GPU: the workload model's attn_split op and the
llm_decode_long_8 workload, the pure-Python grid, workspace and partition rules, the host wrapper's
validation of kv_splits and the workspace (which must fire before the native module is touched),
the profiler's kernel classification, the executor's op dispatch, and what the context lengths and
the target placement of test_gpu_decode_split_exact.py cover.  The kernels themselves are pinned on
the GPU by that module."""
import os

import pytest
import torch

import test_gpu_decode_split_exact as G
from k8s_gpu_scheduler_amd import _native
from k8s_gpu_scheduler_amd.models import workloads as W
from k8s_gpu_scheduler_amd.ops import loadgen
from k8s_gpu_scheduler_amd.parallel import executor


# ------------------------------------------------------------------------------------------------
# workload model
# ------------------------------------------------------------------------------------------------
def test_attn_split_op_flops_bytes_workgroups():
    o = W.Op("attn_split", M=3, N=8, K=64, rows=2, splits=4)
    a = W.Op("attn", M=3, N=8, K=64, rows=2)
    assert not o.is_gemm and not o.on_mfma and o.mfma_rate() == 1.0
    assert o.flops == a.flops == 4 * 3 * 8 * 64 * 128
    assert W.ATTN_PARTIAL_FLOATS == 132 and W.ATTN_MAX_KV_SPLITS == loadgen.ATTN_MAX_KV_SPLITS == 32
    assert W.decode_split_workspace_floats(3, 8, 4) == 3 * 8 * 4 * 132
    assert o.bytes == a.bytes + 2 * 4 * 3 * 8 * 4 * 132                     # the workspace written and read once
    assert o.workgroups(0) == o.workgroups(64) == W.default_attn_split_workgroups(3, 2, 4) == 3 * 2 * 4
    assert loadgen.decode_split_workspace_floats is W.decode_split_workspace_floats


def test_op_keeps_its_positional_fields_and_splits_defaults_to_zero():
    assert W.Op("gemm", 64, 64, 64).splits == 0
    o = W.Op("prefill", 2, 32, 4096, True, 0, 8, 1024)
    assert (o.M, o.N, o.K, o.relu, o.n_floats, o.rows, o.q, o.splits) == (2, 32, 4096, True, 0, 8, 1024, 0)
    assert W.Op("attn_split", 1, 1, 32, True, 0, 1, 0, 5).splits == 5       # the last field


def test_attn_split_cu_fill_counts_the_split_workgroups():
    def lone(splits):
        return W.Workload("a", "llm_decode_long", "hip", 8, (W.Op("attn_split", 8, 32, 32768, rows=8, splits=splits),), 0.0)
    assert W.cu_fill(lone(4)) == 256 / 256
    assert W.cu_fill(lone(2)) == 128 / 256
    assert W.cu_fill(W.Workload("a", "x", "hip", 8, (W.Op("attn", 8, 32, 32768, rows=8),), 0.0)) == 64 / 256


def test_llm_decode_long_workload():
    w = W.get("llm_decode_long_8")
    assert W.workload_for_pod("llm-decode-long-8-x") is w and W.LONG_CONTEXT == {"llm_decode_long_8": w}
    assert (w.family, w.framework, w.batch, w.hbm_gib) == ("llm_decode_long", "hip", 8, 1.25)
    qkv, a, proj = w.ops
    assert a.kind == "attn_split" and (a.M, a.N, a.K, a.rows) == (8, 32, 32768, 8)
    assert 2 <= a.splits <= W.ATTN_MAX_KV_SPLITS
    assert 2 * a.M * a.K * a.rows * W.ATTN_HEAD_DIM * 2 == 1 << 30 and w.hbm_gib * (1 << 30) >= 1 << 30
    assert a.M * (a.K // W.ATTN_BLOCK_TOKENS) == 8 * 1024
    assert qkv == W.Op("gemm", 64, 6144, 4096) and proj == W.Op("gemm", 64, 4096, 4096)
    assert qkv.N == (a.N + 2 * a.rows) * W.ATTN_HEAD_DIM and proj.K == a.N * W.ATTN_HEAD_DIM
    assert a.M <= qkv.M == proj.M == loadgen.BM                           # the 8 tokens ride in the minimum tile
    m, h = W.roofline_split("llm-decode-long-8-x", tflops=1.0e3, tbps=6.0)
    assert h == pytest.approx(a.bytes / 6.0e12) and m == pytest.approx((qkv.flops + proj.flops) / 1.0e15) and h > m
    assert 0.0 < W.cu_fill(w) <= 1.0


def test_the_pinned_tables_are_unchanged():
    assert len(W.CATALOG) == 18
    assert set(W.EXTRA) == {"fp8_llm_2048", "triad_only_2048", "dlrm_2048", "llm_decode_256"}
    assert set(W.STAGED) == {"llm_prefill_2048"}
    for table in (W.CATALOG, W.EXTRA, W.STAGED):
        assert "llm_decode_long_8" not in table
        assert all(o.kind != "attn_split" and o.splits == 0 for w in table.values() for o in w.ops)
    assert W.get("llm_decode_256") is W.EXTRA["llm_decode_256"]
    assert W.get("llm_decode_256").ops == (W.Op("gemm", 256, 6144, 4096), W.Op("attn", 256, 32, 1024, rows=8),
                                           W.Op("gemm", 256, 4096, 4096))
    assert W.get("llm_prefill_2048") is W.STAGED["llm_prefill_2048"]
    assert W.get("llm_prefill_2048").ops == (W.Op("gemm", 2048, 6144, 4096), W.Op("prefill", 2, 32, 4096, rows=8, q=1024),
                                             W.Op("gemm", 2048, 4096, 4096))
    assert W.workload_for_pod("llm-decode-256-x") is W.EXTRA["llm_decode_256"]
    with pytest.raises(KeyError):
        W.get("llm_decode_long")


# ------------------------------------------------------------------------------------------------
# the Python rules against the native ones
# ------------------------------------------------------------------------------------------------
def test_partition_rule():
    assert [W.decode_split_range(257, 8, p) for p in range(8)] == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 9), (9, 9),
                                                                   (9, 9), (9, 9)]
    assert [W.decode_split_range(33, 2, p) for p in range(2)] == [(0, 1), (1, 2)]
    assert [W.decode_split_range(0, 3, p) for p in range(3)] == [(0, 0)] * 3
    assert [W.decode_split_range(32768, 16, p) for p in (0, 15)] == [(0, 64), (960, 1024)]
    for ctx in (0, 1, 31, 32, 33, 97, 257, 1025, 1153, 32768):
        for k in range(1, 33):
            assert loadgen.decode_split_range(ctx, k, 0) == W.decode_split_range(ctx, k, 0)
            rs = [W.decode_split_range(ctx, k, p) for p in range(k)]
            assert rs == [G.split_range(ctx, k, p) for p in range(k)]          # the GPU module's own copy
            # contiguous, in order, covering exactly the sequence's blocks
            assert rs[0][0] == 0 and rs[-1][1] == -(-ctx // 32)
            assert all(a[1] == b[0] for a, b in zip(rs, rs[1:])) and all(lo <= hi for lo, hi in rs)


@pytest.mark.skipif(_native.hip(required=False) is None, reason="HIP extension not built")
def test_python_rules_match_the_native_ones():
    h = _native.hip()
    for s in (0, 1, 7, 8, 256):
        for hkv in (1, 2, 8):
            for k in (2, 3, 16, 32):
                assert h.paged_decode_split_workgroups(s, hkv, k) == W.default_attn_split_workgroups(s, hkv, k)
                for group in (1, 4, 16):
                    assert (h.paged_decode_split_workspace_floats(s, group * hkv, k)
                            == W.decode_split_workspace_floats(s, group * hkv, k)), (s, hkv, k, group)


@pytest.mark.skipif(_native.hip(required=False) is None, reason="HIP extension not built")
def test_native_entry_point_throws_before_it_launches():
    """Pointers that pass the alignment checks but are never dereferenced: every call must throw."""
    h = _native.hip()
    ok = dict(q=4096, k_cache=4096, v_cache=4096, block_table=4096, ctx_lens=4096, workspace=4096, out=4096, S=2, Hq=4,
              Hkv=2, kv_splits=4, ld_q=512, ld_out=512, ld_table=4, scale=1.0, stream=0)
    for bad in (dict(kv_splits=1), dict(kv_splits=0), dict(kv_splits=33), dict(workspace=4100), dict(Hq=6),
                dict(ld_q=500), dict(out=4104), dict(S=1 << 27, Hkv=1, Hq=1, kv_splits=16)):
        with pytest.raises(RuntimeError):
            h.paged_decode_split_bf16(**dict(ok, **bad))
    h.paged_decode_split_bf16(**dict(ok, S=0))                               # no sequences: nothing is launched


# ------------------------------------------------------------------------------------------------
# host wrapper: every rejection happens before the native module is asked for
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def no_native(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the native module was touched")
    monkeypatch.setattr(_native, "hip", boom)


@pytest.fixture
def host_operands_pass(monkeypatch, no_native):
    """Without a GPU the device check is stubbed out, and everything after it up to the native call
    runs on host tensors."""
    monkeypatch.setattr(loadgen, "_check_devices", lambda name, *ts: torch.device("cpu"))


def _operands(S=2, Hq=4, Hkv=2, NB=3, MB=2):
    q = torch.zeros(S, Hq, 128, dtype=torch.bfloat16)
    kc = torch.zeros(NB, Hkv, 32, 128, dtype=torch.bfloat16)
    vc = torch.zeros(NB, Hkv, 128, 32, dtype=torch.bfloat16)
    return q, kc, vc, torch.zeros(S, MB, dtype=torch.int32), torch.ones(S, dtype=torch.int32)


def test_signature_ends_with_the_two_keywords():
    import inspect
    ps = list(inspect.signature(loadgen.paged_decode_attention).parameters.values())
    assert [p.name for p in ps] == ["q", "k_cache", "v_cache", "block_table", "ctx_lens", "out", "scale", "stream",
                                    "check", "kv_splits", "workspace"]
    assert ps[-2].default == 1 and ps[-1].default is None


@pytest.mark.parametrize("bad", [0, -1, 33, 64, 2.0, "4", None, True])
def test_wrapper_rejects_kv_splits(host_operands_pass, bad):
    with pytest.raises(ValueError, match="kv_splits"):
        loadgen.paged_decode_attention(*_operands(), kv_splits=bad)


def test_wrapper_rejects_workspaces(host_operands_pass):
    ops = _operands()
    need = W.decode_split_workspace_floats(2, 4, 4)
    with pytest.raises(TypeError, match="fp32 workspace"):
        loadgen.paged_decode_attention(*ops, kv_splits=4, workspace=torch.zeros(need, dtype=torch.float64))
    with pytest.raises(TypeError, match="fp32 workspace"):
        loadgen.paged_decode_attention(*ops, kv_splits=4, workspace=torch.zeros(need, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="contiguous"):
        loadgen.paged_decode_attention(*ops, kv_splits=4, workspace=torch.zeros(2 * need)[::2])
    with pytest.raises(ValueError, match="16-byte"):
        loadgen.paged_decode_attention(*ops, kv_splits=4, workspace=torch.zeros(need + 4)[1:1 + need])
    with pytest.raises(ValueError, match=f"need {need}"):
        loadgen.paged_decode_attention(*ops, kv_splits=4, workspace=torch.zeros(need - 1))
    with pytest.raises(ValueError, match="need"):                             # enough for 2 splits, not for 4
        loadgen.paged_decode_attention(*ops, kv_splits=4, workspace=torch.zeros(W.decode_split_workspace_floats(2, 4, 2)))
    with pytest.raises(ValueError, match="workspace on"):
        loadgen.paged_decode_attention(*ops, kv_splits=4, workspace=torch.zeros(need, device="meta"))
    # the operand checks of the unsplit op still come first
    with pytest.raises(ValueError, match="Hq / Hkv"):
        loadgen.paged_decode_attention(*_operands(Hq=6), kv_splits=4, workspace=torch.zeros(need))


def test_a_good_call_reaches_the_native_module(host_operands_pass):
    ops = _operands()
    for kw in (dict(kv_splits=4, workspace=torch.zeros(W.decode_split_workspace_floats(2, 4, 4))),
               dict(kv_splits=32, workspace=torch.zeros(W.decode_split_workspace_floats(2, 4, 32) + 4)),
               dict(kv_splits=2), dict(kv_splits=1)):
        with pytest.raises(AssertionError, match="native module was touched"):
            loadgen.paged_decode_attention(*ops, **kw)
    q, kc, vc, table, ctx = ops
    assert loadgen.paged_decode_attention(q[:0], kc, vc, table[:0], ctx[:0], kv_splits=4).shape == (0, 4, 128)


# ------------------------------------------------------------------------------------------------
# profiler and executor
# ------------------------------------------------------------------------------------------------
def test_the_new_kernels_are_not_mfma_kernels():
    from k8s_gpu_scheduler_amd.agent import pod_profiler
    names = ("paged_decode_split_kernel", "paged_decode_merge_kernel",
             "gs::(anonymous namespace)::paged_decode_split_kernel(__bf16 const*, __bf16 const*, __bf16 const*, "
             "int const*, int const*, float*, int, int, int, unsigned long, unsigned long, float)",
             "gs::(anonymous namespace)::paged_decode_merge_kernel(float const*, __bf16*, int, int, int, unsigned long)",
             "_ZN2gs12_GLOBAL__N_125paged_decode_split_kernelEPKDF16bS2_S2_PKiS4_Pfiiimmf",
             "_ZN2gs12_GLOBAL__N_125paged_decode_merge_kernelEPKfPDF16biiim")
    for name in names:
        assert not pod_profiler.is_mfma_kernel(name), name
        assert not any(m in name for m in pod_profiler.MFMA_KERNEL_MARKERS), name
    src = open(os.path.join(os.path.dirname(__file__), "..", "native", "hip", "decode_attn.hip")).read()
    assert "paged_decode_split_kernel(" in src and "paged_decode_merge_kernel(" in src and "paged_decode_kernel(" in src
    assert "asm" not in src.replace("#pragma", "")                           # no inline assembly


def test_enqueue_ops_makes_the_one_split_call(monkeypatch):
    calls = []
    monkeypatch.setattr(loadgen, "paged_decode_attention", lambda *a, **k: calls.append((a, k)))

    class Stub:
        ops = [(W.Op("attn_split", 1, 1, 64, rows=1, splits=2), ("out", "q", "kc", "vc", "table", "ctx", "ws"))]

    executor.enqueue_ops(Stub(), 2, "stream", 64, blocks=7)
    assert calls == [(("q", "kc", "vc", "table", "ctx"), {"out": "out", "stream": "stream", "check": False,
                                                           "kv_splits": 2, "workspace": "ws"})] * 2
    assert executor.op_output(Stub.ops[0][0], Stub.ops[0][1]) == "out"
    assert executor.OP_KINDS["attn_split"][2] == 0


def test_buffers_build_the_attn_split_operands_reproducibly():
    o = W.Op("attn_split", 3, 4, 160, rows=2, splits=3)
    w = W.Workload("pin_split", "pin", "hip", 3, (o, W.Op("gemm", 64, 64, 64)), 0.1)
    a, b = executor._Buffers(w, torch.device("cpu")), executor._Buffers(w, torch.device("cpu"))
    (oa, ta), (ob, tb) = a.ops[0], b.ops[0]
    assert oa == ob == o and len(ta) == 7
    out, q, kc, vc, table, ctx, ws = ta
    assert out.shape == q.shape == (3, 4, 128) and kc.shape == (15, 2, 32, 128) and vc.shape == (15, 2, 128, 32)
    assert table.shape == (3, 5) and sorted(table.flatten().tolist()) == list(range(15)) and ctx.tolist() == [160] * 3
    assert ws.dtype == torch.float32 and ws.shape == (W.decode_split_workspace_floats(3, 4, 3),) and ws.is_contiguous()
    for x, y in zip(ta[1:6], tb[1:6]):
        assert torch.equal(x.view(torch.int16) if x.dtype == torch.bfloat16 else x,
                           y.view(torch.int16) if y.dtype == torch.bfloat16 else y)
    # the same draws as an "attn" op of the same shape: the workspace takes nothing from the generator
    plain = executor._Buffers(W.Workload("pin_split", "pin", "hip", 3, (W.Op("attn", 3, 4, 160, rows=2),
                                                                        W.Op("gemm", 64, 64, 64)), 0.1), torch.device("cpu"))
    for x, y in zip(ta[1:6], plain.ops[0][1][1:6]):
        assert torch.equal(x.float(), y.float())
    assert torch.equal(a.ops[1][1][0].float(), plain.ops[1][1][0].float())
    with pytest.raises(ValueError, match=r"workload odd: attention context 48 is no multiple of 32"):
        executor._Buffers(W.Workload("odd", "pin", "hip", 1, (W.Op("attn_split", 1, 1, 48, rows=1, splits=2),), 0.1),
                          torch.device("cpu"))


# ------------------------------------------------------------------------------------------------
# what the GPU module's context lengths cover, by its copy of the partition rule
# ------------------------------------------------------------------------------------------------
def _sizes(ctx, k):
    return [hi - lo for lo, hi in (G.split_range(ctx, k, p) for p in range(k))]


@pytest.mark.parametrize("ctxs", [G.CTX_A, G.CTX_B])
@pytest.mark.parametrize("k", G.KV_SPLITS)
def test_the_context_lengths_cover_the_partition(ctxs, k):
    assert len(ctxs) == 8 and 0 in ctxs
    sizes = {c: _sizes(c, k) for c in ctxs}
    assert any(0 in sz for c, sz in sizes.items() if c > 0)                   # sequences with empty splits
    # a split whose only block is the sequence's partial last block
    assert any(sz[p] == 1 and G.split_range(c, k, p)[1] == -(-c // 32) and c % 32
               for c, sz in sizes.items() for p in range(k))
    assert any(0 < n < 4 for sz in sizes.values() for n in sz)                 # waves without a block
    assert any(sum(n > 0 for n in sz) >= 2 for sz in sizes.values())           # at least two non-empty splits
    if k != 16:
        assert any(n > 4 for sz in sizes.values() for n in sz)                 # a wave with two blocks
    else:
        assert max(n for sz in sizes.values() for n in sz) <= 4
    # a sequence where the rule gives split 0 two blocks or more AND has two non-empty splits (the
    # pair regime's one-split pairs need it)
    assert any(sz[0] >= 2 and sum(n > 0 for n in sz) >= 2 for sz in sizes.values())
    need = sorted(-(-c // 32) for c in ctxs)
    assert need[-1] != need[-2]                                                # block_tables requires it


def test_the_examples_of_single_partial_block_splits():
    assert _sizes(33, 2) == [1, 1] and _sizes(257, 8) == [2, 2, 2, 2, 1, 0, 0, 0]
    assert G.split_range(33, 2, 1) == (1, 2) and G.split_range(257, 8, 4) == (8, 9)


def test_uniform_and_short_context_lengths():
    assert all(c & (c - 1) == 0 and 0 < c <= 1024 for c in G.CTX_UNIFORM) and len(G.CTX_UNIFORM) == 8
    assert 8 * 1024 < 2 ** 24                                                 # sums of V in [-4, 4] are exact in fp32
    need = sorted(-(-c // 32) for c in G.CTX_SHORT)
    assert need[-1] == 4 and need[-1] != need[-2]
    need = sorted(-(-c // 32) for c in G.CTX_UNIFORM)
    assert need[-1] != need[-2]
    assert G.KV_SPLITS == (2, 3, 4, 8, 16) and G.SHAPES == ((1, 2), (2, 1), (4, 1), (8, 2), (16, 1))
    assert G.CTX_A == (0, 1, 33, 257, 320, 1025, 1121, 97) and G.CTX_B == (1153, 64, 0, 129, 31, 640, 2, 513)


# ------------------------------------------------------------------------------------------------
# the placement of the targets
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", G.KV_SPLITS + (32,))
@pytest.mark.parametrize("group,hkv", G.SHAPES)
def test_target_placement(group, hkv, k):
    """The properties the GPU module's docstring promises.  A group of a single head has a single
    one-hot target per KV head; the placement rotates the leading targets by the KV head, so the
    shape (1, 2) covers two of them per sequence over its two KV heads."""
    ctxs = (G.CTX_A if hkv == 1 else G.CTX_B) if k != 32 else G.CTX_SHORT
    g = torch.Generator().manual_seed(k * 100 + group)
    some_one_split_pair = False
    for ctx in ctxs:
        if ctx == 0:
            continue
        ne = G.nonempty_splits(ctx, k)
        bps = -(-(-(-ctx // 32)) // k)
        onehot_all = []
        for kv in range(hkv):
            one = G.place(ctx, group, k, g, rot=kv)
            two = G.place(ctx, group, k, g, rot=kv, pair=True)
            assert len(one) == len(two) == min(group, ctx) and all(len(t) == 1 for t in one)
            flat1, flat2 = [t for h in one for t in h], [t for h in two for t in h]
            assert len(set(flat1)) == len(flat1) and len(set(flat2)) == len(flat2)           # distinct tokens
            assert all(0 <= t < ctx for t in flat1 + flat2)
            onehot_all += flat1
            if ctx > 32:
                assert len(two[0]) == 2, (ctx, two)                    # later heads may find no free token (ctx 33)
            if len(ne) < 2:
                continue
            split = lambda t: G.split_of(t, ctx, k)                                           # noqa: E731
            # pairs: head 0's in two different splits; head 1's in one split, different waves
            assert split(two[0][0]) != split(two[0][1]), (ctx, two[0])
            if group >= 2 and ctx >= 2 and bps >= 2:
                t, u = two[1]
                assert split(t) == split(u) and t // 32 != u // 32, (ctx, k, two[1])
                assert G.wave_of(t, ctx, k) != G.wave_of(u, ctx, k)
                some_one_split_pair = True
            if group >= 2:
                first_of_later = {32 * G.split_range(ctx, k, p)[0] for p in ne[1:]}
                assert first_of_later & set(flat1) and ctx - 1 in flat1
                assert any(split(t) == ne[-1] for t in flat1)
        if len(ne) >= 2 and group == 1 and hkv == 2:
            first_of_later = {32 * G.split_range(ctx, k, p)[0] for p in ne[1:]}
            assert first_of_later & set(onehot_all) and ctx - 1 in onehot_all
            assert any(G.split_of(t, ctx, k) == ne[-1] for t in onehot_all)
    if group >= 2 and k != 32:
        assert some_one_split_pair


def test_placed_operands_put_each_heads_sign_row_on_its_targets_only():
    g = torch.Generator().manual_seed(3)
    q, ks, vs, targets = G.placed_operands("pair", 4, 2, G.CTX_B, 4, g)
    H = G.hadamard()
    for s, ctx in enumerate(G.CTX_B):
        for kv in range(2):
            scores = torch.einsum("cd,td->ct", q[s, kv * 4:(kv + 1) * 4], ks[s][kv]) * G.D ** -0.5
            for c in range(4):
                hot = (scores[c] > 300).nonzero().flatten().tolist()
                assert sorted(hot) == sorted(targets[s][kv][c]), (s, kv, c)
                assert bool((scores[c][[t for t in range(ctx) if t not in hot]] == 0).all())
    assert torch.equal(q[2], 8 * H[:8])                                       # ctx == 0: q is still set
