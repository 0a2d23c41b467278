"""The mixture-of-experts MLP without a GPU: the three op kinds of the workload model, the tile bound against a brute
force, the pure-torch layout reference's properties, the LLM_MOE table, the host wrappers' validation (which must fire
before the native module is touched), the executor's op dispatch and operands, and the pure-Python grid rules against
the native ones.  The kernels themselves are pinned on the GPU by test_gpu_moe_route_exact.py,
test_gpu_moe_gemm_exact.py, test_gpu_moe_combine_exact.py and test_gpu_moe_chain.py."""
import itertools

import pytest
import torch

from k8s_gpu_scheduler_amd import _native
from k8s_gpu_scheduler_amd.models import workloads as W
from k8s_gpu_scheduler_amd.ops import loadgen

BF = torch.bfloat16
I32 = torch.int32
OLD_TABLES = ("CATALOG", "EXTRA", "STAGED", "LONG_CONTEXT", "LLM_LAYER", "LLM_BLOCK", "LLM_HEAD")
MOE_KINDS = ("moe_route", "moe_gemm", "moe_combine")


# ------------------------------------------------------------------------------------------------
# workload model
# ------------------------------------------------------------------------------------------------
def test_the_constants():
    assert (W.MOE_BLOCK_M, W.MOE_MAX_EXPERTS, W.MOE_MAX_TOP_K, W.MOE_MAX_SLOTS) == (64, 256, 8, 32768)
    assert loadgen.MOE_BLOCK_M == 64 and loadgen.moe_max_tiles is W.moe_max_tiles


def test_op_flops_bytes_workgroups_small():
    r = W.Op("moe_route", 5, 8, 2)                                   # 10 slots, 8 experts: min(10, (10 + 504) // 64 = 8) tiles
    assert not r.is_gemm and not r.on_mfma and r.mfma_rate() == 1.0
    assert W.moe_max_tiles(5, 2, 8) == 8
    assert r.flops == 5 * 8 * 2 == 80
    assert r.bytes == 2 * 5 * 8 + 16 * 10 + 4 * 512 + 4 * 8 + 4 * 9 == 2356
    assert r.workgroups(0) == r.workgroups(64) == 2
    g = W.Op("moe_gemm", 5, 128, 64, rows=8, q=2, gather=True)
    assert g.on_mfma and not g.is_gemm and g.mfma_rate() == 1.0
    assert g.flops == 2 * 10 * 128 * 64 == 163840
    assert g.bytes == 2 * 8 * 128 * 64 + 2 * 10 * 64 + 2 * 10 * 128 == 134912        # min(E, T k) = 8 experts' weights
    assert g.workgroups(0) == g.workgroups(64) == 8 * 1                               # N = 128: one 128-wide column tile
    assert W.Op("moe_gemm", 5, 192, 64, rows=8, q=2).workgroups(0) == 8 * 3           # N = 192: 64-wide tiles
    few = W.Op("moe_gemm", 1, 64, 64, rows=8, q=2)                                    # 2 slots can hit 2 experts
    assert few.bytes == 2 * 2 * 64 * 64 + 2 * 2 * 64 + 2 * 2 * 64 and few.workgroups(0) == 2
    assert g.gather and not few.gather and W.Op("moe_gemm", 5, 128, 64, rows=8, q=2) != g
    c = W.Op("moe_combine", 5, 2056, 2, rows=8)
    assert not c.on_mfma
    assert c.flops == 2 * 5 * 2 * 2056 == 41120
    assert c.bytes == 2 * 10 * 2056 + 2 * 5 * 2056 + 8 * 10 == 61760
    assert c.workgroups(0) == c.workgroups(64) == -(-5 * 257 // 256) == 6
    for o in (W.Op("moe_route", 0, 8, 2), W.Op("moe_gemm", 0, 128, 64, rows=8, q=2), W.Op("moe_combine", 0, 64, 2, rows=8)):
        assert o.flops == 0 and o.workgroups(0) == 0
    assert W.Op("gemm", 64, 64, 64).gather is False                                   # the new field is defaulted, last
    assert W.Op("gemm", 64, 64, 64) == W.Op("gemm", 64, 64, 64, True, 0, 0, 0, 0, False)


def test_op_flops_bytes_workgroups_at_the_workload_shapes():
    assert W.moe_max_tiles(256, 8, 128) == 158 and W.moe_max_tiles(2048, 8, 128) == 382
    up = W.Op("moe_gemm", 256, 1536, 2048, rows=128, q=8, gather=True)
    down = W.Op("moe_gemm", 256, 2048, 768, rows=128, q=8)
    assert up.flops == 2 * 2048 * 1536 * 2048 == 12884901888 and down.flops == 2 * 2048 * 2048 * 768 == 6442450944
    assert up.bytes == 2 * 128 * 1536 * 2048 + 2 * 2048 * 2048 + 2 * 2048 * 1536 == 819986432
    assert down.bytes == 2 * 128 * 2048 * 768 + 2 * 2048 * 768 + 2 * 2048 * 2048 == 414187520
    assert 2 * 128 * (1536 * 2048 + 2048 * 768) == 1207959552                         # "about 1.2 GB" of expert weights
    assert up.workgroups(64) == 158 * 12 and down.workgroups(64) == 158 * 16
    assert W.Op("moe_route", 256, 128, 8).workgroups(64) == 64 and W.Op("moe_route", 2048, 128, 8).workgroups(64) == 512
    assert W.Op("moe_combine", 256, 2048, 8, rows=128).workgroups(64) == 256
    assert W.Op("moe_combine", 2048, 2048, 8, rows=128).workgroups(64) == 2048
    big = W.Op("moe_gemm", 2048, 1536, 2048, rows=128, q=8, gather=True)
    assert big.workgroups(64) == 382 * 12 and big.flops == 8 * up.flops
    assert big.bytes - up.bytes == 2 * 7 * 2048 * (2048 + 1536)                       # the same weights, eight times the rows


def brute_force_max_tiles(n, E):
    """max over all count vectors c >= 0 with sum c = n of sum ceil(c_e / 64), by enumeration of the multisets."""
    best = 0
    for cuts in itertools.combinations_with_replacement(range(n + 1), E - 1):
        edges = (0,) + cuts + (n,)
        best = max(best, sum(-(-(b - a) // 64) for a, b in zip(edges, edges[1:])))
    return best


@pytest.mark.parametrize("E", (1, 2, 3))
def test_moe_max_tiles_is_the_least_upper_bound(E):
    top = {1: 400, 2: 330, 3: 200}[E]
    for n in list(range(0, 12)) + list(range(60, 70)) + list(range(124, 132)) + [190, 191, 192, 193, top]:
        assert W.moe_max_tiles(n, 1, E) == brute_force_max_tiles(n, E), (n, E)
    for T, k in ((3, 2), (32, 4), (33, 4), (25, 8)):
        assert W.moe_max_tiles(T, k, E) == W.moe_max_tiles(T * k, 1, E)


def test_moe_max_tiles_literals():
    assert [W.moe_max_tiles(T, 8, 128) for T in (0, 1, 8, 256, 2048, 4096)] == [0, 8, 64, 158, 382, 638]
    assert W.moe_max_tiles(4096, 8, 256) == (32768 + 63 * 256) // 64 == 764
    assert W.moe_max_tiles(3, 1, 256) == 3 and W.moe_max_tiles(200, 8, 8) == (1600 + 504) // 64 == 32


# ------------------------------------------------------------------------------------------------
# the layout reference
# ------------------------------------------------------------------------------------------------
def check_layout(ids, E, sorted_ids, tile_expert, off, slot_pos):
    """The defining properties of the layout, for any arrays (the GPU tests call this on the kernel's too)."""
    T, k = ids.shape
    n, tiles = T * k, W.moe_max_tiles(T, k, E)
    flat = ids.reshape(-1).long()
    assert sorted_ids.shape == (64 * tiles,) and tile_expert.shape == (tiles,) and off.shape == (E + 1,) and slot_pos.shape == (n,)
    assert all(t.dtype == I32 for t in (sorted_ids, tile_expert, off, slot_pos))
    counts = torch.bincount(flat, minlength=E)
    assert off[0] == 0 and torch.equal((off[1:] - off[:-1]).long(), (counts + 63) // 64 * 64)
    assert int(off[E]) <= 64 * tiles
    for e in range(E):
        rows = sorted_ids[int(off[e]):int(off[e + 1])].long()
        mine = rows[:int(counts[e])]
        assert torch.equal(mine, (flat == e).nonzero().flatten()), e                 # all of e's slots, ascending: stable
        assert bool((rows[int(counts[e]):] == n).all()), e                            # the sentinel fills its last tile
        assert bool((tile_expert[int(off[e]) // 64:int(off[e + 1]) // 64] == e).all()), e
    assert bool((sorted_ids[int(off[E]):] == n).all()) and bool((tile_expert[int(off[E]) // 64:] == -1).all())
    real = sorted_ids[sorted_ids < n].long()
    assert torch.equal(real.sort().values, torch.arange(n))                           # every slot exactly once
    assert torch.equal(sorted_ids[slot_pos.long()].long(), torch.arange(n))           # slot_pos is the inverse map
    assert bool((tile_expert[sorted_ids.view(tiles, 64)[:, 0] < n] >= 0).all())       # a used tile starts with a real row


@pytest.mark.parametrize("T,k,E", [(1, 1, 8), (3, 2, 8), (64, 1, 8), (65, 2, 16), (200, 8, 128), (70, 8, 256), (4096, 8, 64)])
def test_align_reference_properties(T, k, E):
    g = torch.Generator().manual_seed(T * 1000 + k * 10 + E)
    ids = torch.rand(T, E, generator=g).argsort(dim=1)[:, :k].to(I32)               # k distinct experts per token
    out = loadgen.moe_align_reference(ids, E)
    check_layout(ids, E, *out)
    again = loadgen.moe_align_reference(ids.clone(), E)
    assert all(torch.equal(a, b) for a, b in zip(out, again))


def test_align_reference_edge_counts():
    # experts with 0, 1, 63, 64 and 65 slots, then everything to one expert with c = 64 and 65
    counts = [0, 1, 63, 64, 65, 0, 0, 0]
    ids = torch.cat([torch.full((c,), e) for e, c in enumerate(counts)])
    ids = ids[torch.randperm(len(ids), generator=torch.Generator().manual_seed(3))].view(-1, 1).to(I32)
    s, t, off, p = loadgen.moe_align_reference(ids, 8)
    check_layout(ids, 8, s, t, off, p)
    assert off.tolist() == [0, 0, 64, 128, 192, 320, 320, 320, 320] and t.tolist()[:6] == [1, 2, 3, 4, 4, -1]
    for c in (64, 65):
        one = torch.full((c, 1), 5, dtype=I32)
        s, t, off, p = loadgen.moe_align_reference(one, 8)
        check_layout(one, 8, s, t, off, p)
        assert int(off[8]) == 64 * -(-c // 64) and p.tolist() == list(range(c))
    empty = loadgen.moe_align_reference(torch.zeros(0, 2, dtype=I32), 8)
    assert [x.numel() for x in empty] == [0, 0, 9, 0] and empty[2].tolist() == [0] * 9
    with pytest.raises(ValueError, match="outside"):
        loadgen.moe_align_reference(torch.tensor([[8]]), 8)
    with pytest.raises(ValueError, match=r"\[T, k\]"):
        loadgen.moe_align_reference(torch.tensor([1, 2]), 8)


def test_topk_reference_ranks_by_value_then_index():
    row = torch.tensor([[0.5, 3.0, -1.0, 3.0, 2.0, -0.0, 0.0, 1.0]]).to(BF)
    ids, w = loadgen.moe_topk_reference(row, 8)
    assert ids.tolist() == [[1, 3, 4, 7, 0, 5, 6, 2]] and ids.dtype == I32 and w.dtype == torch.float32
    assert abs(w.sum().item() - 1) < 1e-6 and w[0, 0] == w[0, 1] > w[0, 2]
    ids, w = loadgen.moe_topk_reference(torch.zeros(2, 16, dtype=BF), 4)
    assert ids.tolist() == [[0, 1, 2, 3]] * 2 and w.tolist() == [[0.25] * 4] * 2
    inf = torch.tensor([[1.0, float("-inf"), float("inf"), 0.0, 0, 0, 0, 0]]).to(BF)
    assert loadgen.moe_topk_reference(inf, 8)[0].tolist() == [[2, 0, 3, 4, 5, 6, 7, 1]]


# ------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------
def operand_bytes(o):
    """Bytes of the operands parallel.executor allocates for one op, from its shapes."""
    if o.kind == "gemm":
        return 2 * (o.M * o.K + o.N * o.K + o.M * o.N) + 4 * o.N
    if o.kind == "add_rmsnorm":
        return 2 * (4 * o.M * o.N + o.N)
    if o.kind == "swiglu":
        return 6 * o.M * o.N
    if o.kind == "moe_route":
        tiles = W.moe_max_tiles(o.M, o.K, o.N)
        return 2 * o.M * o.N + 3 * 4 * o.M * o.K + 4 * 64 * tiles + 4 * tiles + 4 * (o.N + 1)
    if o.kind == "moe_gemm":
        tiles = W.moe_max_tiles(o.M, o.q, o.rows)
        return 2 * 64 * tiles * o.N + 2 * (o.M if o.gather else 64 * tiles) * o.K + 2 * o.rows * o.N * o.K + 4 * 65 * tiles
    if o.kind == "moe_combine":
        tiles = W.moe_max_tiles(o.M, o.K, o.rows)
        return 2 * o.M * o.N + 2 * 64 * tiles * o.N + 8 * o.M * o.K
    raise AssertionError(o.kind)


def test_llm_moe_workloads_and_their_table():
    dec, pre = W.get("llm_moe_decode_256"), W.get("llm_moe_prefill_2048")
    assert W.LLM_MOE == {"llm_moe_decode_256": dec, "llm_moe_prefill_2048": pre}
    for w, T, tiles in ((dec, 256, 158), (pre, 2048, 382)):
        assert w.ops == (W.Op("add_rmsnorm", T, 2048), W.Op("gemm", T, 128, 2048, relu=False), W.Op("moe_route", T, 128, 8),
                         W.Op("moe_gemm", T, 1536, 2048, rows=128, q=8, gather=True), W.Op("swiglu", 64 * tiles, 768),
                         W.Op("moe_gemm", T, 2048, 768, rows=128, q=8), W.Op("moe_combine", T, 2048, 8, rows=128))
        assert w.batch == T and w.framework == "hip"
        need = sum(operand_bytes(o) for o in w.ops)
        assert w.hbm_gib * 2 ** 30 >= need > (w.hbm_gib - 0.25) * 2 ** 30, (w.name, need / 2 ** 30)
        assert 0.0 < W.cu_fill(w) <= 1.0
        m, h = W.roofline_split(w.name.replace("_", "-") + "-0")
        assert m > 0 and h > 0
    assert 64 * 158 == 10112 and 64 * 382 == 24448
    assert (dec.family, dec.hbm_gib, pre.family, pre.hbm_gib) == ("llm_moe_decode", 1.5, "llm_moe_prefill", 1.75)
    assert [o.workgroups(64) for o in dec.ops] == [256, 8, 64, 1896, 948, 2528, 256]
    assert [o.workgroups(64) for o in pre.ops] == [2048, 64, 512, 4584, 2292, 6112, 2048]
    # at decode the expert GEMMs are bound by their weights: the bytes term of the roofline is the larger one
    for o in dec.ops:
        if o.kind == "moe_gemm":
            assert o.bytes / 5.5e12 > o.flops / 1100e12
    assert sum(o.bytes for o in dec.ops if o.kind == "moe_gemm") > 0.9 * dec.bytes


def test_the_older_tables_are_unchanged():
    assert len(W.CATALOG) == 18 and set(W.EXTRA) == {"fp8_llm_2048", "triad_only_2048", "dlrm_2048", "llm_decode_256"}
    assert set(W.STAGED) == {"llm_prefill_2048"} and set(W.LONG_CONTEXT) == {"llm_decode_long_8"}
    assert set(W.LLM_LAYER) == {"llm_layer_decode_256", "llm_layer_prefill_2048"}
    assert set(W.LLM_BLOCK) == {"llm_block_decode_256", "llm_block_prefill_2048"}
    assert set(W.LLM_HEAD) == {"llm_head_decode_256", "llm_head_decode_8"}
    assert W.LLM_HEAD["llm_head_decode_8"].ops[2] == W.Op("sample", 8, 128256, 50) and W.LLM_HEAD["llm_head_decode_256"].hbm_gib == 1.25
    for name in OLD_TABLES:
        assert all(o.kind not in MOE_KINDS and o.gather is False for w in getattr(W, name).values() for o in w.ops), name


def test_get_and_workload_for_pod():
    dec, pre = W.LLM_MOE["llm_moe_decode_256"], W.LLM_MOE["llm_moe_prefill_2048"]
    assert W.get("llm_moe_decode_256") is dec and W.get("llm_moe_prefill_2048") is pre
    assert W.workload_for_pod("llm-moe-decode-256-x") is dec and W.workload_for_pod("pod-llm-moe-prefill-2048-7") is pre
    assert W.workload_for_pod("llm-head-decode-256-x") is W.LLM_HEAD["llm_head_decode_256"]
    # a pod name that holds an old and a new name: the older tables are consulted first
    assert W.workload_for_pod("llm-moe-decode-256-and-llm-head-decode-256") is W.LLM_HEAD["llm_head_decode_256"]
    assert W.workload_for_pod("llm-moe-prefill-2048-and-llm-prefill-2048") is W.STAGED["llm_prefill_2048"]
    names = [n for t in OLD_TABLES for n in getattr(W, t)]
    for new in W.LLM_MOE:
        assert not any(old in new or new in old for old in names), new
    assert not any(a != b and a in b for a in W.LLM_MOE for b in W.LLM_MOE)
    for bad in ("llm_moe", "llm_moe_decode", "llm-moe-decode-256", "llm_moe_decode_255", "llm_moe_prefill_"):
        with pytest.raises(KeyError):
            W.get(bad)
    for bad in ("llm-moe-decode-255", "llm-moe-decode", "llm-moe-prefill-204"):
        with pytest.raises(KeyError):
            W.workload_for_pod(bad)


# ------------------------------------------------------------------------------------------------
# host wrappers: every rejection happens before the native module is asked for
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def no_native(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the native module was touched")
    monkeypatch.setattr(_native, "hip", boom)


@pytest.fixture
def host_operands_pass(monkeypatch, no_native):
    """The checks after the device check run on host tensors once it is stubbed out."""
    monkeypatch.setattr(loadgen, "_check_devices", lambda name, *ts: torch.device("cpu"))


TOUCHED = "native module was touched"


def test_wrappers_reject_cpu_tensors(no_native):
    lg = torch.zeros(3, 16, dtype=BF)
    with pytest.raises(ValueError, match="device tensors"):
        loadgen.moe_route(lg, 2)
    with pytest.raises(ValueError, match="device tensors"):          # before any dtype complaint
        loadgen.moe_route(lg.float(), 2)
    s, t, _, p = loadgen.moe_align_reference(torch.zeros(3, 2, dtype=I32), 8)
    with pytest.raises(ValueError, match="device tensors"):
        loadgen.moe_gemm(torch.zeros(3, 64, dtype=BF), torch.zeros(8, 64, 64, dtype=BF), s, t, 6, gather_div=2)
    with pytest.raises(ValueError, match="device tensors"):
        loadgen.moe_combine(torch.zeros(s.numel(), 8, dtype=BF), p, torch.ones(3, 2))
    with pytest.raises(ValueError, match="device tensors"):
        loadgen.moe_mlp(torch.zeros(3, 64, dtype=BF), lg, torch.zeros(16, 128, 64, dtype=BF), torch.zeros(16, 64, 64, dtype=BF), 2)


def test_moe_route_rejections(host_operands_pass):
    lg = torch.zeros(3, 16, dtype=BF)
    with pytest.raises(TypeError, match="bf16 logits"):
        loadgen.moe_route(lg.float(), 2)
    with pytest.raises(ValueError, match="logits must be 2-D"):
        loadgen.moe_route(lg[0], 2)
    with pytest.raises(ValueError, match="logits row stride 20"):
        loadgen.moe_route(torch.zeros(3, 20, dtype=BF)[:, :16], 2)
    with pytest.raises(ValueError, match="contiguous rows"):
        loadgen.moe_route(torch.zeros(3, 32, dtype=BF)[:, ::2], 2)
    with pytest.raises(ValueError, match="16-byte aligned"):
        loadgen.moe_route(torch.zeros(3 * 16 + 8, dtype=BF)[4:52].view(3, 16), 2)
    for E in (0, 4, 12, 264, 512):
        with pytest.raises(ValueError, match=r"multiple of 8 in \[8, 256\]"):
            loadgen.moe_route(torch.zeros(2, E, dtype=BF), 1)
    for k in (0, 9, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="top_k"):
            loadgen.moe_route(lg, k)
    with pytest.raises(ValueError, match="top_k"):                   # top_k <= E
        loadgen.moe_route(torch.zeros(2, 8, dtype=BF)[:, :8], 9)
    with pytest.raises(ValueError, match="more than 32768 slots"):
        loadgen.moe_route(torch.zeros(4097, 8, dtype=BF), 8)
    with pytest.raises(AssertionError, match=TOUCHED):               # 32768 slots exactly are legal
        loadgen.moe_route(torch.zeros(4096, 8, dtype=BF), 8)
    tiles = W.moe_max_tiles(3, 2, 16)
    good = dict(topk_ids=torch.zeros(3, 2, dtype=I32), topk_w=torch.zeros(3, 2), sorted_ids=torch.zeros(64 * tiles, dtype=I32),
                tile_expert=torch.zeros(tiles, dtype=I32), expert_offsets=torch.zeros(17, dtype=I32),
                slot_pos=torch.zeros(6, dtype=I32))
    with pytest.raises(AssertionError, match=TOUCHED):               # every check passed
        loadgen.moe_route(lg, 2, **good)
    with pytest.raises(AssertionError, match=TOUCHED):
        loadgen.moe_route(lg, 2, check=False)
    for nm, t in good.items():
        wrong_type = t.float() if t.dtype == I32 else t.double()
        with pytest.raises(TypeError, match=nm):
            loadgen.moe_route(lg, 2, **dict(good, **{nm: wrong_type}))
        longer = torch.zeros(t.numel() + 1, dtype=t.dtype)
        with pytest.raises(ValueError, match=f"{nm} must be contiguous of shape"):
            loadgen.moe_route(lg, 2, **dict(good, **{nm: longer}))
    with pytest.raises(ValueError, match="topk_ids must be contiguous"):
        loadgen.moe_route(lg, 2, **dict(good, topk_ids=torch.zeros(3, 4, dtype=I32)[:, ::2]))
    with pytest.raises(ValueError, match="slot_pos overlaps topk_ids"):
        loadgen.moe_route(lg, 2, **dict(good, slot_pos=good["topk_ids"].view(-1)))
    with pytest.raises(ValueError, match="topk_w overlaps topk_ids"):
        loadgen.moe_route(lg, 2, **dict(good, topk_w=good["topk_ids"].view(torch.float32)))
    shared = torch.zeros(24, dtype=I32)                              # logits and topk_ids in one allocation
    with pytest.raises(ValueError, match="topk_ids overlaps logits"):
        loadgen.moe_route(shared.view(BF).view(3, 16), 2, **dict(good, topk_ids=shared[:6].view(3, 2)))


def _gemm_args(T=3, k=2, E=8, N=128, K=64):
    s, t, _, _ = loadgen.moe_align_reference(torch.arange(T * k, dtype=I32).view(T, k) % E, E)
    return torch.zeros(T, K, dtype=BF), torch.zeros(E, N, K, dtype=BF), s, t, T * k


def test_moe_gemm_rejections(host_operands_pass):
    a, w, s, t, n = _gemm_args()
    P = s.numel()
    with pytest.raises(AssertionError, match=TOUCHED):
        loadgen.moe_gemm(a, w, s, t, n, gather_div=2)
    with pytest.raises(AssertionError, match=TOUCHED):               # strided a, w and out are legal
        loadgen.moe_gemm(torch.zeros(3, 72, dtype=BF)[:, 8:], torch.zeros(8, 130, 72, dtype=BF)[:, 1:129, :64], s, t, n,
                         gather_div=2, out=torch.zeros(P, 136, dtype=BF)[:, 8:], check=False)
    with pytest.raises(AssertionError, match=TOUCHED):               # one matrix shared by every expert
        loadgen.moe_gemm(a, w[:1].expand(8, 128, 64), s, t, n, gather_div=2)
    with pytest.raises(TypeError, match="gather_div"):
        loadgen.moe_gemm(a, w, s, t, n)                              # keyword-only and required
    with pytest.raises(TypeError, match="bf16 tensors"):
        loadgen.moe_gemm(a.float(), w, s, t, n, gather_div=2)
    with pytest.raises(TypeError, match="w is"):
        loadgen.moe_gemm(a, w.float(), s, t, n, gather_div=2)
    with pytest.raises(TypeError, match="int32 sorted_ids and tile_expert"):
        loadgen.moe_gemm(a, w, s.long(), t, n, gather_div=2)
    with pytest.raises(TypeError, match="int32 sorted_ids and tile_expert"):
        loadgen.moe_gemm(a, w, s, t.long(), n, gather_div=2)
    with pytest.raises(ValueError, match="a must be 2-D"):
        loadgen.moe_gemm(a[0], w, s, t, n, gather_div=2)
    with pytest.raises(ValueError, match="a row stride 68"):
        loadgen.moe_gemm(torch.zeros(3, 68, dtype=BF)[:, :64], w, s, t, n, gather_div=2)
    with pytest.raises(ValueError, match=r"w must be \[E, N, K = 64\]"):
        loadgen.moe_gemm(a, torch.zeros(8, 128, 128, dtype=BF), s, t, n, gather_div=2)
    with pytest.raises(ValueError, match=r"w must be \[E, N, K = 64\]"):
        loadgen.moe_gemm(a, w[0], s, t, n, gather_div=2)
    with pytest.raises(ValueError, match="E = 257"):
        loadgen.moe_gemm(a, torch.zeros(1, 64, 64, dtype=BF).expand(257, 64, 64), s, t, n, gather_div=2)
    for N, K in ((96, 64), (64, 96), (32, 64)):
        with pytest.raises(ValueError, match="positive multiples of 64"):
            loadgen.moe_gemm(torch.zeros(3, K, dtype=BF), torch.zeros(8, N, K, dtype=BF), s, t, n, gather_div=2)
    with pytest.raises(ValueError, match="K-contiguous"):
        loadgen.moe_gemm(a, torch.zeros(8, 128, 128, dtype=BF)[:, :, ::2], s, t, n, gather_div=2)
    with pytest.raises(ValueError, match="w row stride 68"):
        loadgen.moe_gemm(a, torch.zeros(8, 128, 68, dtype=BF)[:, :, :64], s, t, n, gather_div=2)
    with pytest.raises(ValueError, match="w expert stride"):
        loadgen.moe_gemm(a, torch.zeros(8 * 128 * 64 + 28, dtype=BF).as_strided((8, 128, 64), (128 * 64 + 4, 64, 1)), s, t, n,
                         gather_div=2)
    with pytest.raises(ValueError, match="w must be 16-byte aligned"):
        loadgen.moe_gemm(a, torch.zeros(8 * 128 * 64 + 8, dtype=BF)[4:-4].view(8, 128, 64), s, t, n, gather_div=2)
    with pytest.raises(ValueError, match="contiguous vectors"):
        loadgen.moe_gemm(a, w, s.repeat(2)[::2], t, n, gather_div=2)
    with pytest.raises(ValueError, match="contiguous vectors"):
        loadgen.moe_gemm(a, w, s.view(-1, 64), t, n, gather_div=2)
    with pytest.raises(ValueError, match="sorted_ids has"):
        loadgen.moe_gemm(a, w, s[:-64], t, n, gather_div=2)
    for bad in (-1, 32769, 2.0, True):
        with pytest.raises(ValueError, match="n_slots"):
            loadgen.moe_gemm(a, w, s, t, bad, gather_div=2)
    for bad in (-1, 9, 1.0, False, None):
        with pytest.raises(ValueError, match="gather_div"):
            loadgen.moe_gemm(a, w, s, t, n, gather_div=bad)
    with pytest.raises(ValueError, match="out must be 2-D with 128 columns"):
        loadgen.moe_gemm(a, w, s, t, n, gather_div=2, out=torch.zeros(P, 64, dtype=BF))
    with pytest.raises(ValueError, match=f"out has {P - 64} rows"):
        loadgen.moe_gemm(a, w, s, t, n, gather_div=2, out=torch.zeros(P - 64, 128, dtype=BF))
    with pytest.raises(TypeError, match="out is"):
        loadgen.moe_gemm(a, w, s, t, n, gather_div=2, out=torch.zeros(P, 128))
    big = torch.zeros(max(P * 128, 8 * 128 * 64), dtype=BF)
    with pytest.raises(ValueError, match="out overlaps w"):
        loadgen.moe_gemm(a, big[:8 * 128 * 64].view(8, 128, 64), s, t, n, gather_div=2, out=big[:P * 128].view(P, 128))
    with pytest.raises(ValueError, match="out overlaps a"):
        loadgen.moe_gemm(big[:P * 64].view(P, 64), w, s, t, n, gather_div=0, out=big[:P * 128].view(P, 128))


def test_moe_gemm_with_no_tile_is_a_no_op(host_operands_pass):
    e = torch.zeros(0, dtype=I32)
    out = loadgen.moe_gemm(torch.zeros(0, 64, dtype=BF), torch.zeros(8, 64, 64, dtype=BF), e, e.clone(), 0, gather_div=2)
    assert out.shape == (0, 64) and out.dtype == BF


def test_moe_combine_rejections(host_operands_pass):
    y, p, w = torch.zeros(128, 16, dtype=BF), torch.zeros(6, dtype=I32), torch.ones(3, 2)
    with pytest.raises(AssertionError, match=TOUCHED):
        loadgen.moe_combine(y, p, w)
    with pytest.raises(AssertionError, match=TOUCHED):
        loadgen.moe_combine(torch.zeros(128, 24, dtype=BF)[:, 8:], p, w, out=torch.zeros(3, 32, dtype=BF)[:, :16])
    with pytest.raises(TypeError, match="fp32 topk_w"):
        loadgen.moe_combine(y, p, w.double())
    with pytest.raises(TypeError, match="int32 slot_pos"):
        loadgen.moe_combine(y, p.long(), w)
    with pytest.raises(TypeError, match="y is"):
        loadgen.moe_combine(y.float(), p, w)
    with pytest.raises(ValueError, match="y must be 2-D"):
        loadgen.moe_combine(y[0], p, w)
    with pytest.raises(ValueError, match="y row stride 20"):
        loadgen.moe_combine(torch.zeros(128, 20, dtype=BF)[:, :16], p, w)
    for D in (0, 4, 12):
        with pytest.raises(ValueError, match="positive multiple of 8"):
            loadgen.moe_combine(torch.zeros(128, D, dtype=BF), p, w)
    for bad in (w[0], torch.ones(3, 9), torch.ones(3, 0), torch.ones(3, 4)[:, ::2]):
        with pytest.raises(ValueError, match="topk_w must be contiguous"):
            loadgen.moe_combine(y, p, bad)
    for bad in (p[:5], p.view(3, 2), torch.zeros(12, dtype=I32)[::2]):
        with pytest.raises(ValueError, match="slot_pos must be a contiguous vector of length T \\* k = 6"):
            loadgen.moe_combine(y, bad, w)
    with pytest.raises(ValueError, match="out must be 2-D with 16 columns"):
        loadgen.moe_combine(y, p, w, out=torch.zeros(3, 8, dtype=BF))
    with pytest.raises(ValueError, match="does not match the 3 tokens"):
        loadgen.moe_combine(y, p, w, out=torch.zeros(4, 16, dtype=BF))
    with pytest.raises(ValueError, match="out overlaps y"):
        loadgen.moe_combine(y, p, w, out=y[:3])
    w8 = torch.ones(3, 8)
    with pytest.raises(ValueError, match="out overlaps topk_w"):
        loadgen.moe_combine(y, torch.zeros(24, dtype=I32), w8, out=w8.view(BF))
    out = loadgen.moe_combine(torch.zeros(0, 16, dtype=BF), torch.zeros(0, dtype=I32), torch.ones(0, 2))      # T == 0
    assert out.shape == (0, 16)


def test_moe_mlp_rejections(host_operands_pass):
    x, lg = torch.zeros(3, 64, dtype=BF), torch.zeros(3, 16, dtype=BF)
    w13, w2 = torch.zeros(16, 128, 64, dtype=BF), torch.zeros(16, 64, 64, dtype=BF)
    with pytest.raises(AssertionError, match=TOUCHED):
        loadgen.moe_mlp(x, lg, w13, w2, 2, workspace=loadgen.moe_workspace(3, 16, 2, 64, 64, "cpu"))
    with pytest.raises(TypeError, match="w2 is"):
        loadgen.moe_mlp(x, lg, w13, w2.float(), 2)
    with pytest.raises(ValueError, match="expects x"):
        loadgen.moe_mlp(x[0], lg, w13, w2, 2)
    for bad in (dict(lg=torch.zeros(4, 16, dtype=BF)), dict(w13=torch.zeros(16, 64, 64, dtype=BF)),
                dict(w2=torch.zeros(8, 64, 64, dtype=BF)), dict(x=torch.zeros(3, 128, dtype=BF))):
        args = dict(x=x, lg=lg, w13=w13, w2=w2)
        args.update(bad)
        with pytest.raises(ValueError, match="disagree"):
            loadgen.moe_mlp(args["x"], args["lg"], args["w13"], args["w2"], 2)
    with pytest.raises(ValueError, match="top_k"):
        loadgen.moe_mlp(x, lg, w13, w2, 9)
    ws = loadgen.moe_workspace(3, 16, 2, 64, 64, "cpu")
    tiles = W.moe_max_tiles(3, 2, 16)
    assert {k: tuple(v.shape) for k, v in ws.items()} == {
        "topk_ids": (3, 2), "topk_w": (3, 2), "sorted_ids": (64 * tiles,), "tile_expert": (tiles,), "expert_offsets": (17,),
        "slot_pos": (6,), "h13": (64 * tiles, 128), "act": (64 * tiles, 64), "y": (64 * tiles, 64)}
    assert not bool(ws["h13"].any())


# ------------------------------------------------------------------------------------------------
# executor
# ------------------------------------------------------------------------------------------------
def test_enqueue_ops_dispatches_the_kinds(monkeypatch):
    from k8s_gpu_scheduler_amd.parallel import executor
    calls = []
    for fn in ("moe_route", "moe_gemm", "moe_combine"):
        monkeypatch.setattr(loadgen, fn, lambda *a, _fn=fn, **k: calls.append((_fn, a, k)))

    class Stub:
        ops = [(W.Op("moe_route", 3, 16, 2), ("ids", "logits", "w", "sorted", "tile", "off", "pos")),
               (W.Op("moe_gemm", 3, 128, 64, rows=16, q=2, gather=True), ("out", "a", "w", "sorted", "tile")),
               (W.Op("moe_gemm", 3, 64, 64, rows=16, q=2), ("out", "a", "w", "sorted", "tile")),
               (W.Op("moe_combine", 3, 64, 2, rows=16), ("out", "y", "pos", "w"))]

    executor.enqueue_ops(Stub(), 1, "stream", 64)
    assert calls == [
        ("moe_route", ("logits", 2), dict(topk_ids="ids", topk_w="w", sorted_ids="sorted", tile_expert="tile",
                                          expert_offsets="off", slot_pos="pos", stream="stream", check=False)),
        ("moe_gemm", ("a", "w", "sorted", "tile", 6), dict(gather_div=2, out="out", stream="stream", check=False)),
        ("moe_gemm", ("a", "w", "sorted", "tile", 6), dict(gather_div=0, out="out", stream="stream", check=False)),
        ("moe_combine", ("y", "pos", "w"), dict(out="out", stream="stream"))]
    assert executor.op_output(*Stub.ops[0]) == "ids" and executor.op_output(*Stub.ops[1]) == "out"
    assert all(executor.OP_KINDS[k][2] == 0 for k in MOE_KINDS)
    assert {o.kind for w in W.LLM_MOE.values() for o in w.ops} <= set(executor.OP_KINDS)


def test_buffers_build_the_operands_on_the_cpu_device():
    from k8s_gpu_scheduler_amd.parallel.executor import _Buffers
    T, E, k, D, F = 70, 16, 4, 128, 64
    tiles = W.moe_max_tiles(T, k, E)
    P = 64 * tiles
    w = W.Workload("t_moe", "test", "hip", T, (
        W.Op("add_rmsnorm", T, D), W.Op("gemm", 128, E * 4, D, relu=False), W.Op("moe_route", T, E, k),
        W.Op("moe_gemm", T, 2 * F, D, rows=E, q=k, gather=True), W.Op("swiglu", P, F),
        W.Op("moe_gemm", T, D, F, rows=E, q=k), W.Op("moe_combine", T, D, k, rows=E)), 0.0)
    cpu = torch.device("cpu")
    a, b = _Buffers(w, cpu), _Buffers(w, cpu)
    ids, logits, tw, s, t, off, pos = a.ops[2][1]
    assert logits.shape == (T, E) and logits.dtype == BF and ids.shape == tw.shape == (T, k) and tw.dtype == torch.float32
    assert (s.shape, t.shape, off.shape, pos.shape) == ((P,), (tiles,), (E + 1,), (T * k,))
    for i, (rows_a, N, K, gather) in ((3, (T, 2 * F, D, True)), (5, (P, D, F, False))):
        out, x, wt, s, t = a.ops[i][1]
        assert out.shape == (P, N) and not bool(out.any()) and x.shape == (rows_a, K) and wt.shape == (E, N, K)
        assert all(v.dtype == BF for v in (out, x, wt)) and s.dtype == t.dtype == I32
        assert torch.equal(wt[0], wt[4]) and torch.equal(wt[3], wt[15]) and not torch.equal(wt[0], wt[1])    # four experts repeat
        assert 0 < wt.float().abs().max() <= torch.tensor(0.05).to(BF).item() and s.shape == (P,) and t.shape == (tiles,)
        used = int((t >= 0).sum())
        assert 0 < used <= tiles and bool((t[:used] >= 0).all()) and bool((t[used:] == -1).all())
        real = s[s < T * k].long()
        assert torch.equal(real.sort().values, torch.arange(T * k))                 # a consistent layout of every slot
        assert bool((s.view(tiles, 64)[:used, 0] < T * k).all())
    out, y, pos, tw = a.ops[6][1]
    assert out.shape == (T, D) and y.shape == (P, D) and pos.shape == (T * k,) and tw.shape == (T, k)
    assert torch.allclose(tw.sum(1), torch.ones(T), atol=1e-6) and bool((tw[:, :-1] >= tw[:, 1:]).all())
    assert len(pos.unique()) == T * k and int(pos.max()) < P
    for (o, x), (_, z) in zip(a.ops, b.ops):                          # the MoE ops' inputs are reproducible
        if o.kind in MOE_KINDS:
            last = 2 if o.kind == "moe_route" else None               # (the routing's other six are torch.empty outputs)
            for u, v in zip(x[1:last], z[1:last]):
                assert torch.equal(u, v) and u.data_ptr() != v.data_ptr()


def test_the_executors_operands_pass_the_wrappers(host_operands_pass):
    from k8s_gpu_scheduler_amd.parallel import executor
    T, E, k = 70, 16, 4
    w = W.Workload("t_moe2", "test", "hip", T, (
        W.Op("moe_route", T, E, k), W.Op("moe_gemm", T, 128, 128, rows=E, q=k, gather=True),
        W.Op("moe_gemm", T, 128, 64, rows=E, q=k), W.Op("moe_combine", T, 128, k, rows=E)), 0.0)
    bufs = executor._Buffers(w, torch.device("cpu"))
    for o, t in bufs.ops:
        with pytest.raises(AssertionError, match=TOUCHED):           # valid all the way to the launch
            executor.enqueue_op(o, t, None, 64)


# ------------------------------------------------------------------------------------------------
# the native grid rules
# ------------------------------------------------------------------------------------------------
@pytest.mark.skipif(_native.hip(required=False) is None, reason="HIP extension not built")
def test_default_workgroups_match_the_native_rules():
    h = _native.hip()
    for T, k, E in ((0, 1, 8), (1, 1, 8), (3, 2, 8), (64, 8, 64), (65, 8, 128), (256, 8, 128), (2048, 8, 128), (4096, 8, 256),
                    (32768, 1, 256), (200, 2, 16)):
        assert h.moe_max_tiles(T, k, E) == W.moe_max_tiles(T, k, E)
        assert h.moe_route_workgroups(T) == W.default_moe_route_workgroups(T)
        for N in (64, 128, 192, 256, 1536, 2048):
            assert h.moe_gemm_workgroups(T, k, E, N) == W.default_moe_gemm_workgroups(T, k, E, N)
        for D in (8, 2048, 2056):
            assert h.moe_combine_workgroups(T, D) == W.default_moe_combine_workgroups(T, D)
    for bad in ((4097, 8, 8), (1, 9, 16), (1, 0, 16), (1, 1, 257), (-1, 1, 8)):
        with pytest.raises(RuntimeError):
            h.moe_max_tiles(*bad)
    with pytest.raises(RuntimeError):
        h.moe_gemm_workgroups(4, 2, 8, 96)
    with pytest.raises(RuntimeError):
        h.moe_combine_workgroups(4, 12)
    with pytest.raises(RuntimeError):
        h.moe_route_workgroups(-1)
