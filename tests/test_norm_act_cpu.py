"""The residual add + RMSNorm and SwiGLU without a GPU: the workload model's two op kinds, the two LLM-block
workloads and their table, the pure-Python grid rules, the host wrappers' validation (which must fire before
the native module is touched), the executor's op dispatch and operands, and the references of the GPU tests.
The kernels themselves are pinned on the GPU by test_gpu_rmsnorm_exact.py and test_gpu_swiglu_exact.py."""
import pytest
import torch

from k8s_gpu_scheduler_amd import _native
from k8s_gpu_scheduler_amd.models import workloads as W
from k8s_gpu_scheduler_amd.ops import loadgen

BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------
# workload model
# ------------------------------------------------------------------------------------------------
def test_op_flops_bytes_workgroups():
    n = W.Op("add_rmsnorm", 3, 2056)
    assert not n.is_gemm and not n.on_mfma and n.mfma_rate() == 1.0
    assert n.flops == 5 * 3 * 2056 == 30840
    assert n.bytes == 8 * 3 * 2056 + 2 * 2056 == 53456               # two reads, two writes, the weight
    assert n.workgroups(0) == n.workgroups(64) == 3
    s = W.Op("swiglu", 5, 14336)
    assert not s.is_gemm and not s.on_mfma and s.mfma_rate() == 1.0
    assert s.flops == 6 * 5 * 14336 == 430080
    assert s.bytes == 6 * 5 * 14336 == 430080                        # gate and up read, out written
    assert s.workgroups(0) == s.workgroups(64) == 9
    assert W.Op("add_rmsnorm", 0, 4096).bytes == 8192 and W.Op("add_rmsnorm", 0, 4096).workgroups(0) == 0
    assert W.Op("swiglu", 0, 8).flops == 0 and W.Op("swiglu", 0, 8).workgroups(0) == 0


def test_default_workgroups():
    got = [W.default_swiglu_workgroups(*x) for x in ((1, 8), (1, 8192), (1, 8200), (5, 14336), (256, 14336),
                                                     (2048, 14336), (0, 14336))]
    assert got == [1, 1, 2, 9, 448, 3584, 0]
    assert W.SWIGLU_CHUNKS_PER_WORKGROUP == 1024
    for T, F in ((3, 1016), (3, 1024), (3, 1032), (7, 8184), (1025, 8)):
        assert W.default_swiglu_workgroups(T, F) == -(-T * F // 8192)
    assert [W.default_add_rmsnorm_workgroups(t) for t in (0, 1, 256, 2048)] == [0, 1, 256, 2048]


@pytest.mark.skipif(_native.hip(required=False) is None, reason="HIP extension not built")
def test_default_workgroups_match_the_native_rules():
    h = _native.hip()
    for T in (0, 1, 3, 5, 256, 2048, 100000, 2 ** 31 - 1):
        assert h.add_rmsnorm_workgroups(T) == W.default_add_rmsnorm_workgroups(T)
        for F in (8, 16, 1016, 1024, 1032, 8192, 8200, 14336):
            if T * (F // 8) >= 2 ** 31 * 1024:                       # past the grid limit: raises, below
                continue
            assert h.swiglu_workgroups(T, F) == W.default_swiglu_workgroups(T, F), (T, F)
    for bad in ((1, 0), (1, 12), (-1, 8)):
        with pytest.raises(RuntimeError):
            h.swiglu_workgroups(*bad)
    with pytest.raises(RuntimeError):
        h.swiglu_workgroups(2 ** 31 - 1, 16384)                      # 2^32 - 2 workgroups
    with pytest.raises(RuntimeError):
        h.add_rmsnorm_workgroups(-1)


def operand_bytes(o):
    """Bytes of the operands parallel.executor allocates for one op, from its shapes."""
    D, T = W.ATTN_HEAD_DIM, W.ATTN_BLOCK_TOKENS
    if o.kind == "gemm":
        return 2 * (o.M * o.K + o.N * o.K + o.M * o.N) + 4 * o.N
    if o.kind == "add_rmsnorm":
        return 2 * (4 * o.M * o.N + o.N)
    if o.kind == "swiglu":
        return 2 * 3 * o.M * o.N
    caches = 2 * 2 * (o.M * o.K // T) * o.rows * T * D
    ints = 4 * (o.M * o.K // T) + 4 * o.M
    if o.kind == "attn":
        return caches + ints + 2 * 2 * o.M * o.N * D
    if o.kind == "prefill":
        return caches + ints + 4 * (o.M + 1) + 2 * 2 * o.M * o.q * o.N * D
    if o.kind == "rope_append":
        return (caches + ints + 4 * (o.M + 1) + 2 * o.M * o.q * (o.N + 2 * o.rows) * D + 2 * o.M * o.q * o.N * D
                + 4 * o.K * D)
    raise AssertionError(o.kind)


def test_llm_block_workloads_and_their_table():
    dec, pre = W.get("llm_block_decode_256"), W.get("llm_block_prefill_2048")
    assert W.LLM_BLOCK == {"llm_block_decode_256": dec, "llm_block_prefill_2048": pre}
    G = lambda m, n, k: W.Op("gemm", m, n, k, relu=False)            # noqa: E731
    assert dec.ops == (W.Op("add_rmsnorm", 256, 4096), G(256, 6144, 4096), W.Op("rope_append", 256, 32, 1024, rows=8, q=1),
                       W.Op("attn", 256, 32, 1024, rows=8), G(256, 4096, 4096), W.Op("add_rmsnorm", 256, 4096),
                       G(256, 28672, 4096), W.Op("swiglu", 256, 14336), G(256, 4096, 14336))
    assert pre.ops == (W.Op("add_rmsnorm", 2048, 4096), G(2048, 6144, 4096), W.Op("rope_append", 2, 32, 4096, rows=8, q=1024),
                       W.Op("prefill", 2, 32, 4096, rows=8, q=1024), G(2048, 4096, 4096), W.Op("add_rmsnorm", 2048, 4096),
                       G(2048, 28672, 4096), W.Op("swiglu", 2048, 14336), G(2048, 4096, 14336))
    assert (dec.family, dec.framework, dec.batch, dec.hbm_gib) == ("llm_block_decode", "hip", 256, 2.5)
    assert (pre.family, pre.framework, pre.batch, pre.hbm_gib) == ("llm_block_prefill", "hip", 2048, 1.25)
    for w in (dec, pre):
        n1, qkv, a, att, proj, n2, gu, act, down = w.ops
        rows = a.M * a.q
        assert all(not o.relu for o in w.ops if o.is_gemm) and all(o.M == rows for o in (n1, qkv, proj, n2, gu, act, down))
        assert n1.N == qkv.K == 4096 and qkv.N == (a.N + 2 * a.rows) * W.ATTN_HEAD_DIM == (32 + 16) * 128
        assert (att.M, att.N, att.K, att.rows) == (a.M, a.N, a.K, a.rows) and proj.K == a.N * W.ATTN_HEAD_DIM
        assert proj.N == n2.N == gu.K == 4096 and gu.N == 2 * act.N and down.K == act.N == 14336 and down.N == n1.N
        need = sum(operand_bytes(o) for o in w.ops)
        assert w.hbm_gib * 2 ** 30 >= need > (w.hbm_gib - 0.25) * 2 ** 30, (w.name, need / 2 ** 30)
        assert 0.0 < W.cu_fill(w) <= 1.0
        m, h = W.roofline_split(w.name.replace("_", "-") + "-0")
        assert m > 0 and h >= (n1.bytes + n2.bytes + act.bytes) / 6.0e12 > 0
        # the MLP is the block's dominant GEMM work
        assert gu.flops + down.flops > 2 * (qkv.flops + proj.flops)
    assert [o.workgroups(64) for o in dec.ops if not o.is_gemm] == [256, 2048, 2048, 256, 448]
    assert [o.workgroups(64) for o in pre.ops if not o.is_gemm] == [2048, 528, 512, 2048, 3584]
    # the older tables are unchanged, and hold neither new kind
    assert len(W.CATALOG) == 18 and set(W.EXTRA) == {"fp8_llm_2048", "triad_only_2048", "dlrm_2048", "llm_decode_256"}
    assert set(W.STAGED) == {"llm_prefill_2048"} and set(W.LONG_CONTEXT) == {"llm_decode_long_8"}
    assert set(W.LLM_LAYER) == {"llm_layer_decode_256", "llm_layer_prefill_2048"}
    assert W.LLM_LAYER["llm_layer_decode_256"].ops == (W.Op("gemm", 256, 6144, 4096), W.Op("rope_append", 256, 32, 1024, rows=8, q=1),
                                                       W.Op("attn", 256, 32, 1024, rows=8), W.Op("gemm", 256, 4096, 4096))
    for table in (W.CATALOG, W.EXTRA, W.STAGED, W.LONG_CONTEXT, W.LLM_LAYER):
        assert all(o.kind not in ("add_rmsnorm", "swiglu") for w in table.values() for o in w.ops)


def test_get_and_workload_for_pod():
    dec, pre = W.LLM_BLOCK["llm_block_decode_256"], W.LLM_BLOCK["llm_block_prefill_2048"]
    assert W.get("llm_block_decode_256") is dec and W.get("llm_block_prefill_2048") is pre
    assert W.workload_for_pod("llm-block-decode-256-x") is dec and W.workload_for_pod("pod-llm-block-prefill-2048-7") is pre
    assert W.workload_for_pod("llm-layer-decode-256-x") is W.LLM_LAYER["llm_layer_decode_256"]
    assert W.workload_for_pod("llm-decode-256-x") is W.EXTRA["llm_decode_256"]
    # a pod name that holds an old and a new name: the older tables are consulted first
    assert W.workload_for_pod("llm-block-decode-256-and-llm-layer-decode-256") is W.LLM_LAYER["llm_layer_decode_256"]
    assert W.workload_for_pod("llm-block-prefill-2048-and-llm-prefill-2048") is W.STAGED["llm_prefill_2048"]
    names = [n for t in (W.CATALOG, W.EXTRA, W.STAGED, W.LONG_CONTEXT, W.LLM_LAYER) for n in t]
    for new in W.LLM_BLOCK:
        assert not any(old in new or new in old for old in names)
    for bad in ("llm_block", "llm_block_decode", "llm-block-decode-256", "llm_block_decode_255"):
        with pytest.raises(KeyError):
            W.get(bad)
    with pytest.raises(KeyError):
        W.workload_for_pod("llm-block-decode-255")
    with pytest.raises(KeyError):
        W.workload_for_pod("llm-block-prefill-204")


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


def _norm(T=3, D=16):
    return torch.zeros(T, D, dtype=BF), torch.ones(D, dtype=BF), torch.zeros(T, D, dtype=BF)


def test_wrappers_reject_cpu_tensors(no_native):
    x, w, r = _norm()
    with pytest.raises(ValueError, match="device tensors"):
        loadgen.add_rmsnorm(x, w, r)
    with pytest.raises(ValueError, match="device tensors"):          # before any dtype complaint
        loadgen.add_rmsnorm(x.float(), w)
    with pytest.raises(ValueError, match="device tensors"):
        loadgen.swiglu(torch.zeros(3, 32, dtype=BF))


def test_add_rmsnorm_rejects_dtypes_shapes_and_strides(host_operands_pass):
    x, w, r = _norm()
    for bad in ((x.float(), w, r), (x, w.float(), r), (x, w, r.half())):
        with pytest.raises(TypeError, match="bf16"):
            loadgen.add_rmsnorm(*bad)
    with pytest.raises(TypeError, match="bf16"):
        loadgen.add_rmsnorm(x, w, r, out=torch.zeros(3, 16))
    with pytest.raises(TypeError, match="bf16"):
        loadgen.add_rmsnorm(x, w, r, residual_out=torch.zeros(3, 16))
    for bad in (x[0], x[None]):
        with pytest.raises(ValueError, match="x must be 2-D"):
            loadgen.add_rmsnorm(bad, w)
    for D in (0, 4, 12, 8200, 16384):
        with pytest.raises(ValueError, match=r"multiple of 8 in \[8, 8192\]"):
            loadgen.add_rmsnorm(torch.zeros(2, D, dtype=BF), torch.ones(D, dtype=BF))
    with pytest.raises(ValueError, match="contiguous rows"):
        loadgen.add_rmsnorm(torch.zeros(3, 32, dtype=BF)[:, ::2], w)
    with pytest.raises(ValueError, match="x row stride 20"):
        loadgen.add_rmsnorm(torch.zeros(3, 20, dtype=BF)[:, :16], w)
    with pytest.raises(ValueError, match="x row stride 8"):          # rows overlap
        loadgen.add_rmsnorm(torch.zeros(64, dtype=BF).as_strided((3, 16), (8, 1)), w)
    with pytest.raises(ValueError, match="x must be 16-byte aligned"):
        loadgen.add_rmsnorm(torch.zeros(3 * 16 + 8, dtype=BF)[4:4 + 48].view(3, 16), w)
    with pytest.raises(ValueError, match="residual row stride 20"):
        loadgen.add_rmsnorm(x, w, torch.zeros(3, 20, dtype=BF)[:, :16])
    with pytest.raises(ValueError, match="residual must be 2-D with 16 columns"):
        loadgen.add_rmsnorm(x, w, torch.zeros(3, 24, dtype=BF))
    with pytest.raises(ValueError, match="residual .* does not match"):
        loadgen.add_rmsnorm(x, w, torch.zeros(2, 16, dtype=BF))
    with pytest.raises(ValueError, match="out must be 2-D with 16 columns"):
        loadgen.add_rmsnorm(x, w, out=torch.zeros(3, 8, dtype=BF))
    with pytest.raises(ValueError, match="out .* does not match"):
        loadgen.add_rmsnorm(x, w, out=torch.zeros(4, 16, dtype=BF))
    with pytest.raises(ValueError, match="out row stride 20"):
        loadgen.add_rmsnorm(x, w, out=torch.zeros(3, 20, dtype=BF)[:, :16])
    with pytest.raises(ValueError, match="residual_out must be 16-byte aligned"):
        loadgen.add_rmsnorm(x, w, r, residual_out=torch.zeros(3 * 16 + 8, dtype=BF)[4:4 + 48].view(3, 16))
    # the weight: a contiguous, 16-byte aligned [D]
    for bad in (torch.ones(8, dtype=BF), torch.ones(1, 16, dtype=BF), torch.ones(32, dtype=BF)[::2],
                torch.ones(24, dtype=BF)[4:20]):
        with pytest.raises(ValueError, match="weight must be a contiguous, 16-byte aligned vector of length D = 16"):
            loadgen.add_rmsnorm(x, bad)


def test_add_rmsnorm_rejects_eps(host_operands_pass):
    x, w, r = _norm()
    for bad in (-1e-5, float("nan"), float("inf"), -float("inf"), None, "1e-5", True):
        with pytest.raises(ValueError, match="eps"):
            loadgen.add_rmsnorm(x, w, eps=bad)
    with pytest.raises(ValueError, match="fp32 range"):
        loadgen.add_rmsnorm(x, w, eps=1e39)
    for ok in (0.0, 0, 1e-6, 1e-45):
        assert loadgen.add_rmsnorm(x[:0], w, eps=ok).shape == (0, 16)


def test_add_rmsnorm_residual_rules(host_operands_pass):
    x, w, r = _norm()
    with pytest.raises(ValueError, match="residual_out without a residual"):
        loadgen.add_rmsnorm(x, w, residual_out=torch.zeros(3, 16, dtype=BF))
    # exactly residual is allowed: every check passes and the native module is asked for
    big = torch.zeros(3, 24, dtype=BF)
    view = big[:, 8:]
    with pytest.raises(AssertionError, match="native module was touched"):
        loadgen.add_rmsnorm(x, w, view, residual_out=view)           # every check passed
    with pytest.raises(AssertionError, match="native module was touched"):
        loadgen.add_rmsnorm(x, w, r, residual_out=r)
    # any other overlap of residual_out with residual
    with pytest.raises(ValueError, match="residual_out overlaps residual"):
        loadgen.add_rmsnorm(x[:2], w, r[:2], residual_out=r[1:])     # shifted by a row
    wide = torch.zeros(3, 32, dtype=BF)
    with pytest.raises(ValueError, match="residual_out overlaps residual"):
        loadgen.add_rmsnorm(x, w, wide[:, :16], residual_out=wide[:, 16:])      # interleaved rows of one allocation
    with pytest.raises(ValueError, match="residual_out overlaps residual"):
        loadgen.add_rmsnorm(x, w, wide[:, :16], residual_out=wide.view(6, 16)[:3])   # same data_ptr, other strides
    with pytest.raises(ValueError, match="residual_out overlaps x"):
        loadgen.add_rmsnorm(x, w, r, residual_out=x)
    with pytest.raises(ValueError, match="out overlaps x"):
        loadgen.add_rmsnorm(x, w, r, out=x)
    with pytest.raises(ValueError, match="out overlaps residual"):
        loadgen.add_rmsnorm(x, w, r, out=r)
    ro = torch.zeros(3, 16, dtype=BF)
    with pytest.raises(ValueError, match="out overlaps residual_out"):
        loadgen.add_rmsnorm(x, w, r, out=ro, residual_out=ro)
    with pytest.raises(ValueError, match="out overlaps weight"):
        loadgen.add_rmsnorm(torch.zeros(1, 16, dtype=BF), w, out=w[None, :])
    with pytest.raises(ValueError, match="out overlaps residual"):   # in place, and y into the same rows
        loadgen.add_rmsnorm(x, w, r, out=r, residual_out=r)


def test_add_rmsnorm_empty_launches_nothing(host_operands_pass):
    x, w, r = _norm(T=0)
    y = loadgen.add_rmsnorm(x, w)
    assert y.shape == (0, 16) and y.dtype == BF
    y, ro = loadgen.add_rmsnorm(x, w, r)
    assert y.shape == ro.shape == (0, 16)
    given = torch.ones(0, 16, dtype=BF)
    assert loadgen.add_rmsnorm(x, w, out=given) is given
    got = loadgen.add_rmsnorm(x, w, r, residual_out=r)
    assert got[1] is r


def test_swiglu_rejections_and_empty(host_operands_pass):
    gu = torch.zeros(3, 32, dtype=BF)
    for bad in (gu.float(), gu.half()):
        with pytest.raises(TypeError, match="bf16"):
            loadgen.swiglu(bad)
    with pytest.raises(TypeError, match="bf16"):
        loadgen.swiglu(gu, out=torch.zeros(3, 16))
    for bad in (gu[0], gu[None]):
        with pytest.raises(ValueError, match="gate_up must be 2-D"):
            loadgen.swiglu(bad)
    for cols in (0, 8, 24, 20):
        with pytest.raises(ValueError, match="no 2 \\* F"):
            loadgen.swiglu(torch.zeros(3, cols, dtype=BF))
    with pytest.raises(ValueError, match="contiguous rows"):
        loadgen.swiglu(torch.zeros(3, 64, dtype=BF)[:, ::2])
    with pytest.raises(ValueError, match="gate_up row stride 36"):
        loadgen.swiglu(torch.zeros(3, 36, dtype=BF)[:, :32])
    with pytest.raises(ValueError, match="gate_up row stride 16"):
        loadgen.swiglu(torch.zeros(96, dtype=BF).as_strided((3, 32), (16, 1)))
    with pytest.raises(ValueError, match="gate_up must be 16-byte aligned"):
        loadgen.swiglu(torch.zeros(3 * 32 + 8, dtype=BF)[4:4 + 96].view(3, 32))
    with pytest.raises(ValueError, match="out must be 2-D with 16 columns"):
        loadgen.swiglu(gu, out=torch.zeros(3, 32, dtype=BF))
    with pytest.raises(ValueError, match="out .* does not match"):
        loadgen.swiglu(gu, out=torch.zeros(2, 16, dtype=BF))
    with pytest.raises(ValueError, match="out row stride 20"):
        loadgen.swiglu(gu, out=torch.zeros(3, 20, dtype=BF)[:, :16])
    with pytest.raises(ValueError, match="out must be 16-byte aligned"):
        loadgen.swiglu(gu, out=torch.zeros(3 * 16 + 8, dtype=BF)[4:4 + 48].view(3, 16))
    with pytest.raises(ValueError, match="out overlaps gate_up"):
        loadgen.swiglu(gu, out=gu[:, :16])
    with pytest.raises(ValueError, match="out overlaps gate_up"):
        loadgen.swiglu(gu, out=gu[:, 16:])
    wide = torch.zeros(3, 48, dtype=BF)
    with pytest.raises(ValueError, match="out overlaps gate_up"):    # in the gap a padded row stride leaves
        loadgen.swiglu(wide[:, :32], out=wide[:, 32:])
    with pytest.raises(AssertionError, match="native module was touched"):
        loadgen.swiglu(gu)                                           # every check passed
    # T < 2^31 and T * F / 8 < 2^31 * 1024: a meta tensor has the shape and no memory
    with pytest.raises(ValueError, match="more than 2\\^31 - 1 rows"):
        loadgen.swiglu(torch.empty(2 ** 31, 16, dtype=BF, device="meta"))
    with pytest.raises(ValueError, match="more than 2\\^31 - 1 workgroups"):
        loadgen.swiglu(torch.empty(2 ** 31 - 1, 2 * 16384, dtype=BF, device="meta"))
    with pytest.raises(ValueError, match="more than 2\\^31 - 1 rows"):
        loadgen.add_rmsnorm(torch.empty(2 ** 31, 16, dtype=BF, device="meta"), torch.ones(16, dtype=BF))
    assert loadgen.swiglu(gu[:0]).shape == (0, 16)
    given = torch.ones(0, 16, dtype=BF)
    assert loadgen.swiglu(gu[:0], out=given) is given


# ------------------------------------------------------------------------------------------------
# executor
# ------------------------------------------------------------------------------------------------
def test_enqueue_ops_dispatches_both_kinds(monkeypatch):
    from k8s_gpu_scheduler_amd.parallel import executor
    calls = []
    monkeypatch.setattr(loadgen, "add_rmsnorm", lambda *a, **k: calls.append(("add_rmsnorm", a, k)))
    monkeypatch.setattr(loadgen, "swiglu", lambda *a, **k: calls.append(("swiglu", a, k)))

    class Stub:
        ops = [(W.Op("add_rmsnorm", 2, 16), ("y", "res_out", "x", "residual", "weight")),
               (W.Op("swiglu", 2, 16), ("out", "gate_up"))]

    executor.enqueue_ops(Stub(), 2, "stream", 64)
    assert calls == [("add_rmsnorm", ("x", "weight", "residual"), {"out": "y", "residual_out": "res_out", "stream": "stream"}),
                     ("swiglu", ("gate_up",), {"out": "out", "stream": "stream"})] * 2
    assert executor.op_output(*Stub.ops[0]) == "y" and executor.op_output(*Stub.ops[1]) == "out"
    assert executor.OP_KINDS["add_rmsnorm"][2] == 0 and executor.OP_KINDS["swiglu"][2] == 0
    assert {o.kind for w in W.LLM_BLOCK.values() for o in w.ops} <= set(executor.OP_KINDS)


def test_buffers_build_the_operands_reproducibly():
    from k8s_gpu_scheduler_amd.parallel.executor import _Buffers
    w = W.Workload("t_norm_act", "test", "hip", 3, (W.Op("add_rmsnorm", 3, 4096), W.Op("swiglu", 3, 1032)), 0.0)
    cpu = torch.device("cpu")
    a, b = _Buffers(w, cpu), _Buffers(w, cpu)
    y, ro, x, res, wt = a.ops[0][1]
    assert all(t.shape == (3, 4096) and t.dtype == BF for t in (y, ro, x, res)) and wt.shape == (4096,) and wt.dtype == BF
    assert len({t.data_ptr() for t in (y, ro, x, res)}) == 4          # separate output buffers
    assert 0.5 < x.float().std() < 1.5 and 0.5 < res.float().std() < 1.5 and not torch.equal(x, res)
    assert abs(wt.float().mean() - 1) < 0.02 and 0.05 < wt.float().std() < 0.15
    out, gu = a.ops[1][1]
    assert out.shape == (3, 1032) and gu.shape == (3, 2064) and out.dtype == gu.dtype == BF and 0.5 < gu.float().std() < 1.5
    for (_, ta), (_, tb) in zip(a.ops, b.ops):
        for u, v in zip(ta[1:] if len(ta) == 2 else ta[2:], tb[1:] if len(tb) == 2 else tb[2:]):
            assert torch.equal(u.view(torch.int16), v.view(torch.int16))


# ------------------------------------------------------------------------------------------------
# the GPU tests' references
# ------------------------------------------------------------------------------------------------
def test_rmsnorm_references_assert_their_preconditions():
    import test_gpu_rmsnorm_exact as N
    N.test_the_shapes_cover_the_chunk_layouts()
    for D in (8, 2056, 8192):
        for eps in N.EPS:
            x, r, w = N.operands("integer", 5, D, True, eps, 1)
            ro, y, ss = N.emulate(x, w, r, eps)
            h = x.double() + r.double()
            assert torch.equal(ro.double(), h) and bool(h.abs().max() <= 16)        # the sum is exact in bf16
            assert torch.equal(ss.double(), (h * h).sum(-1)) and bool((ss < 2 ** 24).all())   # integral, below 2^24
            assert eps != 0.0 or bool((ss > 0).all())
            # any order of the sum gives the same bits
            assert torch.equal(N.emulate(x, w, r, eps, sequential=True)[1].view(torch.int16), y.view(torch.int16))
            assert torch.equal(N.emulate(x.flip(1), w.flip(0), r.flip(1), eps)[1].flip(1).view(torch.int16), y.view(torch.int16))
    for res in (True, False):
        x, r, w = N.operands("true", 5, 8192, res, 1e-5, 2)
        ro, y, _ = N.emulate(x, w, r, 1e-5)
        ref = N.reference(ro if res else x, w, 1e-5)
        assert bool((ref.abs() >= 2.0 ** -126).all()), "a subnormal or zero reference output"
        assert 0.08 < (w.float() - 1).std() < 0.12


def test_rmsnorm_emulation_is_inside_the_true_bound():
    """The fp32 emulation of the contract, with a sequential sum at D = 8192, against float64."""
    import test_gpu_rmsnorm_exact as N
    worst = 0.0
    for D in (8, 2056, 8192):
        for res in (True, False):
            x, r, w = N.operands("true", 5, D, res, 1e-5, 3)
            ro, y, _ = N.emulate(x, w, r, 1e-5, sequential=True)
            if res:
                assert torch.equal(ro.view(torch.int16), (x.float() + r.float()).to(BF).view(torch.int16))
            ref = N.reference(ro if res else x, w, 1e-5)
            ratio = ((y.double() - ref).abs() / (N.TRUE_BOUND * ref.abs())).max().item()
            worst = max(worst, ratio)
    print(f"add_rmsnorm emulation: max |y - ref| / bound = {worst:.4f}")
    assert 0.5 < worst <= 1.0, worst


def test_swiglu_references_assert_their_preconditions():
    import test_gpu_swiglu_exact as S
    S.test_the_shapes_cover_the_grid_walk()
    gu = S.operands("saturated", 5, 14336, 1)
    F = 14336
    g, u = gu[:, :F].float(), gu[:, F:].float()
    gbits = set(gu[:, :F].contiguous().view(torch.int16).flatten().tolist())
    assert len(gbits) == len(S.G_VALUES) == 10 and 0 in gbits and -32768 in gbits          # +0 and -0 among them
    assert set(g.unique().tolist()) >= {128.0, -128.0, 256.0, -256.0, 512.0, -512.0}
    for row in range(5):                                                                   # the integers of [-127, 127], scaled
        assert sorted((u[row, :255] / 2.0 ** (row % 7 - 3)).tolist()) == list(range(-127, 128))
    exp = S.saturated_expected(gu)
    eb = exp.contiguous().view(torch.int16)
    assert bool((eb == 0).any()) and bool((eb == -32768).any())                             # both zero signs
    p = torch.where(g <= -128, torch.tensor(-0.0), g).double() * u.double()
    assert bool((exp.double() != p).any()), "no exact product that needs a rounding"
    frac = p.float().view(torch.int32) & 0xFFFF
    assert bool((frac == 0x8000).any()), "no rounding tie"
    # the expectation is what the formula gives with an exponential that saturates as the contract says
    e = torch.where(g >= 128, torch.tensor(0.0), torch.where(g <= -128, torch.tensor(float("inf")), torch.tensor(1.0)))
    assert torch.equal(((g / (1.0 + e)) * u).to(BF).view(torch.int16), eb)
    assert 128 * S.LOG2E > 149 + 24                                                         # 2^-(128 log2 e) is below half the smallest subnormal
    gt = S.operands("true", 5, 14336, 2)
    ref = S.reference(gt)
    assert bool((ref.abs() >= 2.0 ** -126).all()) and bool((gt[:, :F].float().abs() <= 8).all())
    assert bool(torch.nn.functional.silu(torch.tensor(-float("inf"))).isnan())


def test_swiglu_emulation_is_inside_the_true_bound():
    import test_gpu_swiglu_exact as S
    gu = S.operands("true", 5, 14336, 3)
    ref = S.reference(gu)
    ratio = ((S.emulate(gu).double() - ref).abs() / (S.TRUE_BOUND * ref.abs())).max().item()
    print(f"swiglu emulation: max |out - ref| / bound = {ratio:.4f}")
    assert 0.5 < ratio <= 1.0, ratio
