"""The embedding-bag gather without a GPU: the workload model's gather op and the dlrm_2048
workload, the pure-Python grid rule, the host wrapper's validation (which must fire before the
native module is touched), the profiler's kernel classification and the executor's op dispatch.
The kernel itself is pinned on the GPU by test_gpu_gather_exact.py."""
import math

import pytest
import torch

from k8s_gpu_scheduler_amd import _native
from k8s_gpu_scheduler_amd.models import workloads as W
from k8s_gpu_scheduler_amd.ops import loadgen


# ------------------------------------------------------------------------------------------------
# workload model
# ------------------------------------------------------------------------------------------------
def test_gather_op_bytes_flops():
    o = W.Op("gather", M=8, N=64, K=3, rows=100)
    assert not o.is_gemm
    assert o.flops == 8 * 3 * 64
    assert o.bytes == 2 * 8 * 3 * 64 + 4 * 8 * 3 + 4 * (8 + 1) + 2 * 8 * 64
    assert o.rows == 100 and W.Op("triad", n_floats=4).rows == 0


def _old_flops(o):
    return 2.0 * o.M * o.N * o.K if o.kind in ("gemm", "gemm8") else 2.0 * o.n_floats


def _old_bytes(o):
    if o.kind == "gemm":
        return 2.0 * (o.M * o.K + o.N * o.K + o.M * o.N)
    if o.kind == "gemm8":
        return 1.0 * (o.M * o.K + o.N * o.K) + 2.0 * o.M * o.N
    return 12.0 * o.n_floats


def _old_roofline(w, share, peak_tflops=1100.0, hbm_tbps=5.5, share_bw_exp=0.6):
    t = 0.0
    for o in w.ops:
        mem = _old_bytes(o) / (hbm_tbps * 1e12 * share ** share_bw_exp)
        if o.kind in ("gemm", "gemm8"):
            rate = 2.0 if o.kind == "gemm8" else 1.0
            t += max(_old_flops(o) / (peak_tflops * rate * 1e12 * share), mem)
        else:
            t += mem
    return t


def _old_cu_fill(w, cu_budget=W.POD_CU_BUDGET):
    t = f = 0.0
    for o in w.ops:
        dt = _old_roofline(W.Workload(w.name, w.family, w.framework, w.batch, (o,), 0.0), 1.0)
        if o.kind in ("gemm", "gemm8"):
            fo = min(1.0, W.default_gemm_workgroups(o.M, o.N, o.K, cu_budget, o.kind == "gemm8") / W.CUS)
        else:
            fo = 1.0
        t += dt
        f += dt * fo
    return f / t


def test_existing_workloads_keep_their_values_bit_for_bit():
    """Expected values from the formulas as they stood before the gather op (copied above)."""
    assert len(W.CATALOG) == 18
    for w in W.CATALOG.values():
        assert all(o.kind in ("gemm", "triad") for o in w.ops)
        assert w.flops == sum(_old_flops(o) for o in w.ops)
        assert w.bytes == sum(_old_bytes(o) for o in w.ops)
        for share in (1.0, 0.5, 0.25, 0.125):
            assert W.roofline_seconds(w, share) == _old_roofline(w, share)
    for name in ("fp8_llm_2048", "triad_only_2048"):
        w = W.EXTRA[name]
        assert w.flops == sum(_old_flops(o) for o in w.ops) and w.bytes == sum(_old_bytes(o) for o in w.ops)
        for budget in (W.POD_CU_BUDGET, 0, 128):
            assert W.cu_fill(w, budget) == _old_cu_fill(w, budget)


def test_dlrm_workload():
    w = W.get("dlrm_2048")
    assert W.workload_for_pod("dlrm-2048-abc") is w
    assert (w.family, w.framework, w.batch) == ("dlrm", "hip", 2048)
    g, *gemms = w.ops
    assert g.kind == "gather" and (g.M, g.N, g.K, g.rows) == (2048 * 26, 128, 32, 4194304)
    assert g.rows * g.N * 2 >= 1 << 30 and w.hbm_gib * (1 << 30) >= g.rows * g.N * 2
    assert [(o.kind, o.M, o.N, o.K) for o in gemms] == [("gemm", 2048, 1024, 3328), ("gemm", 2048, 1024, 1024)]
    assert all(d % 64 == 0 for o in gemms for d in (o.M, o.N, o.K))
    t = W.roofline_seconds(w, 1.0)
    assert math.isfinite(t) and t > 0
    assert t == pytest.approx(g.bytes / 5.5e12 + sum(max(o.flops / 1100e12, o.bytes / 5.5e12) for o in gemms))
    m, h = W.roofline_split("dlrm-2048-abc", tflops=1.0e3, tbps=6.0)
    assert h == pytest.approx(g.bytes / 6.0e12) and m == pytest.approx(sum(o.flops for o in gemms) / 1.0e15)
    f = W.cu_fill(w)
    assert 0.0 < f <= 1.0


def test_gather_cu_fill_counts_workgroups():
    one = W.Workload("g", "dlrm", "hip", 1, (W.Op("gather", 512, 128, 32, rows=1024),), 0.0)
    assert W.cu_fill(one) == pytest.approx(128 / W.CUS)             # 512 bags = 128 workgroups of 4
    assert W.cu_fill(W.Workload("g", "dlrm", "hip", 1, (W.Op("gather", 4096, 128, 32, rows=1024),), 0.0)) == 1.0


def test_default_gather_workgroups():
    assert [W.default_gather_workgroups(b) for b in (1, 4, 5)] == [1, 1, 2]
    assert W.default_gather_workgroups(53248) == 13312
    assert W.default_gather_workgroups(37, 3) == 3 and W.default_gather_workgroups(5, 8) == 2


@pytest.mark.skipif(_native.hip(required=False) is None, reason="HIP extension not built")
def test_default_gather_workgroups_match_the_native_rule():
    h = _native.hip()
    for b in (1, 3, 4, 5, 9, 37, 53248, 2 ** 31 - 1):
        for blocks in (0, 1, 2, 3, 8192):
            assert h.embedding_bag_workgroups(b, blocks) == W.default_gather_workgroups(b, blocks), (b, blocks)


# ------------------------------------------------------------------------------------------------
# host wrapper: every rejection happens before the native module is asked for
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def no_native(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the native module was touched")
    monkeypatch.setattr(_native, "hip", boom)


def _operands(R=16, D=64, B=2, P=3):
    table = torch.zeros(R, D, dtype=torch.bfloat16)
    idx = torch.zeros(B * P, dtype=torch.int32)
    offsets = torch.arange(B + 1, dtype=torch.int32) * P
    return table, idx, offsets


def test_wrapper_rejects_cpu_tensors(no_native):
    table, idx, offsets = _operands()
    with pytest.raises(ValueError, match="device tensors"):
        loadgen.embedding_bag(table, idx, offsets)
    with pytest.raises(ValueError, match="device tensors"):          # before any dtype complaint
        loadgen.embedding_bag(table.float(), idx.long(), offsets)


@pytest.fixture
def host_operands_pass(monkeypatch, no_native):
    """The remaining checks need tensors that pass the device check; without a GPU the check is
    stubbed out, and everything after it up to the native call runs on host tensors."""
    monkeypatch.setattr(loadgen, "_check_devices", lambda name, *ts: torch.device("cpu"))


def test_wrapper_rejects_dtypes(host_operands_pass):
    table, idx, offsets = _operands()
    with pytest.raises(TypeError, match="bf16"):
        loadgen.embedding_bag(table.float(), idx, offsets)
    with pytest.raises(TypeError, match="bf16"):
        loadgen.embedding_bag(table.half(), idx, offsets)
    with pytest.raises(TypeError, match="int32"):
        loadgen.embedding_bag(table, idx.long(), offsets)
    with pytest.raises(TypeError, match="int32"):
        loadgen.embedding_bag(table, idx, offsets.long())


@pytest.mark.parametrize("D", [96, 4096, 32, 8])
def test_wrapper_rejects_row_lengths(host_operands_pass, D):
    table, idx, offsets = _operands(D=D)
    with pytest.raises(ValueError, match="power of two"):
        loadgen.embedding_bag(table, idx, offsets)


def test_wrapper_rejects_strides_and_layouts(host_operands_pass):
    table, idx, offsets = _operands()
    narrow = torch.zeros(16, 68, dtype=torch.bfloat16)[:, :64]         # row stride 68
    with pytest.raises(ValueError, match="multiple of 8"):
        loadgen.embedding_bag(narrow, idx, offsets)
    with pytest.raises(ValueError, match="contiguous"):
        loadgen.embedding_bag(torch.zeros(64, 16, dtype=torch.bfloat16).T, idx, offsets)
    out = torch.zeros(2, 68, dtype=torch.bfloat16)[:, :64]
    with pytest.raises(ValueError, match="multiple of 8"):
        loadgen.embedding_bag(table, idx, offsets, out=out)
    with pytest.raises(ValueError, match="bad output"):
        loadgen.embedding_bag(table, idx, offsets, out=torch.zeros(3, 64, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="16-byte"):
        loadgen.embedding_bag(torch.zeros(16 * 64 + 8, dtype=torch.bfloat16)[4:4 + 16 * 64].view(16, 64), idx, offsets)


def test_wrapper_rejects_index_forms(host_operands_pass):
    table, idx, offsets = _operands()
    with pytest.raises(ValueError, match="no offsets"):
        loadgen.embedding_bag(table, idx.view(2, 3), offsets)
    with pytest.raises(ValueError, match="needs offsets"):
        loadgen.embedding_bag(table, idx)
    with pytest.raises(ValueError, match="1-D or 2-D"):
        loadgen.embedding_bag(table, idx.view(1, 2, 3))
    with pytest.raises(ValueError, match="contiguous"):
        loadgen.embedding_bag(table, torch.zeros(12, dtype=torch.int32)[::2], offsets)


# ------------------------------------------------------------------------------------------------
# profiler and executor
# ------------------------------------------------------------------------------------------------
def test_gather_kernel_is_not_an_mfma_kernel():
    from k8s_gpu_scheduler_amd.agent import pod_profiler
    for name in ("embedding_bag_kernel",
                 "void gs::(anonymous namespace)::embedding_bag_kernel<128>(__bf16 const*, int const*, int const*, "
                 "__bf16*, int, unsigned long, unsigned long)",
                 "_ZN2gs12_GLOBAL__N_120embedding_bag_kernelILi128EEEvPKDF16bPKiS5_PDF16bimm"):
        assert not pod_profiler.is_mfma_kernel(name), name
    assert pod_profiler.is_mfma_kernel("gemm_bf16_kernel")


def test_enqueue_ops_raises_on_an_unknown_kind():
    from k8s_gpu_scheduler_amd.parallel import executor

    class Stub:
        ops = [(W.Op("scatter"), ())]

    with pytest.raises(ValueError, match="scatter"):
        executor.enqueue_ops(Stub(), 1, None, 0)
