"""CPU-only tests of the helpers of test_gpu_corun_exact.py: the overlap predicate, the aggressor
sizing and its cap, the derived GEMM bound (an honest fp32 product in any order stays inside it, a
dropped K chunk or a shifted bias does not), the representable cap of every shape the module runs,
and that its two tiny workloads register and leave through monkeypatch."""
import zlib

import pytest
import torch

import test_gpu_corun_exact as C
import test_gpu_kernels_exact as X


def test_overlap_predicate():
    assert C.victim_inside(0.0, 10.0, 2.0, 8.0)                 # contained
    assert C.victim_inside(0.0, 10.0, 0.0, 10.0)                # contained, sharing both ends
    assert not C.victim_inside(0.0, 10.0, 10.0, 12.0)           # touching: starts as the aggressor ends
    assert not C.victim_inside(5.0, 10.0, 2.0, 5.0)             # touching: ends as the aggressor starts
    assert not C.victim_inside(0.0, 10.0, 11.0, 12.0)           # disjoint, after
    assert not C.victim_inside(5.0, 10.0, 1.0, 2.0)             # disjoint, before
    assert not C.victim_inside(2.0, 8.0, 0.0, 10.0)             # reversed: the aggressor inside the victim
    assert not C.victim_inside(0.0, 10.0, 2.0, 11.0)            # the victim outlasts the aggressor
    assert not C.victim_inside(0.0, 10.0, -1.0, 5.0)            # the victim starts first
    assert not C.victim_inside(0.0, 10.0, 8.0, 2.0)             # reversed victim interval
    assert not C.victim_inside(0.0, 10.0, 4.0, 4.0)             # an empty victim interval proves nothing
    assert not C.victim_inside(0.0, 10.0, float("nan"), 5.0)


def test_aggressor_sizing_and_cap():
    assert C.aggressor_passes(1.0e-3, 1.0e-3) == 6              # 4 victim times and 2 passes
    assert C.aggressor_passes(1.0e-3, 3.0e-3) == 4              # ceil(4 / 3) + 2
    assert C.aggressor_passes(1.0e-4, 1.0) == 3                 # never fewer than 3
    assert C.aggressor_passes(510 * 0.25e-3, 1.0e-3) == 512     # the cap itself is allowed
    with pytest.raises(AssertionError, match=r"cap 512.*127\.750 ms.*1\.0000 ms"):
        C.aggressor_passes(511 * 0.25e-3, 1.0e-3)
    with pytest.raises(AssertionError):
        C.aggressor_passes(1.0e-3, 0.0)
    assert C.aggressor_passes(1.0, 1.0, cap=6) == 6


def test_gate_sizing():
    # each 72 us pass that takes 8 us to enqueue buys 64 us; twice 3 ms of hold (93.75 passes), and two more
    assert C.gate_passes(3.0e-3, 72e-6, 8e-6) == 96
    with pytest.raises(AssertionError, match="gate pass"):
        C.gate_passes(3.0e-3, 20e-6, 16e-6)
    with pytest.raises(AssertionError, match="cap"):
        C.gate_passes(1.0, 70e-6, 10e-6)


def t_mix_gemm():
    """(op, a, bt) of the t_mix workload's first GEMM as the executor's _Buffers makes them, and a
    bias of this test's own (the executor's is zero, which no shift would change)."""
    from k8s_gpu_scheduler_amd.parallel.executor import _gemm_operands
    w = C.tiny_workloads()[0]
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(w.name.encode()) & 0xFFFF)
    o = w.ops[0]
    a, bt, zero, _ = _gemm_operands(o, g, torch.device("cpu"))
    assert o.kind == "gemm" and a.shape == (o.M, o.K) and bt.shape == (o.N, o.K) and not zero.any()
    bias = 1.0 + torch.randn(o.N, generator=torch.Generator().manual_seed(5))
    return o, a.float(), bt.float(), bias


def fp32_product(a, bt, bias, chunks, shift=0):
    """bf16(relu(sum over the K chunks, in the order given, in fp32 + bias)); shift rolls the bias."""
    acc = torch.zeros(a.shape[0], bt.shape[0])
    for c in chunks:
        acc += a[:, c] @ bt[:, c].T
    return (acc + bias.roll(shift)).clamp_min(0.0).to(torch.bfloat16)


def test_gemm_bound_admits_any_summation_order_and_catches_a_dropped_chunk_or_a_shifted_bias():
    o, a, bt, bias = t_mix_gemm()
    ref, bound = C.gemm_bound(a, bt, bias)
    assert ref.dtype == torch.float64 and bool((bound > 0).all())
    perm = torch.randperm(o.K, generator=torch.Generator().manual_seed(9))
    for width in (1, 8, 64):                                       # element by element, and in blocks
        out = fp32_product(a, bt, bias, perm.split(width))
        err = (out.double() - ref).abs()
        assert bool((err <= bound).all()), (width, (err / bound).max().item())
    in_order = list(torch.arange(o.K).split(64))
    assert len(in_order) == 5
    dropped = fp32_product(a, bt, bias, in_order[:2] + in_order[3:])
    bad = ((dropped.double() - ref).abs() > bound).double().mean().item()
    assert bad > 0.5, bad
    shifted = fp32_product(a, bt, bias, in_order, shift=1)
    bad = ((shifted.double() - ref).abs() > bound).double().mean().item()
    assert bad > 0.5, bad
    hole = fp32_product(a, bt, bias, in_order)
    hole[3, 5] = float("nan")                                      # an unwritten element
    assert not bool(((hole.double() - ref).abs() <= bound).all())


def test_gemm_bound_zero_bias_is_the_executors_case():
    o, a, bt, _ = t_mix_gemm()
    zero = torch.zeros(o.N)
    ref, bound = C.gemm_bound(a, bt, zero)
    out = fp32_product(a, bt, zero, list(torch.arange(o.K).split(32)))
    assert bool(((out.double() - ref).abs() <= bound).all())
    dropped = fp32_product(a, bt, zero, list(torch.arange(o.K).split(64))[1:])
    # with a zero bias the ReLU makes half of both products 0: where the reference is not, the chunk shows
    assert ((dropped.double() - ref).abs() > bound)[ref > 0].double().mean().item() > 0.9


def test_representable_cap_holds_for_every_victim_shape():
    shapes = C.victim_shapes()
    assert len(shapes) > 20 and C.MFMA_SHAPE + (False,) in shapes
    for M, N, K, fp8 in shapes:
        a, bt, bias = X.build_operands(M, N, K, "rep", fp8)
        cap = (X.reference(a, bt) + bias.double()).abs().max().item()
        assert cap <= X.REP_CAP, (M, N, K, fp8, cap)


def test_workloads_register_and_leave(monkeypatch):
    from k8s_gpu_scheduler_amd.models import workloads as W
    before = dict(W.EXTRA)
    with monkeypatch.context() as m:
        for w in C.tiny_workloads():
            m.setitem(W.EXTRA, w.name, w)
        assert W.get("t_mix").ops[1].kind == "triad" and W.get("t_idx").ops[0].rows == 5000
        assert W.get("t_idx").ops[1].workgroups(64) == 10 and W.get("t_mix").ops[0].workgroups(64) is not None
        assert len(W.EXTRA) == len(before) + 2
    assert W.EXTRA == before
    with pytest.raises(KeyError):
        W.get("t_mix")


def test_tiny_workloads_take_the_repeat_tails():
    from k8s_gpu_scheduler_amd.parallel import executor as E
    _, idx = C.tiny_workloads()
    gather, attn = idx.ops
    assert gather.rows > E.GATHER_BLOCK_ROWS and gather.rows % E.GATHER_BLOCK_ROWS
    blocks = attn.M * attn.K // 32
    assert blocks == 75 and blocks > E.ATTN_PATTERN_BLOCKS and blocks % E.ATTN_PATTERN_BLOCKS
