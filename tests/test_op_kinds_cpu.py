"""The executor's table of op kinds (parallel.executor.OP_KINDS) -- no GPU: the operands it builds
are pinned across commits, its launches are recorded through stubbed loadgen entry points, and it
is complete for every workload the project defines."""
import zlib

import pytest
import torch

from k8s_gpu_scheduler_amd.models import workloads as W
from k8s_gpu_scheduler_amd.ops import loadgen
from k8s_gpu_scheduler_amd.parallel import executor

KINDS = ("gemm", "gemm8", "triad", "gather", "attn")

# the smallest ops that reach every branch of the operand code: a table longer than
# GATHER_BLOCK_ROWS and no multiple of it, a cache of 75 blocks (more than ATTN_PATTERN_BLOCKS, no
# multiple of it) and one of 6 (fewer), a trailing GEMM that sees the generator state every other
# kind left behind
PIN_OPS = (W.Op("gemm", 64, 128, 64), W.Op("gemm8", 64, 64, 128), W.Op("triad", n_floats=1024),
           W.Op("gather", 6, 64, 3, rows=5000), W.Op("attn", 5, 4, 480, rows=2), W.Op("attn", 3, 2, 64, rows=1),
           W.Op("gemm", 64, 64, 64))

# (position in the operand tuple, shape, dtype, CRC-32 of the bytes) of every operand that is not
# torch.empty, per op of PIN_OPS -- recorded with fingerprint() below at the commit before the
# table existed (_Buffers' per-kind ladder)
PINNED = (
    ((0, (64, 64), "bfloat16", 0x78065EAA), (1, (128, 64), "bfloat16", 0x6F923058),
     (2, (128,), "float32", 0xB2AA7578)),
    ((0, (64, 128), "float8_e4m3fn", 0x5C97F42D), (1, (64, 128), "float8_e4m3fn", 0x7F7EF5F9),
     (2, (64,), "float32", 0x0D968558)),
    ((0, (1024,), "float32", 0x69A164BC), (1, (1024,), "float32", 0x69A164BC), (2, (1024,), "float32", 0x69A164BC)),
    ((1, (5000, 64), "bfloat16", 0x54B9A3D6), (2, (18,), "int32", 0xF80531A6), (3, (7,), "int32", 0xA70C8DF3)),
    ((1, (5, 4, 128), "bfloat16", 0x65DCFAAE), (2, (75, 2, 32, 128), "bfloat16", 0xC8168F49),
     (3, (75, 2, 128, 32), "bfloat16", 0x1C5249F0), (4, (5, 15), "int32", 0x4EDE6FEE),
     (5, (5,), "int32", 0x3B84C98D)),
    ((1, (3, 2, 128), "bfloat16", 0x289849B4), (2, (6, 1, 32, 128), "bfloat16", 0x81A0602A),
     (3, (6, 1, 128, 32), "bfloat16", 0xE8870AA6), (4, (3, 2), "int32", 0x8C90153D),
     (5, (3,), "int32", 0xF93FEB4F)),
    ((0, (64, 64), "bfloat16", 0x4274207C), (1, (64, 64), "bfloat16", 0x93E49C56), (2, (64,), "float32", 0x0D968558)),
)


def fingerprint(o: W.Op, t: tuple) -> tuple:
    """PINNED's row for one op: every operand but a torch.empty output (the triad's x is written
    by the kernel too, but starts as ones)."""
    skip = None if o.kind == "triad" else (3 if o.is_gemm else 0)
    return tuple((i, tuple(x.shape), str(x.dtype).replace("torch.", ""),
                  zlib.crc32(x.contiguous().view(torch.uint8).numpy().tobytes()))
                 for i, x in enumerate(t) if i != skip)


def test_operands_are_the_ones_the_per_kind_ladder_built():
    w = W.Workload("pin_operands", "pin", "hip", 64, PIN_OPS, 0.1)
    assert executor.GATHER_BLOCK_ROWS == 4096 and executor.ATTN_PATTERN_BLOCKS == 64      # what PIN_OPS straddles
    bufs = executor._Buffers(w, torch.device("cpu"))
    assert [o for o, _ in bufs.ops] == list(PIN_OPS)
    lengths = {"gemm": 4, "gemm8": 4, "triad": 3, "gather": 4, "attn": 6}
    for (o, t), want in zip(bufs.ops, PINNED):
        assert len(t) == lengths[o.kind], o
        got = fingerprint(o, t)
        for g, e in zip(got, want):
            assert g == e, (o, g, tuple(e[:3]) + (hex(e[3]),))
        assert len(got) == len(want), o
        out = t[3] if o.is_gemm else t[0]
        assert out.dtype == (torch.float32 if o.kind == "triad" else torch.bfloat16)
        assert tuple(out.shape) == {"gemm": (o.M, o.N), "gemm8": (o.M, o.N), "triad": (o.n_floats,),
                                    "gather": (o.M, o.N), "attn": (o.M, o.N, 128)}[o.kind]


def test_buffers_name_the_workload_in_their_errors():
    with pytest.raises(ValueError, match=r"workload odd: unknown op kind 'scatter'"):
        executor._Buffers(W.Workload("odd", "pin", "hip", 1, (W.Op("scatter"),), 0.1), torch.device("cpu"))
    with pytest.raises(ValueError, match=r"workload odd: attention context 48 is no multiple of 32"):
        executor._Buffers(W.Workload("odd", "pin", "hip", 1, (W.Op("attn", 1, 1, 48, rows=1),), 0.1),
                          torch.device("cpu"))


# the one loadgen call of each kind: (entry point, operand tuple, positional arguments, keywords)
# for enqueue_ops(stub, 2, "stream", 64, blocks=7)
LAUNCHES = {
    "gemm": ("gemm", ("a", "bt", "bias", "c"), ("a", "bt"),
             {"out": "c", "bias": "bias", "relu": False, "stream": "stream", "cu_budget": 64}),
    "gemm8": ("gemm_fp8", ("a", "bt", "bias", "c"), ("a", "bt"),
              {"out": "c", "bias": "bias", "relu": False, "stream": "stream", "cu_budget": 64}),
    "gather": ("embedding_bag", ("out", "table", "idx", "offsets"), ("table", "idx", "offsets"),
               {"out": "out", "stream": "stream", "check_indices": False}),
    "attn": ("paged_decode_attention", ("out", "q", "kc", "vc", "table", "ctx"), ("q", "kc", "vc", "table", "ctx"),
             {"out": "out", "stream": "stream", "check": False}),
    "triad": ("triad", ("x", "y", "z"), ("x", "y", "z", 1.0001), {"blocks": 7, "stream": "stream"}),
}
ENTRY_POINTS = ("gemm", "gemm_fp8", "triad", "embedding_bag", "paged_decode_attention")


def test_launch_table_covers_the_kinds():
    assert set(LAUNCHES) == set(KINDS) and {v[0] for v in LAUNCHES.values()} == set(ENTRY_POINTS)


@pytest.fixture
def recorded(monkeypatch):
    calls = []
    for name in ENTRY_POINTS:
        monkeypatch.setattr(loadgen, name, lambda *a, _n=name, **k: calls.append((_n, a, k)))
    return calls


@pytest.mark.parametrize("kind", KINDS)
def test_enqueue_ops_makes_the_one_call_of_each_kind(recorded, kind):
    entry, operands, args, kwargs = LAUNCHES[kind]
    # a sibling op in front: the calls come in op order, each with its own operands and relu
    first = W.Op("gemm", relu=True)

    class Stub:
        ops = [(first, ("a0", "bt0", "bias0", "c0")), (W.Op(kind, relu=False), operands)]

    executor.enqueue_ops(Stub(), 2, "stream", 64, blocks=7)
    lead = ("gemm", ("a0", "bt0"), {"out": "c0", "bias": "bias0", "relu": True, "stream": "stream", "cu_budget": 64})
    assert recorded == [lead, (entry, args, kwargs)] * 2


def test_enqueue_op_is_one_launch_and_blocks_default_to_the_kernels_choice(recorded):
    executor.enqueue_op(W.Op("triad"), ("x", "y", "z"), "stream", 0)
    assert recorded == [("triad", ("x", "y", "z", 1.0001), {"blocks": 0, "stream": "stream"})]
    with pytest.raises(ValueError, match="scatter"):
        executor.enqueue_op(W.Op("scatter"), (), None, 0)
    assert len(recorded) == 1


def _all_ops():
    return [(w.name, o) for table in (W.CATALOG, W.EXTRA) for w in table.values() for o in w.ops]


def test_every_workload_kind_is_in_the_table():
    used = {o.kind for _, o in _all_ops()}
    assert used == set(KINDS)                             # a new kind has to be added to this file's tables too
    assert used <= set(executor.OP_KINDS)
    t = ("t0", "t1", "t2", "t3", "t4", "t5")
    for kind in KINDS:
        assert executor.op_output(W.Op(kind), t) == ("t3" if kind in ("gemm", "gemm8") else "t0"), kind
    with pytest.raises(ValueError, match="scatter"):
        executor.op_output(W.Op("scatter"), t)


@pytest.mark.parametrize("budget", [64, 0, 128])
def test_op_workgroups_are_the_default_launch_grids(budget):
    for name, o in _all_ops():
        wg = o.workgroups(budget)
        if o.kind == "gemm":
            want = W.default_gemm_workgroups(o.M, o.N, o.K, budget, False)
        elif o.kind == "gemm8":
            want = W.default_gemm_workgroups(o.M, o.N, o.K, budget, True)
        elif o.kind == "gather":
            want = W.default_gather_workgroups(o.M)
        elif o.kind == "attn":
            want = W.default_attn_workgroups(o.M, o.rows)
        else:
            want = None
        assert wg == want and (wg is None) == (o.kind == "triad"), (name, o, budget)
