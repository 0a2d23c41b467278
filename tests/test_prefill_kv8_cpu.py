"""The GPU-free part of the chunked-prefill attention over the FP8 paged-KV cache: the two prefill wrappers'
parameter lists, every rejection of loadgen.paged_prefill_attention_kv8 (before the native module is touched), the
throws of the native entry point (before any launch), the "prefill_kv8" op kind's cost model and the
LLM_KV8_PREFILL table written out literally, and the executor's row on the CPU device."""
import inspect

import pytest
import torch

from k8s_gpu_scheduler_amd import _native
from k8s_gpu_scheduler_amd.models import workloads as W
from k8s_gpu_scheduler_amd.ops import loadgen
from k8s_gpu_scheduler_amd.parallel import executor

BF, FP8, U8, I32 = torch.bfloat16, loadgen.FP8, torch.uint8, torch.int32


# ------------------------------------------------------------------------------------------------
# signatures
# ------------------------------------------------------------------------------------------------
def test_the_two_prefill_wrappers_parameter_lists():
    assert list(inspect.signature(loadgen.paged_prefill_attention_kv8).parameters) == [
        "q", "k_cache", "v_cache", "block_table", "ctx_lens", "q_start", "k_scale", "v_scale", "max_q_len", "out", "scale",
        "stream", "check"]
    assert list(inspect.signature(loadgen.paged_prefill_attention).parameters) == [
        "q", "k_cache", "v_cache", "block_table", "ctx_lens", "q_start", "max_q_len", "out", "scale", "stream", "check"]
    assert "k_scale" not in loadgen.paged_prefill_attention.__code__.co_varnames
    p = inspect.signature(loadgen.paged_prefill_attention_kv8).parameters
    assert all(p[n].default is None for n in ("k_scale", "v_scale", "max_q_len", "out", "scale", "stream")) and p["check"].default is True


# ------------------------------------------------------------------------------------------------
# host rejections: every one happens before the native module is asked for
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def host_operands_pass(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the native module was touched")
    monkeypatch.setattr(_native, "hip", boom)
    monkeypatch.setattr(loadgen, "_check_devices", lambda name, *ts: torch.device("cpu"))


def _prefill(S=2, Tq=3, Hq=4, Hkv=2, NB=3, MB=2, dtype=FP8):
    """(q, k_cache, v_cache, block_table, ctx_lens, q_start)."""
    def cache(*shape):
        return torch.zeros(shape, dtype=U8).view(FP8) if dtype == FP8 else torch.zeros(shape, dtype=dtype)
    q_start = torch.tensor(([0, 1, Tq] + [Tq] * S)[:S + 1], dtype=I32)
    return (torch.zeros(Tq, Hq, 128, dtype=BF), cache(NB, Hkv, 32, 128), cache(NB, Hkv, 128, 32), torch.zeros(S, MB, dtype=I32),
            torch.full((S,), 2, dtype=I32), q_start)


def SCALES(n=2):
    return torch.ones(n), torch.ones(n)


def KV8(*a, **kw):
    return loadgen.paged_prefill_attention_kv8(*a, **kw)


def test_bf16_caches_are_a_value_error_that_names_the_bf16_wrapper(host_operands_pass):
    ks, vs = SCALES()
    with pytest.raises(ValueError, match="paged_prefill_attention reads them"):
        KV8(*_prefill(dtype=BF), max_q_len=2)
    for kw in (dict(k_scale=ks, v_scale=vs), dict(k_scale=ks), dict(v_scale=vs)):
        with pytest.raises(ValueError, match="these are bf16"):
            KV8(*_prefill(dtype=BF), max_q_len=2, **kw)
    with pytest.raises(ValueError, match="these are bf16"):
        KV8(*_prefill(dtype=BF), ks, vs)                                            # positional scales


def test_mixed_and_other_cache_dtypes_are_type_errors(host_operands_pass):
    ks, vs = SCALES()
    q_, kc8, vc8, table, ctx, q_start = _prefill()
    _, kc16, vc16, _, _, _ = _prefill(dtype=BF)
    for kc, vc in ((kc8, vc16), (kc16, vc8)):
        with pytest.raises(TypeError, match="one cache dtype"):
            KV8(q_, kc, vc, table, ctx, q_start, k_scale=ks, v_scale=vs)
    for other in (torch.float16, torch.float32, U8, torch.float8_e5m2):
        _, kc, vc, _, _, _ = _prefill(dtype=other)
        for pair in ((kc, vc), (kc, vc8), (kc8, vc)):
            with pytest.raises(TypeError, match="bf16"):
                KV8(q_, *pair, table, ctx, q_start, k_scale=ks, v_scale=vs)
    with pytest.raises(TypeError, match="bf16"):                                     # q stays bf16
        KV8(q_.float(), kc8, vc8, table, ctx, q_start, k_scale=ks, v_scale=vs)
    with pytest.raises(TypeError, match="bf16"):                                     # the bf16 wrapper keeps rejecting FP8 caches
        loadgen.paged_prefill_attention(q_, kc8, vc8, table, ctx, q_start, max_q_len=2)
    with pytest.raises(TypeError):
        loadgen.paged_prefill_attention(q_, kc8, vc8, table, ctx, q_start, k_scale=ks, v_scale=vs)


def test_scales_missing_or_misshapen(host_operands_pass):
    ks, vs = SCALES()
    args = _prefill()
    for kw in ({}, dict(k_scale=ks), dict(v_scale=vs)):
        with pytest.raises(ValueError, match="need k_scale and v_scale"):
            KV8(*args, **kw)
    with pytest.raises(TypeError, match="fp32 k_scale"):
        KV8(*args, k_scale=ks.double(), v_scale=vs)
    with pytest.raises(TypeError, match="fp32 v_scale"):
        KV8(*args, k_scale=ks, v_scale=vs.to(BF))
    for bad in (torch.ones(3), torch.ones(1), torch.ones(2, 1), torch.ones(4)[::2], torch.tensor(1.0)):
        with pytest.raises(ValueError, match=r"contiguous \[2\] vector"):
            KV8(*args, k_scale=bad, v_scale=vs)
        with pytest.raises(ValueError, match=r"contiguous \[2\] vector"):
            KV8(*args, k_scale=ks, v_scale=bad)
    with pytest.raises(ValueError, match="on meta, the caches on cpu"):
        KV8(*args, k_scale=ks.to("meta"), v_scale=vs)
    with pytest.raises(ValueError, match="on meta, the caches on cpu"):
        KV8(*args, k_scale=ks, v_scale=vs.to("meta"))


def test_check_false_needs_max_q_len_and_its_range(host_operands_pass):
    ks, vs = SCALES()
    with pytest.raises(ValueError, match="check=False needs max_q_len"):
        KV8(*_prefill(), k_scale=ks, v_scale=vs, check=False)
    for bad in (-1, 2 ** 31):
        with pytest.raises(ValueError, match="max_q_len"):
            KV8(*_prefill(), k_scale=ks, v_scale=vs, max_q_len=bad)


def test_the_layout_group_and_stride_rules_hold_on_fp8_caches(host_operands_pass):
    """Every rule of _paged_attn_operands, on FP8 caches."""
    ks, vs = SCALES()
    q_, kc, vc, table, ctx, q_start = _prefill()

    def raises(exc, match, **kw):
        a = dict(q=q_, kc=kc, vc=vc, table=table, ctx=ctx, q_start=q_start, k_scale=ks, v_scale=vs)
        a.update(kw)
        with pytest.raises(exc, match=match):
            KV8(a["q"], a["kc"], a["vc"], a["table"], a["ctx"], a["q_start"], k_scale=a["k_scale"], v_scale=a["v_scale"],
                max_q_len=2, **{k: v for k, v in a.items() if k == "out"})

    def fp8(*shape):
        return torch.zeros(shape, dtype=U8).view(FP8)
    raises(TypeError, "int32 block_table and ctx_lens", table=table.long())
    raises(TypeError, "int32 block_table and ctx_lens", ctx=ctx.long())
    raises(TypeError, "int32 q_start", q_start=q_start.long())
    raises(ValueError, r"expects q \[Tq, Hq, 128\]", q=q_[0])
    raises(ValueError, r"expects q \[Tq, Hq, 128\]", kc=kc[0])
    raises(ValueError, r"expects q \[Tq, Hq, 128\]", table=table[0])
    raises(ValueError, "q_start must be 1-D", q_start=q_start.view(1, 3))
    raises(ValueError, "head dim must be 128", q=torch.zeros(3, 4, 64, dtype=BF))
    raises(ValueError, "head dim must be 128", kc=fp8(3, 2, 32, 64))
    raises(ValueError, "block size must be 32", kc=fp8(3, 2, 16, 128), vc=fp8(3, 2, 128, 16))
    raises(ValueError, "disagree on the blocks or the KV heads", vc=fp8(4, 2, 128, 32))
    raises(ValueError, "disagree on the blocks or the KV heads", vc=fp8(3, 1, 128, 32))
    raises(ValueError, "Hq / Hkv", q=torch.zeros(3, 6, 128, dtype=BF))
    raises(ValueError, "Hq / Hkv", q=torch.zeros(3, 3, 128, dtype=BF))
    raises(ValueError, "contiguous caches", kc=fp8(6, 2, 32, 128)[::2])
    raises(ValueError, "contiguous caches", vc=fp8(3, 2, 32, 128).transpose(2, 3))
    off = torch.zeros(3 * 2 * 32 * 128 + 16, dtype=U8)[8:-8].view(FP8)
    raises(ValueError, "caches must be 16-byte aligned", kc=off.view(3, 2, 32, 128))
    raises(ValueError, "do not match the 2 sequences of q_start", table=torch.zeros(3, 2, dtype=I32))
    raises(ValueError, "do not match the 2 sequences of q_start", ctx=torch.ones(3, dtype=I32))
    raises(ValueError, "contiguous block_table rows", table=torch.zeros(2, 4, dtype=I32)[:, ::2])
    raises(ValueError, "block_table row stride", table=torch.zeros(4, dtype=I32).as_strided((2, 2), (1, 1)))
    raises(ValueError, "contiguous ctx_lens", ctx=torch.ones(4, dtype=I32)[::2])
    raises(ValueError, "contiguous q_start", q_start=torch.zeros(6, dtype=I32)[::2])
    raises(ValueError, "bad output tensor", out=torch.zeros(3, 4, 64, dtype=BF))
    raises(ValueError, "bad output tensor", out=torch.zeros(3, 4, 128))
    raises(ValueError, r"contiguous \[Hq, 128\] slabs", q=torch.zeros(3, 4, 256, dtype=BF)[:, :, ::2])
    raises(ValueError, r"contiguous \[Hq, 128\] slabs", out=torch.zeros(3, 8, 128, dtype=BF)[:, ::2])
    raises(ValueError, "q token stride", q=torch.zeros(3, 4 * 128 + 4, dtype=BF)[:, :512].unflatten(1, (4, 128)))
    raises(ValueError, "out token stride", out=torch.zeros(3, 4 * 128 + 4, dtype=BF)[:, :512].unflatten(1, (4, 128)))
    raises(ValueError, "q must be 16-byte aligned", q=torch.zeros(3 * 512 + 8, dtype=BF)[4:-4].view(3, 4, 128))
    # a wider token stride and a wider table stride are accepted (and then the empty chunk list returns)
    wide = torch.zeros(3, 4 * 128 + 8, dtype=BF)[:, :512].unflatten(1, (4, 128))
    out = KV8(wide, kc, vc, torch.zeros(2, 5, dtype=I32)[:, :2], ctx, q_start, k_scale=ks, v_scale=vs, max_q_len=0)
    assert tuple(out.shape) == (3, 4, 128)


def test_empty_launches_return_without_the_native_module(host_operands_pass):
    ks, vs = SCALES()
    assert tuple(KV8(*_prefill(S=0), ks, vs).shape) == (3, 4, 128)                   # S == 0, positional scales
    assert tuple(KV8(*_prefill(Tq=0, S=1), k_scale=ks, v_scale=vs).shape) == (0, 4, 128)
    out = torch.full((3, 4, 128), 3.0, dtype=BF)
    assert KV8(*_prefill(), k_scale=ks, v_scale=vs, max_q_len=0, out=out, check=False) is out and bool((out == 3).all())


# ------------------------------------------------------------------------------------------------
# the native entry point: every throw precedes any launch
# ------------------------------------------------------------------------------------------------
def test_native_entry_point_throws_on_bad_operands():
    h = _native.hip(required=True)
    A = 4096                                                                         # an aligned non-null address: nothing launches

    def call(q=A, kc=A, vc=A, ks=A, vs=A, table=A, ctx=A, q_start=A, out=A, S=1, Hq=4, Hkv=2, mq=1, ld_q=512, ld_out=512, ld_t=1):
        h.paged_prefill_kv8(q, kc, vc, ks, vs, table, ctx, q_start, out, S, Hq, Hkv, mq, ld_q, ld_out, ld_t, 1.0, 0)
    for kw in (dict(Hq=6), dict(Hq=64, Hkv=2, ld_q=8192, ld_out=8192), dict(Hq=3, Hkv=2)):
        with pytest.raises(RuntimeError, match="paged_prefill_kv8: Hq / Hkv"):
            call(**kw)
    for kw in (dict(ld_q=504), dict(ld_out=504), dict(ld_q=516), dict(ld_out=516)):
        with pytest.raises(RuntimeError, match="token strides"):
            call(**kw)
    with pytest.raises(RuntimeError, match="negative block-table stride"):
        call(ld_t=-1)
    for kw in (dict(q=A + 8), dict(out=A + 8), dict(kc=A + 8), dict(vc=A + 8)):
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            call(**kw)
    for kw in (dict(table=A + 2), dict(ctx=A + 2), dict(q_start=A + 2), dict(ks=A + 2), dict(vs=A + 1)):
        with pytest.raises(RuntimeError, match="4-byte aligned"):
            call(**kw)
    for kw in (dict(ks=0), dict(vs=0)):
        with pytest.raises(RuntimeError, match="k_scale and v_scale are needed"):
            call(**kw)
    for kw in (dict(S=-1), dict(Hq=0), dict(Hkv=0), dict(Hkv=-2)):
        with pytest.raises(RuntimeError, match="negative or zero sizes"):
            call(**kw)
    with pytest.raises(RuntimeError, match="negative max_q_len"):
        call(mq=-1)
    # S == 0 or max_q_len == 0 launches nothing and needs no GPU
    call(S=0)
    call(mq=0)
    assert h.paged_prefill_workgroups(2, 32, 8, 1024) == 512


# ------------------------------------------------------------------------------------------------
# the cost model and the table
# ------------------------------------------------------------------------------------------------
def test_op_accounting_written_out():
    a = W.Op("prefill_kv8", 2, 32, 4096, rows=8, q=1024)
    assert a.flops == 4.0 * 128 * 2 * 32 * (1024 * 3072 + 1024 * 1025 / 2) == 120275861504.0
    assert a.bytes == 2 * 2 * 8 * 4096 * 128 + 4 * 2 * 1024 * 32 * 128 + 4 * 2 * 128 + 4 * 2 + 4 * 3 + 8 * 8 == 50332756
    assert a.workgroups(0) == a.workgroups(64) == 2 * 8 * 32 == 512
    b = W.Op("prefill_kv8", 64, 32, 8192, rows=8, q=32)
    assert b.flops == 4.0 * 128 * 64 * 32 * (32 * 8160 + 32 * 33 / 2) == 274357813248.0
    assert b.bytes == 2 * 64 * 8 * 8192 * 128 + 4 * 64 * 32 * 32 * 128 + 4 * 64 * 256 + 4 * 64 + 4 * 65 + 8 * 8 == 1107362372
    assert b.workgroups(0) == b.workgroups(64) == 64 * 8 * 1 == 512
    for o in (a, b):
        bf = W.Op("prefill", o.M, o.N, o.K, rows=o.rows, q=o.q)
        assert o.flops == bf.flops and o.workgroups(0) == bf.workgroups(0)
        assert o.bytes == bf.bytes - 2 * o.M * o.rows * o.K * 128 + 8 * o.rows
        assert o.on_mfma and not o.is_gemm and o.mfma_rate() == 1.0
    # the bf16 kind is unchanged
    assert W.Op("prefill", 2, 32, 4096, rows=8, q=1024).bytes == 4 * 2 * 8 * 4096 * 128 + 4 * 2 * 1024 * 32 * 128 + 4 * 2 * 128 + 4 * 2 + 4 * 3
    # flops per cache byte of the chunk shape: 256 in FP8, 128 in bf16
    assert round(b.flops / (2 * 64 * 8 * 8192 * 128), 1) == 255.5


def test_llm_kv8_prefill_table_written_out():
    lay = W.Workload("llm_kv8_layer_prefill_2048", "llm_kv8_layer_prefill", "hip", 2048,
                     (W.Op("gemm", 2048, 6144, 4096), W.Op("rope_append_kv8", 2, 32, 4096, rows=8, q=1024),
                      W.Op("prefill_kv8", 2, 32, 4096, rows=8, q=1024), W.Op("gemm", 2048, 4096, 4096)), 0.5)
    chk = W.Workload("llm_kv8_chunk_prefill_64", "llm_kv8_chunk_prefill", "hip", 64,
                     (W.Op("gemm", 2048, 6144, 4096), W.Op("rope_append_kv8", 64, 32, 8192, rows=8, q=32),
                      W.Op("prefill_kv8", 64, 32, 8192, rows=8, q=32), W.Op("gemm", 2048, 4096, 4096)), 2.25)
    assert W.LLM_KV8_PREFILL == {"llm_kv8_layer_prefill_2048": lay, "llm_kv8_chunk_prefill_64": chk}
    assert W._TABLES[-1] is W.LLM_KV8_PREFILL and W._TABLES[-2] is W.LLM_KV8 and len(W._TABLES) == 11
    assert len(W.LLM_KV8) == 2
    # llm_layer_prefill_2048 with the two kv8 kinds
    want = tuple(W.Op(o.kind + "_kv8", o.M, o.N, o.K, rows=o.rows, q=o.q) if o.kind in ("rope_append", "prefill") else o
                 for o in W.LLM_LAYER["llm_layer_prefill_2048"].ops)
    assert lay.ops == want
    for w in W.LLM_KV8_PREFILL.values():
        assert W.get(w.name) is w
        assert W.workload_for_pod(f"pod-{w.name.replace('_', '-')}-17") is w
        assert W.roofline_seconds(w, 1.0) > 0 and 0 < W.cu_fill(w) <= 1
        m, hb = W.roofline_split(w.name)
        assert m > 0 and hb > 0
        # the attention is on the MFMA side of the split, the append on the HBM side
        assert m == sum(o.flops for o in w.ops if o.kind != "rope_append_kv8") / 1e15
        assert hb == w.ops[1].bytes / 6e12


def _allocated_bytes(w: W.Workload) -> float:
    """What executor._Buffers allocates for the workload, from the operand layouts of its OP_KINDS rows."""
    total = 0.0
    for o in w.ops:
        if o.kind == "gemm":
            total += 2 * (o.M * o.K + o.N * o.K + o.M * o.N) + 4 * o.N
        elif o.kind in ("prefill_kv8", "rope_append_kv8"):
            rows = o.M * o.q
            total += 2 * o.M * o.K * o.rows * 128 + 2 * 2 * rows * o.N * 128 + 8 * o.rows        # 1-byte caches, q / out, scales
            total += 4 * o.M * o.K // 32 + 4 * o.M + 4 * (o.M + 1)                              # table, ctx, q_start
            if o.kind == "rope_append_kv8":
                total += 2 * rows * 2 * o.rows * 128 + 4 * 128 * o.K                            # the K / V part of qkv, cos_sin
        else:
            raise AssertionError(o)
    return total


def test_declared_footprints_follow_the_quarter_gib_rule():
    for w, cache_mib in ((W.LLM_KV8_PREFILL["llm_kv8_layer_prefill_2048"], 16), (W.LLM_KV8_PREFILL["llm_kv8_chunk_prefill_64"], 1024)):
        for o in w.ops:
            if o.kind.endswith("_kv8"):
                assert 2 * o.M * o.K * o.rows * 128 == cache_mib << 20                          # K + V of one op
        gib = _allocated_bytes(w) / 2 ** 30
        assert gib <= w.hbm_gib < gib + 0.25 and w.hbm_gib % 0.25 == 0, (w.name, gib)
    # the formula against what the executor really allocates, on the small workload
    w = W.LLM_KV8_PREFILL["llm_kv8_layer_prefill_2048"]
    bufs = executor._Buffers(w, torch.device("cpu"))
    assert sum(t.numel() * t.element_size() for _, ts in bufs.ops for t in ts if t is not None) == _allocated_bytes(w)


def test_new_names_change_no_existing_lookup():
    tables = (W.CATALOG, W.EXTRA, W.STAGED, W.LONG_CONTEXT, W.LLM_LAYER, W.LLM_BLOCK, W.LLM_HEAD, W.LLM_MOE, W.LLM_MX, W.LLM_KV8)
    assert tables == W._TABLES[:-1]
    old = [n for t in tables for n in t]
    for new in W.LLM_KV8_PREFILL:
        assert not any(o in new for o in old), new                      # an older name would win the lookup of a new pod
        assert not any(new in o for o in old), new
    assert not any(a != b and a in b for a in W.LLM_KV8_PREFILL for b in W.LLM_KV8_PREFILL)
    for t in tables:
        for n, w in t.items():
            assert W.workload_for_pod(f"x-{n.replace('_', '-')}-0").name in (n, W.workload_for_pod(n).name)
            assert W.get(n) is w


# ------------------------------------------------------------------------------------------------
# the executor's row
# ------------------------------------------------------------------------------------------------
def test_op_kinds_row_builds_operands_on_the_cpu():
    assert executor.OP_KINDS["prefill_kv8"][2] == 0
    assert {o.kind for w in W.LLM_KV8_PREFILL.values() for o in w.ops} <= set(executor.OP_KINDS)
    o = W.Op("prefill_kv8", 3, 4, 64, rows=2, q=5)
    w = W.Workload("prefill_kv8_row", "pin", "hip", 3, (o,), 0.1)
    cpu = torch.device("cpu")
    bufs, again = executor._Buffers(w, cpu), executor._Buffers(w, cpu)
    (o0, t), (_, u) = bufs.ops[0], again.ops[0]
    assert len(t) == 9
    out, q, kc, vc, table, ctx, q_start, ks, vs = t
    assert executor.op_output(o0, t) is out and out.dtype == q.dtype == BF and tuple(out.shape) == tuple(q.shape) == (15, 4, 128)
    assert kc.dtype == vc.dtype == FP8 and tuple(kc.shape) == (6, 2, 32, 128) and tuple(vc.shape) == (6, 2, 128, 32)
    assert table.dtype == ctx.dtype == q_start.dtype == I32
    assert torch.equal(q_start, torch.arange(4, dtype=I32) * 5) and ctx.tolist() == [64] * 3
    assert sorted(table.flatten().tolist()) == list(range(6))
    for c in (kc, vc):
        b = c.view(U8)
        assert int((b & 0x7F).max()) == 0x40 and int((b & 0x7F).min()) == 0 and len(b.unique()) > 100      # codes of [0, 0x41), any sign
        d = loadgen.dequantize_kv8_reference(c, 1.0)
        assert bool(d.isfinite().all()) and float(d.max()) == 2.0 and float(d.min()) == -2.0
    for s in (ks, vs):
        assert s.dtype == torch.float32 and tuple(s.shape) == (2,) and s.is_contiguous()
    assert ks.tolist() == [executor.KV8_K_SCALE] * 2 and vs.tolist() == [executor.KV8_V_SCALE] * 2
    assert all(torch.equal(a.view(U8) if a.dtype == FP8 else a, b.view(U8) if b.dtype == FP8 else b) for a, b in zip(t[1:], u[1:]))
    with pytest.raises(ValueError, match="longer than the context"):
        executor._Buffers(W.Workload("x", "pin", "hip", 1, (W.Op("prefill_kv8", 1, 4, 32, rows=2, q=33),), 0.1), cpu)

    calls = []
    saved = loadgen.paged_prefill_attention_kv8, loadgen.paged_prefill_attention

    def no_bf16_call(*a, **kw):
        raise AssertionError("the kv8 kind called the bf16 wrapper")
    loadgen.paged_prefill_attention_kv8 = lambda *a, **kw: calls.append((a, kw))
    loadgen.paged_prefill_attention = no_bf16_call
    try:
        executor.enqueue_ops(bufs, 1, "st", 64)
    finally:
        loadgen.paged_prefill_attention_kv8, loadgen.paged_prefill_attention = saved
    (a, kw), = calls
    assert len(a) == 8 and all(x is y for x, y in zip(a, (q, kc, vc, table, ctx, q_start, ks, vs)))
    assert kw == dict(max_q_len=5, out=out, stream="st", check=False)


def test_paged_kv8_operands_without_the_row_count_are_what_they_were():
    """The decode draw: same seed, every operand equal to a literal re-derivation of the order of draws."""
    o = W.Op("attn_kv8", 3, 4, 64, rows=2)
    cpu = torch.device("cpu")
    t = executor._paged_kv8_operands(o, torch.Generator().manual_seed(1234), cpu)
    g = torch.Generator().manual_seed(1234)
    q = torch.randn(3, 4, 128, generator=g).to(BF)

    def cache(*shape):
        lo = torch.randint(0, 0x41, (6,) + shape, generator=g)
        return (lo | (torch.randint(0, 2, (6,) + shape, generator=g) << 7)).to(U8)
    kc, vc = cache(2, 32, 128), cache(2, 128, 32)
    table = torch.randperm(6, generator=g).to(I32).view(3, 2)
    assert len(t) == 8
    assert torch.equal(t[1], q) and torch.equal(t[2].view(U8), kc) and torch.equal(t[3].view(U8), vc) and torch.equal(t[4], table)
    assert t[5].tolist() == [64] * 3 and tuple(t[0].shape) == (3, 4, 128) and t[0].dtype == BF
    assert t[6].tolist() == [0.5, 0.5] and t[7].tolist() == [0.25, 0.25]
    # the new argument changes the rows of q and out and nothing of the draw order
    t5 = executor._paged_kv8_operands(o, torch.Generator().manual_seed(1234), cpu, 15)
    assert tuple(t5[0].shape) == tuple(t5[1].shape) == (15, 4, 128) and torch.equal(t5[1][:0], q[:0])
    assert torch.equal(executor._paged_kv8_operands(o, torch.Generator().manual_seed(1234), cpu, 3)[2].view(U8), kc)
