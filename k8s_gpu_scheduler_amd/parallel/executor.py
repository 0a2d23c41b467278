"""Per-GPU pod executor ("kubelet + container runtime" of the bench and e2e tests).

One process per GPU.  The executor receives the scheduler's placements for its device
(pod id, workload, CU-slice unit range, iterations), runs each pod's kernel mix on a HIP
stream whose CU mask is exactly the pod's CU slices (ops.cumask.MaskedStream), and measures
per-pod device time with HIP events.  Pods are ordered on the device per CU-slice unit
(a pod waits for the previous occupant of each of its units), so the scheduler's
capacity model (a unit is free when its previous pod finishes) holds without host
synchronisation: the host can schedule epoch t+1 while the GPU executes epoch t.

Working buffers are allocated once per (workload, slot) and reused -- a warm container.
"""
from __future__ import annotations

import os
import time
import zlib
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from ..models.workloads import Op, Workload, get as workload_by_name
from ..ops import loadgen
from ..plugins.gpu.devices import CUS_PER_XCD as CUS_PER_UNIT, cu_slice_mask


@dataclass
class PodRun:
    pod_id: int
    workload: str
    first_unit: int
    n_units: int
    iters: int
    slo: float = 0.0
    masked: bool = True          # Guaranteed QoS: hard CU mask; Burstable: accounted share only
    start: Optional[torch.cuda.Event] = None
    end: Optional[torch.cuda.Event] = None
    ms: float = 0.0
    gpu: int = 0                 # the node's GPU index (simulated executors keep one pipeline per GPU)
    policy: int = 0              # kernel policy from the scheduler: 1 = wide GEMM tiles (whole-chip budget)

    @property
    def throughput(self) -> float:
        return self.iters / (self.ms / 1e3) if self.ms > 0 else 0.0


GATHER_BLOCK_ROWS = 4096          # rows of the CPU-generated block a gather table repeats
ATTN_PATTERN_BLOCKS = 64          # KV-cache blocks of the CPU-generated pattern an attention cache repeats


def _repeat(pattern: torch.Tensor, n: int) -> torch.Tensor:
    """n entries that cycle through `pattern`'s (along dim 0): one small CPU-generated block
    repeated on the device, so a GiB operand never exists on the host."""
    out = torch.empty((n,) + pattern.shape[1:], dtype=pattern.dtype, device=pattern.device)
    full = n - n % len(pattern)
    out[:full].view(-1, *pattern.shape).copy_(pattern)
    out[full:].copy_(pattern[:n - full])
    return out


def _gemm_operands(o: Op, g: torch.Generator, device: torch.device) -> tuple:
    a = ((torch.rand(o.M, o.K, generator=g) * 2 - 1).to(torch.bfloat16)).to(device)
    bt = ((torch.rand(o.N, o.K, generator=g) * 2 - 1).to(torch.bfloat16) * 0.05).to(device)
    if o.kind == "gemm8":                   # e4m3 operands (weights scaled into range)
        a, bt = a.to(loadgen.FP8), (bt * 16).to(loadgen.FP8)
    bias = torch.zeros(o.N, dtype=torch.float32, device=device)
    c = torch.empty(o.M, o.N, dtype=torch.bfloat16, device=device)
    return a, bt, bias, c


def _gather_operands(o: Op, g: torch.Generator, device: torch.device) -> tuple:
    """M bags of K rows of N elements out of a table of o.rows rows.  The table repeats one block
    of values k / 128, |k| <= 127: every fp32 partial sum of a bag is exact, so the output does
    not depend on the kernel's summation order."""
    n = min(o.rows, GATHER_BLOCK_ROWS)
    blk = ((torch.randint(-127, 128, (n, o.N), generator=g).float() / 128).to(torch.bfloat16)).to(device)
    table = _repeat(blk, o.rows)
    idx = torch.randint(o.rows, (o.M * o.K,), generator=g, dtype=torch.int32).to(device)
    offsets = (torch.arange(o.M + 1, dtype=torch.int32) * o.K).to(device)
    out = torch.empty(o.M, o.N, dtype=torch.bfloat16, device=device)
    return out, table, idx, offsets


def _paged_operands(o: Op, q_rows: int, g: torch.Generator, device: torch.device) -> tuple:
    """(out, q, k_cache, v_cache, table, ctx) of an attention op over M sequences of K context
    tokens, N query heads over o.rows KV heads and q_rows rows of q, in a paged cache of M * K / 32
    blocks that a seeded random permutation deals out to the sequences.  q is randn; the caches
    repeat one pattern of values k / 64, |k| <= 127."""
    T, D = loadgen.ATTN_BLOCK_TOKENS, loadgen.ATTN_HEAD_DIM
    if o.K % T:
        raise ValueError(f"attention context {o.K} is no multiple of {T}")
    per_seq = o.K // T
    nb = o.M * per_seq
    n = min(nb, ATTN_PATTERN_BLOCKS)
    q = torch.randn(q_rows, o.N, D, generator=g).to(torch.bfloat16).to(device)

    def cache(*shape: int) -> torch.Tensor:
        pat = (torch.randint(-127, 128, (n,) + shape, generator=g).float() / 64).to(torch.bfloat16).to(device)
        return _repeat(pat, nb)
    kc, vc = cache(o.rows, T, D), cache(o.rows, D, T)
    table = torch.randperm(nb, generator=g).to(torch.int32).view(o.M, per_seq).to(device)
    ctx = torch.full((o.M,), o.K, dtype=torch.int32, device=device)
    out = torch.empty(q_rows, o.N, D, dtype=torch.bfloat16, device=device)
    return out, q, kc, vc, table, ctx


def _attn_operands(o: Op, g: torch.Generator, device: torch.device) -> tuple:
    """Decode: one query token per sequence."""
    return _paged_operands(o, o.M, g, device)


def _attn_split_operands(o: Op, g: torch.Generator, device: torch.device) -> tuple:
    """Split-KV decode: the decode operands and the fp32 workspace of the split partials, allocated
    once per op (one launch of the op is in flight at a time: its stream orders them)."""
    ws = torch.empty(loadgen.decode_split_workspace_floats(o.M, o.N, o.splits), dtype=torch.float32, device=device)
    return _paged_operands(o, o.M, g, device) + (ws,)


def _prefill_operands(o: Op, g: torch.Generator, device: torch.device) -> tuple:
    """Prefill: the last o.q of every sequence's K context tokens are its chunk, the chunks packed
    in sequence order (q_start = arange(M + 1) * q)."""
    if o.q > o.K:
        raise ValueError(f"prefill chunk {o.q} is longer than the context {o.K}")
    q_start = (torch.arange(o.M + 1, dtype=torch.int32) * o.q).to(device)
    return _paged_operands(o, o.M * o.q, g, device) + (q_start,)


def _rope_append_operands(o: Op, g: torch.Generator, device: torch.device, cache_dtype=torch.bfloat16) -> tuple:
    """(q_out, qkv, cos_sin, k_cache, v_cache, table, ctx, q_start): the last o.q of every sequence's K
    context tokens are its chunk, packed in sequence order; qkv is randn, the caches (M * K / 32 blocks
    that a seeded random permutation deals out) are what the op writes and start as zeros."""
    T, D = loadgen.ATTN_BLOCK_TOKENS, loadgen.ATTN_HEAD_DIM
    if o.K % T:
        raise ValueError(f"attention context {o.K} is no multiple of {T}")
    if o.q > o.K:
        raise ValueError(f"append chunk {o.q} is longer than the context {o.K}")
    per_seq = o.K // T
    nb = o.M * per_seq
    qkv = torch.randn(o.M * o.q, o.N + 2 * o.rows, D, generator=g).to(torch.bfloat16).to(device)
    cos_sin = loadgen.rope_table(o.K).to(device)
    kc = torch.zeros(nb, o.rows, T, D, dtype=cache_dtype, device=device)
    vc = torch.zeros(nb, o.rows, D, T, dtype=cache_dtype, device=device)
    table = torch.randperm(nb, generator=g).to(torch.int32).view(o.M, per_seq).to(device)
    ctx = torch.full((o.M,), o.K, dtype=torch.int32, device=device)
    q_start = (torch.arange(o.M + 1, dtype=torch.int32) * o.q).to(device)
    q_out = torch.empty(o.M * o.q, o.N, D, dtype=torch.bfloat16, device=device)
    return q_out, qkv, cos_sin, kc, vc, table, ctx, q_start


KV8_K_SCALE, KV8_V_SCALE = 0.5, 0.25          # the kv8 ops' scales, the same for every KV head


def _kv8_scales(o: Op, device: torch.device) -> tuple:
    return (torch.full((o.rows,), KV8_K_SCALE, dtype=torch.float32, device=device),
            torch.full((o.rows,), KV8_V_SCALE, dtype=torch.float32, device=device))


def _paged_kv8_operands(o: Op, g: torch.Generator, device: torch.device, q_rows: Optional[int] = None) -> tuple:
    """_paged_operands over an FP8 cache, and (k_scale, v_scale): the caches repeat one seeded pattern of finite
    e4m3fn codes of magnitude <= 2 (the low seven bits drawn from [0, 0x41): 0x40 is 2.0), any sign.  q_rows: the
    rows of q and out (None: decode's o.M, one per sequence)."""
    if q_rows is None:
        q_rows = o.M
    T, D = loadgen.ATTN_BLOCK_TOKENS, loadgen.ATTN_HEAD_DIM
    if o.K % T:
        raise ValueError(f"attention context {o.K} is no multiple of {T}")
    per_seq = o.K // T
    nb = o.M * per_seq
    n = min(nb, ATTN_PATTERN_BLOCKS)
    q = torch.randn(q_rows, o.N, D, generator=g).to(torch.bfloat16).to(device)

    def cache(*shape: int) -> torch.Tensor:
        pat = torch.randint(0, 0x41, (n,) + shape, generator=g) | (torch.randint(0, 2, (n,) + shape, generator=g) << 7)
        return _repeat(pat.to(torch.uint8).to(device), nb).view(loadgen.FP8)
    kc, vc = cache(o.rows, T, D), cache(o.rows, D, T)
    table = torch.randperm(nb, generator=g).to(torch.int32).view(o.M, per_seq).to(device)
    ctx = torch.full((o.M,), o.K, dtype=torch.int32, device=device)
    out = torch.empty(q_rows, o.N, D, dtype=torch.bfloat16, device=device)
    return (out, q, kc, vc, table, ctx) + _kv8_scales(o, device)


def _attn_kv8_operands(o: Op, g: torch.Generator, device: torch.device) -> tuple:
    """(out, q, k_cache, v_cache, table, ctx, k_scale, v_scale)."""
    return _paged_kv8_operands(o, g, device)


def _attn_split_kv8_operands(o: Op, g: torch.Generator, device: torch.device) -> tuple:
    """(out, q, k_cache, v_cache, table, ctx, ws, k_scale, v_scale): the workspace as _attn_split_operands makes it."""
    ws = torch.empty(loadgen.decode_split_workspace_floats(o.M, o.N, o.splits), dtype=torch.float32, device=device)
    t = _paged_kv8_operands(o, g, device)
    return t[:6] + (ws,) + t[6:]


def _prefill_kv8_operands(o: Op, g: torch.Generator, device: torch.device) -> tuple:
    """(out, q, k_cache, v_cache, table, ctx, q_start, k_scale, v_scale): the chunks as _prefill_operands packs them."""
    if o.q > o.K:
        raise ValueError(f"prefill chunk {o.q} is longer than the context {o.K}")
    q_start = (torch.arange(o.M + 1, dtype=torch.int32) * o.q).to(device)
    t = _paged_kv8_operands(o, g, device, o.M * o.q)
    return t[:6] + (q_start,) + t[6:]


def _rope_append_kv8_operands(o: Op, g: torch.Generator, device: torch.device) -> tuple:
    """_rope_append_operands with FP8 caches that start as zeros (code 0x00), and (k_scale, v_scale)."""
    return _rope_append_operands(o, g, device, loadgen.FP8) + _kv8_scales(o, device)


def _add_rmsnorm_operands(o: Op, g: torch.Generator, device: torch.device) -> tuple:
    """(y, res_out, x, residual, weight): M rows of N elements; x and residual are randn, the weight is
    1 + 0.1 * randn, all bf16.  The outputs are buffers of their own (the launch is replayable)."""
    x = torch.randn(o.M, o.N, generator=g).to(torch.bfloat16).to(device)
    residual = torch.randn(o.M, o.N, generator=g).to(torch.bfloat16).to(device)
    weight = (1 + 0.1 * torch.randn(o.N, generator=g)).to(torch.bfloat16).to(device)
    y = torch.empty(o.M, o.N, dtype=torch.bfloat16, device=device)
    res_out = torch.empty(o.M, o.N, dtype=torch.bfloat16, device=device)
    return y, res_out, x, residual, weight


def _swiglu_operands(o: Op, g: torch.Generator, device: torch.device) -> tuple:
    """(out, gate_up): M rows of N gate and N up columns, randn in bf16."""
    gate_up = torch.randn(o.M, 2 * o.N, generator=g).to(torch.bfloat16).to(device)
    return torch.empty(o.M, o.N, dtype=torch.bfloat16, device=device), gate_up


SAMPLE_TEMPERATURE, SAMPLE_TOP_P = 0.8, 0.9          # the "sample" op's parameters, the same on every row


def _sample_operands(o: Op, g: torch.Generator, device: torch.device) -> tuple:
    """(out, logits, u, temperature, top_k, top_p): M rows of N logits, bf16(1.5 * randn); u is rand, the
    temperature 0.8, top_k = o.K and top_p 0.9 on every row.  The per-row u is drawn before the logits
    (tests/test_sample_cpu.py counts how many rows of the two LLM-head workloads put u or top_p close to a
    boundary of the cumulative weights)."""
    u = torch.rand(o.M, generator=g).to(device)
    logits = (1.5 * torch.randn(o.M, o.N, generator=g)).to(torch.bfloat16).to(device)
    temperature = torch.full((o.M,), SAMPLE_TEMPERATURE, dtype=torch.float32, device=device)
    top_k = torch.full((o.M,), o.K, dtype=torch.int32, device=device)
    top_p = torch.full((o.M,), SAMPLE_TOP_P, dtype=torch.float32, device=device)
    return torch.empty(o.M, dtype=torch.int32, device=device), logits, u, temperature, top_k, top_p


MOE_PATTERN_EXPERTS = 4           # experts of the CPU-generated pattern the expert weights repeat


def _moe_routing(T: int, E: int, k: int, g: torch.Generator) -> tuple:
    """(topk_w, sorted_ids, tile_expert, slot_pos) on the CPU for T tokens with randn router logits: the routing of
    a moe_gemm / moe_combine op's operands, computed once with loadgen's pure-torch references."""
    logits = torch.randn(T, E, generator=g).to(torch.bfloat16)
    ids, w = loadgen.moe_topk_reference(logits, k)
    sorted_ids, tile_expert, _, slot_pos = loadgen.moe_align_reference(ids, E)
    return w, sorted_ids, tile_expert, slot_pos


def _moe_route_operands(o: Op, g: torch.Generator, device: torch.device) -> tuple:
    """(topk_ids, logits, topk_w, sorted_ids, tile_expert, expert_offsets, slot_pos): M tokens' randn logits over N
    experts in bf16, and the six outputs of the top-K routing."""
    logits = torch.randn(o.M, o.N, generator=g).to(torch.bfloat16).to(device)
    tiles = loadgen.moe_max_tiles(o.M, o.K, o.N)
    i32 = dict(dtype=torch.int32, device=device)
    return (torch.empty(o.M, o.K, **i32), logits, torch.empty(o.M, o.K, dtype=torch.float32, device=device),
            torch.empty(tiles * loadgen.MOE_BLOCK_M, **i32), torch.empty(tiles, **i32), torch.empty(o.N + 1, **i32),
            torch.empty(o.M * o.K, **i32))


def _moe_gemm_operands(o: Op, g: torch.Generator, device: torch.device) -> tuple:
    """(out, a, w, sorted_ids, tile_expert): the routing of M tokens over o.rows experts (top-o.q) from random logits;
    a is randn -- the [M, K] token rows with o.gather, else the [P_max, K] sorted intermediate --; the weights
    [o.rows, N, K] repeat a pattern of four experts of uniform values in +-0.05.  out starts as zeros: the rows of
    the tiles the routing leaves unused are never written."""
    _, sorted_ids, tile_expert, _ = _moe_routing(o.M, o.rows, o.q, g)
    P = sorted_ids.numel()
    a = torch.randn(o.M if o.gather else P, o.K, generator=g).to(torch.bfloat16).to(device)
    pat = ((torch.rand(min(o.rows, MOE_PATTERN_EXPERTS), o.N, o.K, generator=g) * 2 - 1) * 0.05).to(torch.bfloat16).to(device)
    out = torch.zeros(P, o.N, dtype=torch.bfloat16, device=device)
    return out, a, _repeat(pat, o.rows), sorted_ids.to(device), tile_expert.to(device)


def _moe_combine_operands(o: Op, g: torch.Generator, device: torch.device) -> tuple:
    """(out, y, slot_pos, topk_w): the routing of M tokens over o.rows experts (top-K) from random logits, y randn
    [P_max, N] in bf16."""
    w, sorted_ids, _, slot_pos = _moe_routing(o.M, o.rows, o.K, g)
    y = torch.randn(sorted_ids.numel(), o.N, generator=g).to(torch.bfloat16).to(device)
    return torch.empty(o.M, o.N, dtype=torch.bfloat16, device=device), y, slot_pos.to(device), w.to(device)


def _quant_mx_operands(o: Op, g: torch.Generator, device: torch.device) -> tuple:
    """(q, scales, x): M rows of N elements, randn in bf16, and the MX outputs of format o.fmt."""
    x = torch.randn(o.M, o.N, generator=g).to(torch.bfloat16).to(device)
    q = torch.empty(o.M, loadgen.mx_row_bytes(o.fmt, o.N), dtype=loadgen.mx_element_dtype(o.fmt), device=device)
    return q, torch.empty(o.M, o.N // loadgen.MX_BLOCK, dtype=torch.uint8, device=device), x


MX_PATTERN_ROWS = 256             # rows of the CPU-generated block an MX weight matrix repeats


def _mx_random(rows: int, K: int, fmt: str, g: torch.Generator, device: torch.device) -> tuple:
    """(elements, scales) of a [rows, K] MX operand made without quantising anything: random element bytes -- for fp8
    without the two NaN codes 0x7F and 0xFF (the low seven bits are drawn from [0, 0x7F)) -- and scale bytes from
    [120, 127].  A matrix of more than MX_PATTERN_ROWS rows repeats one CPU-generated block of that many."""
    n = min(rows, MX_PATTERN_ROWS)
    if fmt == "fp8":
        el = torch.randint(0, 0x7F, (n, K), generator=g) | (torch.randint(0, 2, (n, K), generator=g) << 7)
    else:
        el = torch.randint(0, 256, (n, K // 2), generator=g)
    sc = torch.randint(120, 128, (n, K // loadgen.MX_BLOCK), generator=g).to(torch.uint8)
    el = _repeat(el.to(torch.uint8).to(device), rows).view(loadgen.mx_element_dtype(fmt))
    return el, _repeat(sc.to(device), rows)


def _gemm_mx_operands(o: Op, g: torch.Generator, device: torch.device) -> tuple:
    """(c, a_q, a_scales, w_q, w_scales, bias): activations [M, K] of format o.fmt, fp4 weights [N, K] (_mx_random),
    a zero bias and the bf16 output."""
    a_q, a_s = _mx_random(o.M, o.K, o.fmt, g, device)
    w_q, w_s = _mx_random(o.N, o.K, "fp4", g, device)
    bias = torch.zeros(o.N, dtype=torch.float32, device=device)
    return torch.empty(o.M, o.N, dtype=torch.bfloat16, device=device), a_q, a_s, w_q, w_s, bias


def _triad_operands(o: Op, g: torch.Generator, device: torch.device) -> tuple:
    return tuple(torch.ones(o.n_floats, dtype=torch.float32, device=device) for _ in range(3))


# The launches look their loadgen entry point up when called (tests replace the attributes).  The
# gather's indices, and the attention's ctx_lens and block ids, are in range by construction: no
# check, no sync (this runs under graph capture); so are the prefill's q_start and max_q_len, and the
# sampler's parameters, and the MoE ops' layouts (the CPU reference built them).
def _launch_gemm(o: Op, t: tuple, st, budget: int, blocks: int) -> None:
    a, bt, bias, c = t
    loadgen.gemm(a, bt, out=c, bias=bias, relu=o.relu, stream=st, cu_budget=budget)


def _launch_gemm8(o: Op, t: tuple, st, budget: int, blocks: int) -> None:
    a, bt, bias, c = t
    loadgen.gemm_fp8(a, bt, out=c, bias=bias, relu=o.relu, stream=st, cu_budget=budget)


def _launch_gather(o: Op, t: tuple, st, budget: int, blocks: int) -> None:
    out, table, idx, offsets = t
    loadgen.embedding_bag(table, idx, offsets, out=out, stream=st, check_indices=False)


def _launch_attn(o: Op, t: tuple, st, budget: int, blocks: int) -> None:
    out, q, kc, vc, table, ctx = t
    loadgen.paged_decode_attention(q, kc, vc, table, ctx, out=out, stream=st, check=False)


def _launch_attn_split(o: Op, t: tuple, st, budget: int, blocks: int) -> None:
    out, q, kc, vc, table, ctx, ws = t
    loadgen.paged_decode_attention(q, kc, vc, table, ctx, out=out, stream=st, check=False, kv_splits=o.splits,
                                   workspace=ws)


def _launch_prefill(o: Op, t: tuple, st, budget: int, blocks: int) -> None:
    out, q, kc, vc, table, ctx, q_start = t
    loadgen.paged_prefill_attention(q, kc, vc, table, ctx, q_start, max_q_len=o.q, out=out, stream=st, check=False)


def _launch_rope_append(o: Op, t: tuple, st, budget: int, blocks: int) -> None:
    q_out, qkv, cos_sin, kc, vc, table, ctx, q_start = t
    loadgen.rope_append(qkv, cos_sin, kc, vc, table, ctx, q_start, max_q_len=o.q, q_out=q_out, stream=st, check=False)


def _launch_attn_kv8(o: Op, t: tuple, st, budget: int, blocks: int) -> None:
    out, q, kc, vc, table, ctx, ks, vs = t
    loadgen.paged_decode_attention_kv8(q, kc, vc, table, ctx, ks, vs, out=out, stream=st, check=False)


def _launch_attn_split_kv8(o: Op, t: tuple, st, budget: int, blocks: int) -> None:
    out, q, kc, vc, table, ctx, ws, ks, vs = t
    loadgen.paged_decode_attention_kv8(q, kc, vc, table, ctx, ks, vs, out=out, stream=st, check=False,
                                       kv_splits=o.splits, workspace=ws)


def _launch_rope_append_kv8(o: Op, t: tuple, st, budget: int, blocks: int) -> None:
    q_out, qkv, cos_sin, kc, vc, table, ctx, q_start, ks, vs = t
    loadgen.rope_append(qkv, cos_sin, kc, vc, table, ctx, q_start, max_q_len=o.q, q_out=q_out, stream=st, check=False,
                        k_scale=ks, v_scale=vs)


def _launch_prefill_kv8(o: Op, t: tuple, st, budget: int, blocks: int) -> None:
    out, q, kc, vc, table, ctx, q_start, ks, vs = t
    loadgen.paged_prefill_attention_kv8(q, kc, vc, table, ctx, q_start, ks, vs, max_q_len=o.q, out=out, stream=st,
                                        check=False)


def _launch_add_rmsnorm(o: Op, t: tuple, st, budget: int, blocks: int) -> None:
    y, res_out, x, residual, weight = t
    loadgen.add_rmsnorm(x, weight, residual, out=y, residual_out=res_out, stream=st)


def _launch_swiglu(o: Op, t: tuple, st, budget: int, blocks: int) -> None:
    out, gate_up = t
    loadgen.swiglu(gate_up, out=out, stream=st)


def _launch_sample(o: Op, t: tuple, st, budget: int, blocks: int) -> None:
    out, logits, u, temperature, top_k, top_p = t
    loadgen.sample_tokens(logits, u, temperature, top_k, top_p, out=out, stream=st, check=False)


def _launch_moe_route(o: Op, t: tuple, st, budget: int, blocks: int) -> None:
    topk_ids, logits, topk_w, sorted_ids, tile_expert, expert_offsets, slot_pos = t
    loadgen.moe_route(logits, o.K, topk_ids=topk_ids, topk_w=topk_w, sorted_ids=sorted_ids, tile_expert=tile_expert,
                      expert_offsets=expert_offsets, slot_pos=slot_pos, stream=st, check=False)


def _launch_moe_gemm(o: Op, t: tuple, st, budget: int, blocks: int) -> None:
    out, a, w, sorted_ids, tile_expert = t
    loadgen.moe_gemm(a, w, sorted_ids, tile_expert, o.M * o.q, gather_div=o.q if o.gather else 0, out=out, stream=st,
                     check=False)


def _launch_moe_combine(o: Op, t: tuple, st, budget: int, blocks: int) -> None:
    out, y, slot_pos, topk_w = t
    loadgen.moe_combine(y, slot_pos, topk_w, out=out, stream=st)


def _launch_quant_mx(o: Op, t: tuple, st, budget: int, blocks: int) -> None:
    q, scales, x = t
    loadgen.quantize_mx(x, o.fmt, out=q, scales=scales, stream=st)


def _launch_gemm_mx(o: Op, t: tuple, st, budget: int, blocks: int) -> None:
    c, a_q, a_s, w_q, w_s, bias = t
    loadgen.gemm_mx(a_q, a_s, w_q, w_s, o.fmt, out=c, bias=bias, relu=o.relu, stream=st, cu_budget=budget)


def _launch_triad(o: Op, t: tuple, st, budget: int, blocks: int) -> None:
    x, y, z = t
    loadgen.triad(x, y, z, 1.0001, blocks=blocks, stream=st)


# What the executor knows of an op kind: kind -> (make(o, g, device) -> the operand tuple, drawing
# from the CPU generator g; launch(o, t, st, budget, blocks), the kind's one loadgen call; the
# position of the output in the tuple).  Operand layouts: GEMMs (a, bt, bias, c); gather (out,
# table, idx, offsets); attn (out, q, k_cache, v_cache, table, ctx); prefill the same and q_start;
# attn_split the same and the workspace; rope_append (q_out, qkv, cos_sin, k_cache, v_cache, table, ctx,
# q_start); add_rmsnorm (y, res_out, x, residual, weight); swiglu (out, gate_up); sample (out, logits, u,
# temperature, top_k, top_p); moe_route (topk_ids, logits, topk_w, sorted_ids, tile_expert, expert_offsets,
# slot_pos); moe_gemm (out, a, w, sorted_ids, tile_expert); moe_combine (out, y, slot_pos, topk_w); quant_mx (q, scales,
# x); gemm_mx (c, a_q, a_scales, w_q, w_scales, bias); attn_kv8, attn_split_kv8 and rope_append_kv8 their bf16 kinds'
# and (k_scale, v_scale), the caches float8_e4m3fn; prefill_kv8 prefill's and (k_scale, v_scale) likewise; triad
# (x, y, z), x = y + s z.
OP_KINDS = {
    "gemm": (_gemm_operands, _launch_gemm, 3),
    "gemm8": (_gemm_operands, _launch_gemm8, 3),
    "gather": (_gather_operands, _launch_gather, 0),
    "attn": (_attn_operands, _launch_attn, 0),
    "attn_split": (_attn_split_operands, _launch_attn_split, 0),
    "prefill": (_prefill_operands, _launch_prefill, 0),
    "rope_append": (_rope_append_operands, _launch_rope_append, 0),
    "add_rmsnorm": (_add_rmsnorm_operands, _launch_add_rmsnorm, 0),
    "swiglu": (_swiglu_operands, _launch_swiglu, 0),
    "sample": (_sample_operands, _launch_sample, 0),
    "moe_route": (_moe_route_operands, _launch_moe_route, 0),
    "moe_gemm": (_moe_gemm_operands, _launch_moe_gemm, 0),
    "moe_combine": (_moe_combine_operands, _launch_moe_combine, 0),
    "quant_mx": (_quant_mx_operands, _launch_quant_mx, 0),
    "gemm_mx": (_gemm_mx_operands, _launch_gemm_mx, 0),
    "attn_kv8": (_attn_kv8_operands, _launch_attn_kv8, 0),
    "attn_split_kv8": (_attn_split_kv8_operands, _launch_attn_split_kv8, 0),
    "rope_append_kv8": (_rope_append_kv8_operands, _launch_rope_append_kv8, 0),
    "prefill_kv8": (_prefill_kv8_operands, _launch_prefill_kv8, 0),
    "triad": (_triad_operands, _launch_triad, 0),
}


def _kind(o: Op) -> tuple:
    try:
        return OP_KINDS[o.kind]
    except KeyError:
        raise ValueError(f"unknown op kind {o.kind!r}") from None


class _Buffers:
    def __init__(self, w: Workload, device: torch.device):
        # (a CRC of the name, not hash(): str hashes change from process to process, and two runs
        # of the bench must feed the kernels the same operands)
        g = torch.Generator(device="cpu").manual_seed(zlib.crc32(w.name.encode()) & 0xFFFF)
        try:
            self.ops: List[Tuple[Op, tuple]] = [(o, _kind(o)[0](o, g, device)) for o in w.ops]
        except ValueError as e:
            raise ValueError(f"workload {w.name}: {e}") from None


def enqueue_op(o: Op, t: tuple, st, budget: int, blocks: int = 0) -> None:
    """One op on stream `st`, on the operands `t` that _Buffers made for it."""
    _kind(o)[1](o, t, st, budget, blocks)


def op_output(o: Op, t: tuple) -> torch.Tensor:
    """The tensor of `t` that the op's kernel writes."""
    return t[_kind(o)[2]]


def enqueue_ops(bufs: _Buffers, iters: int, st, budget: int, blocks: int = 0) -> None:
    """`iters` iterations of a workload's op list on stream `st` (GEMM tiles sized for `budget`
    CUs, 0 = the whole chip)."""
    # the kinds are looked up once, not per iteration (podrun and --graphs 0 pay this per launch)
    launches = [(_kind(o)[1], o, t) for o, t in bufs.ops]
    for _ in range(iters):
        for launch, o, t in launches:
            launch(o, t, st, budget, blocks)


def lpt_balance(runs: List[PodRun], slot_work: Dict[Tuple[int, int], float], work=None) -> None:
    """Reassign the slots of each group of same-size Burstable pods of this epoch: longest pod
    first onto the slot with the least cumulative work (ties: the lower slot).  `slot_work`
    ((first unit, units) -> cumulative work) is the caller's running state."""
    work = work or DeviceExecutor.pod_work
    groups: Dict[int, List[PodRun]] = {}
    for r in runs:
        if not r.masked:
            groups.setdefault(r.n_units, []).append(r)
    for n, rs in groups.items():
        if len(rs) < 2:
            continue
        slots = sorted(r.first_unit for r in rs)
        if len(set(slots)) != len(slots):
            continue
        for r in sorted(rs, key=work, reverse=True):
            u = min(slots, key=lambda s: (slot_work.get((s, n), 0.0), s))
            slots.remove(u)
            r.first_unit = u
            slot_work[(u, n)] = slot_work.get((u, n), 0.0) + work(r)


class DeviceExecutor:
    # co-run launch policy (tools/pod_mix.py measures these on the catalog mix):
    #   gemm_share   -- tell the GEMM tile picker the pod's CU share instead of the chip
    #   triad_blocks -- workgroups per stream-kernel launch (0 = the kernel's default)
    #   (capping the stream kernels at k workgroups per CU of the pod's share was measured and
    #   dropped: 380 / 509 / 550 pods/s at k = 1 / 2 / 4 vs 586 uncapped, profiles/archive/r03_triad_cap_ab.json)
    gemm_share = True
    triad_blocks = 0
    #   use_graphs   -- replay each pod's whole kernel sequence (iters x ops) as one captured
    #                   HIP graph on the pod's stream (captured once per workload/slot)
    use_graphs = False
    #   balance_slots -- (off by default; an A/B arm) re-slot each epoch's same-size Burstable
    #                   pods longest first onto the slot stream with the least cumulative work
    #                   (LPT).  It was round 3's default: +1.5 % pods/s over the scheduler's
    #                   first-fit slots, but blind to SLOs (-9 points of SLO attainment).  The
    #                   scheduler now chooses each pod's slot itself on its model of the slot
    #                   pipelines (plugins.gpu.timeline, --plan-slots), and the executor runs
    #                   every pod on the slot it was given (MI355X, 20 steps x 3 interleaved:
    #                   603.5 pods/s / 56.25 % SLOs vs 600.7 / 53.75 % for LPT re-slotting,
    #                   gpurun_out r04_slots_ab20 -> profiles/archive/r04_slots_ab/)
    balance_slots = os.environ.get("GPUSCHED_BALANCE_SLOTS", "0") == "1"

    def __init__(self, device: int = 0, use_cu_masks: bool = True, units_per_gpu: int = 8):
        self.device = device
        self.dev = torch.device("cuda", device)
        self.use_cu_masks = use_cu_masks
        self.units = units_per_gpu
        self._streams: Dict[Tuple[int, int], object] = {}
        self._bufs: Dict[Tuple[str, int, int], _Buffers] = {}
        self._last_events: List[torch.cuda.Event] = []
        self._unit_last: Dict[int, Tuple[Tuple[int, int], torch.cuda.Event]] = {}
        # (workload, units, iterations) of every pod launched, per epoch -- not the PodRuns: those
        # hold two HIP events each, and a long run would keep every one of them alive
        self.epoch_pods: List[List[Tuple[str, int, int]]] = []
        self._graphs: Dict[Tuple, "torch.cuda.CUDAGraph"] = {}
        self.lazy_captures = 0           # graphs captured by launch_epoch (not warm()): outside pod timing
        self.flops_done = 0.0
        self.bytes_done = 0.0
        self._slot_work: Dict[Tuple[int, int], float] = {}     # (first unit, units) -> cumulative work
        # the executor's clock: pod start / end events are reported as ms after this event
        # (the co-run learner rebuilds which pods of neighbouring epochs overlapped)
        self.clock = torch.cuda.Event(enable_timing=True)
        self.clock.record(torch.cuda.current_stream(self.device))

    def stream_for(self, first_unit: int, n_units: int, masked: bool = True):
        key = (first_unit, n_units, masked)
        st = self._streams.get(key)
        if st is None:
            if self.use_cu_masks and masked:
                from ..ops.cumask import MaskedStream
                st = MaskedStream(cu_slice_mask(first_unit, n_units), self.device)
            else:
                st = _PlainStream(self.device)
            self._streams[key] = st
        return st

    # one buffer set per workload instead of per (workload, slot): ~1/4 of the HBM, for
    # multi-rank rehearsals that map every rank onto one GPU (GPUSCHED_FORCE_DEVICE);
    # co-running pods of one workload then share operands (load generation only)
    shared_buffers = os.environ.get("GPUSCHED_SHARED_BUFFERS", "") == "1"

    def buffers(self, w: Workload, first_unit: int, n_units: int) -> _Buffers:
        k = (w.name, 0, 0) if self.shared_buffers else (w.name, first_unit, n_units)
        b = self._bufs.get(k)
        if b is None:
            b = _Buffers(w, self.dev)
            self._bufs[k] = b
        return b

    def warm(self, placements: List[PodRun]) -> None:
        """Pre-create streams/buffers -- and, with use_graphs, capture the pods' graphs --
        outside any timed region."""
        for p in placements:
            st = self.stream_for(p.first_unit, p.n_units, p.masked)
            bufs = self.buffers(workload_by_name(p.workload), p.first_unit, p.n_units)
            if self.use_graphs:
                self._graph_for(p, bufs, st.stream, self._budget(p))
        torch.cuda.synchronize(self.device)

    def _budget(self, r: PodRun) -> int:
        if r.policy == 1:
            return 0                     # wide: tiles for the whole chip (more, smaller workgroups)
        return r.n_units * CUS_PER_UNIT if self.gemm_share else 0   # the pod's CU share

    def _enqueue_ops(self, r: PodRun, bufs: "_Buffers", st, budget: int) -> None:
        enqueue_ops(bufs, r.iters, st, budget, self.triad_blocks)

    def _graph_for(self, r: PodRun, bufs: "_Buffers", st, budget: int) -> "torch.cuda.CUDAGraph":
        """One HIP graph per (workload, unit slot, QoS, iters): captured on the pod's own
        stream, so replaying it there keeps the stream's CU mask and its ordering."""
        k = (r.workload, r.first_unit, r.n_units, r.masked, r.iters, budget, self.triad_blocks)
        g = self._graphs.get(k)
        if g is None:
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                self._enqueue_ops(r, bufs, st, budget)
            torch.cuda.synchronize(self.device)
            self._graphs[k] = g
        return g

    def launch_epoch(self, runs: List[PodRun]) -> None:
        """Enqueue one epoch's pods; returns immediately (async).

        Ordering is per CU-slice unit, not per epoch: a pod waits (device-side) only for
        the last pod that occupied any of ITS units on another stream; pods reusing the
        same unit range share a stream and are ordered by it.  So a slot whose pod
        finished early starts its next pod at once instead of idling until the slowest
        pod of the epoch completes (work-conserving), while two pods never overlap on the
        same CUs -- exactly the ledger's capacity model."""
        if self.balance_slots:
            self._balance(runs)
        # buffers, streams and (with use_graphs) graphs of every pod are made BEFORE any pod's
        # start event is recorded: a lazy capture synchronises the device and captures on the
        # host, and inside a pod's [start, end) it would be measured as that pod's run time --
        # an outlier the planner's feedback would read as a slow GPU (GPUTEST_r04.json)
        prep = []
        for r in runs:
            w = workload_by_name(r.workload)
            bufs = self.buffers(w, r.first_unit, r.n_units)
            budget = self._budget(r)
            st = self.stream_for(r.first_unit, r.n_units, r.masked).stream
            g = None
            if self.use_graphs:
                n0 = len(self._graphs)
                g = self._graph_for(r, bufs, st, budget)
                self.lazy_captures += len(self._graphs) - n0
            prep.append((w, bufs, budget, g))
        for r, (w, bufs, budget, g) in zip(runs, prep):
            key = (r.first_unit, r.n_units, r.masked)
            r.start = torch.cuda.Event(enable_timing=True)
            r.end = torch.cuda.Event(enable_timing=True)
            st = self.stream_for(*key).stream
            waited = set()
            for u in range(r.first_unit, r.first_unit + r.n_units):
                last = self._unit_last.get(u)
                if last is not None and last[0] != key and id(last[1]) not in waited:
                    # a stream-wait is a barrier packet pending on this pod's queue until the
                    # previous occupant ends -- it slows the queue sharing its hardware pipe
                    # (see wait_all); skip it when that pod has already finished
                    if not last[1].query():
                        st.wait_event(last[1])
                    waited.add(id(last[1]))
            r.start.record(st)
            if g is not None:
                with torch.cuda.stream(st):
                    g.replay()
            else:
                self._enqueue_ops(r, bufs, st, budget)
            r.end.record(st)
            for u in range(r.first_unit, r.first_unit + r.n_units):
                self._unit_last[u] = (key, r.end)
            self.flops_done += w.flops * r.iters
            self.bytes_done += w.bytes * r.iters
        self._last_events = [ev for _, ev in {id(e): (k, e) for k, e in self._unit_last.values()}.values()]
        self.epoch_pods.append([(r.workload, r.n_units, r.iters) for r in runs])

    @staticmethod
    def pod_work(r: PodRun) -> float:
        """Relative work of a pod (its kernels' roofline time alone on the GPU x iterations)."""
        from ..models.workloads import roofline_seconds
        return roofline_seconds(workload_by_name(r.workload), 1.0) * max(r.iters, 1)

    def _balance(self, runs: List[PodRun]) -> None:
        lpt_balance(runs, self._slot_work, self.pod_work)

    # host poll period while waiting for an epoch's end events
    poll_s = 20e-6

    def wait_epoch(self, runs: List[PodRun]) -> None:
        """Host-wait until every pod of an epoch finished (its end events), by polling the
        events (wakes within tens of microseconds; never a stream-wait, see wait_all)."""
        for r in runs:
            ev = r.end
            if ev is None:
                continue
            while not ev.query():
                time.sleep(self.poll_s)

    def wait_all(self) -> None:
        """Host-wait until every enqueued pod finished, by polling their end events.

        Never by making another stream wait on them: a stream-wait leaves a barrier packet
        pending on that stream's hardware queue for as long as the pods run, and the queue of
        the pod stream sharing its hardware pipe is then served at about half rate -- with
        the default stream joined on 4 co-running pods, the 4th pod stream took 6.0 ms instead
        of 3.5 and the group 6.2 ms instead of 3.7 (profiles/archive/r03_queue_fairness/README.md)."""
        for ev in self._last_events:
            while not ev.query():
                time.sleep(self.poll_s)

    def collect(self, runs: List[PodRun]) -> Dict[str, float]:
        """After a sync: per-pod times + busy accounting for one epoch."""
        busy_unit_ms = 0.0
        t_first, t_last = None, None
        slo_ok = 0
        for r in runs:
            r.ms = r.start.elapsed_time(r.end)
            busy_unit_ms += r.ms * r.n_units
            if r.slo <= 0 or r.throughput >= r.slo:
                slo_ok += 1
        if runs:
            starts = [r.start for r in runs]
            ends = [r.end for r in runs]
            t0 = starts[0]
            t_first = min(t0.elapsed_time(s) for s in starts)
            t_last = max(t0.elapsed_time(e) for e in ends)
        span = (t_last - t_first) if runs else 0.0
        return {"pods": float(len(runs)), "busy_unit_ms": busy_unit_ms, "span_ms": span,
                "slo_ok": float(slo_ok)}

    def close(self) -> None:
        torch.cuda.synchronize(self.device)
        self._graphs.clear()
        for s in self._streams.values():
            s.close()
        self._streams.clear()


class _PlainStream:
    def __init__(self, device: int):
        self.stream = torch.cuda.Stream(device=device)

    def close(self) -> None:
        pass
