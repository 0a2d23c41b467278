"""The FP8 paged-KV cache's writer and its chunked-prefill reader in a row (run with `-m gpu` on an MI355X): 8 ragged
sequences get a prefix chunk appended with rope_append into float8_e4m3fn caches whose every byte is SENT8 before,
then a further chunk, and paged_prefill_attention_kv8 runs over the second chunk's q_out.  The reference is
PRE.reference (float64) on loadgen.dequantize_kv8_reference of the caches READ BACK from the device, with the scales
applied per KV head, and the device's q_out: whatever the writer stored is what the reader must have seen.

  match    identity rotation table (c = 1, s = 0); K of token t is 4 H[t % 128] (stored +-16 and +-32 under k_scale =
           (2^-2, 2^-3)), q of the second chunk's columns PRE's match rows, V = v_scale * (an e4m3fn value of six
           binades) with v_scale = (4, 2^-3): the appends are exact -- the cache bytes are asserted against the
           operands -- and so is the attention: `torch.equal` with PRE's exact expectation, which the float64
           reference, rounded float64 -> fp32 -> bf16, is asserted to equal.
  random   the true rope_table, q and K randn (k_scale = 1/16), V uniform in [-1, 1] (v_scale = 2^-8):
           |out - ref| <= 2^-7 * max|V_deq|, the decode modules' bound.

In both, the last token of each chunk -- the prefix's with ctx = the prefix, the second chunk's with the whole
context -- goes through paged_decode_attention_kv8 on the same caches and agrees with the float64 reference within
that bound.

The two LLM_KV8_PREFILL workloads run through podrun and through the executor, whose buffers are checked and whose
append and attention outputs are spot-checked on 8 rows against the references.
"""
import json
import subprocess
import sys

import pytest
import torch

import test_gpu_decode_attn_exact as ATT
import test_gpu_prefill_attn_exact as PRE
import test_gpu_rope_append_exact as ROPE

pytestmark = pytest.mark.gpu

# MEASURED on an MI355X (printed by the tests):
MEASURED = """
  random regime: max|out - ref| = 0.00272 (bound 0.00781); 0 of 277,248 K bytes differ from the reference bytes.  The
  chunks' last tokens through the decode reader: 0.00155 (prefix) and 0.00128 (second chunk) in the random regime,
  0.03740 and 0.01562 in the match regime (bound 0.11719: max|V_deq| = 15); decode against prefill on the second
  chunk's rows: 0 in the match regime, 0.00195 in the random one.
  llm_kv8_layer_prefill_2048: append K 0.9859 and q_out 0.8873 of their bounds on 8 rows, attention max|out - ref| =
  0.00005 (bound 0.00391); llm_kv8_chunk_prefill_64: 0.9970, 0.9095, 0.00006.  The module: 7 tests in 7 s, 5.5 s of them
  the two podrun processes.
"""

D, T, HALF = ATT.D, ATT.T, ROPE.HALF
FP8, U8 = torch.float8_e4m3fn, torch.uint8
SENT8 = 0x5A
GROUP, HKV = 4, 2
HQ = GROUP * HKV
PREFIX = (160, 0, 33, 150, 97, 31, 64, 130)
CHUNK = (96, 33, 31, 90, 32, 1, 65, 70)
CTXS = tuple(p + c for p, c in zip(PREFIX, CHUNK))
SEQS = tuple(zip(CTXS, CHUNK))                                            # PRE's (ctx, q_len) list of the second chunk


def lg():
    from k8s_gpu_scheduler_amd.ops import loadgen
    return loadgen


def test_the_sequences_are_ragged():
    assert len(SEQS) == 8 and max(CTXS) == 256 and 0 in PREFIX and 1 in CHUNK
    assert any(p % T and (p + c) % T for p, c in zip(PREFIX, CHUNK))       # a chunk that starts and ends inside a block
    assert any(c * GROUP > 2 * PRE.COLUMNS for c in CHUNK)                 # more than two workgroups per (sequence, KV head)


def operands(regime, g):
    """(per-sequence qkv bf16 [ctx, Ht, 128], cos_sin, k_scale, v_scale, logical V per sequence [Hkv, ctx, D])."""
    if regime == "random":
        x = [torch.cat([torch.randn(c, HQ + HKV, D, generator=g), torch.rand(c, HKV, D, generator=g) * 2 - 1], dim=1).to(torch.bfloat16)
             for c in CTXS]
        return x, lg().rope_table(max(CTXS)), torch.tensor([1 / 16, 1 / 16]), torch.tensor([2.0 ** -8] * 2), None
    ks, vs = torch.tensor([2.0 ** -2, 2.0 ** -3]), torch.tensor([4.0, 2.0 ** -3])
    H = ATT.hadamard()
    rows, logical_v = [], []
    for c, n in SEQS:
        code = torch.randint(0x18, 0x48, (c, HKV, D), generator=g) | (torch.randint(0, 2, (c, HKV, D), generator=g) << 7)
        v = code.to(U8).view(FP8).float() * vs.view(1, HKV, 1)
        q = torch.randn(c, HQ, D, generator=g)                                          # the prefix's q rows: any
        q[c - n:] = 8 * H[PRE.match_columns(c, n, HQ)[1]]
        k = (4 * H[torch.arange(c) % 128])[:, None].repeat(1, HKV, 1)
        rows.append(torch.cat([q, k, v], dim=1).to(torch.bfloat16))
        logical_v.append(v.transpose(0, 1))
    cs = torch.cat([torch.ones(max(CTXS), HALF), torch.zeros(max(CTXS), HALF)], dim=1)
    return rows, cs, ks, vs, logical_v


@pytest.mark.parametrize("regime", ["match", "random"])
def test_append_append_then_prefill(regime):
    g = torch.Generator().manual_seed(9800 + len(regime))
    table, nb = PRE.block_tables(CTXS, g)
    per_seq, cs, ks, vs, logical_v = operands(regime, g)
    qkv1 = torch.cat([x[:p] for x, p in zip(per_seq, PREFIX)])
    qkv2 = torch.cat([x[p:] for x, p in zip(per_seq, PREFIX)])
    ctx1, ctx2 = torch.tensor(PREFIX, dtype=torch.int32), torch.tensor(CTXS, dtype=torch.int32)
    start1 = torch.tensor((0,) + PREFIX).cumsum(0).to(torch.int32)
    start2 = torch.tensor((0,) + CHUNK).cumsum(0).to(torch.int32)
    tab = table.cuda()
    kc = torch.full((nb, HKV, T, D), SENT8, dtype=U8, device="cuda").view(FP8)
    vc = torch.full((nb, HKV, D, T), SENT8, dtype=U8, device="cuda").view(FP8)
    sc = dict(k_scale=ks.cuda(), v_scale=vs.cuda())
    q_out1 = lg().rope_append(qkv1.cuda(), cs.cuda(), kc, vc, tab, ctx1.cuda(), start1.cuda(), **sc)
    q_out2 = lg().rope_append(qkv2.cuda(), cs.cuda(), kc, vc, tab, ctx2.cuda(), start2.cuda(), **sc)
    out = lg().paged_prefill_attention_kv8(q_out2, kc, vc, tab, ctx2.cuda(), start2.cuda(), **sc)
    torch.cuda.synchronize()
    kb, vb = kc.view(U8).cpu(), vc.view(U8).cpu()
    # nothing but the tokens' slots was written, and V is the reference's bytes
    whole = torch.cat(per_seq)
    start = torch.tensor((0,) + CTXS).cumsum(0).to(torch.int32)
    ref_kb, ref_vb = lg().rope_append_kv8_reference(whole, cs, ctx2, start, ks, vs)
    _, _, pos, seq = ROPE.reference(whole, cs, ctx2, start, HKV)
    blk, slot = table[seq, pos // T].long(), pos % T
    assert torch.equal(vb[blk, :, :, slot], ref_vb)
    rest_k, rest_v = kb.clone(), vb.clone()
    rest_k[blk, :, slot] = SENT8
    rest_v[blk, :, :, slot] = SENT8
    assert bool((rest_k == SENT8).all()) and bool((rest_v == SENT8).all())
    kd = lg().dequantize_kv8_reference(kb, ks.view(1, HKV, 1, 1))
    vd = lg().dequantize_kv8_reference(vb, vs.view(1, HKV, 1, 1))
    ref = PRE.reference(q_out2.cpu(), kd, vd, table, ctx2, start2)
    inside = torch.zeros(nb, T, dtype=torch.bool)
    inside[blk, slot] = True
    vmax = float(vd.abs()[inside[:, None, None, :].expand(-1, HKV, D, -1)].max())
    bound = ATT.RANDOM_BOUND * vmax
    if regime == "match":
        assert torch.equal(kb[blk, :, slot], ref_kb)                                    # the appends are exact here
        assert torch.equal(q_out2.cpu(), qkv2[:, :HQ])                                  # identity rotation
        x = whole.float()
        assert torch.equal(kd[blk, :, slot].float(), x[:, HQ:HQ + HKV]) and torch.equal(vd[blk, :, :, slot].float(), x[:, HQ + HKV:])
        exact, facts = PRE.exact_expectation("match", GROUP, HKV, SEQS, logical_v)
        assert facts["trap1"] and facts["two"] > 0
        f = exact.float()
        assert torch.equal(f.double(), exact)
        exp = f.to(torch.bfloat16)
        assert torch.equal(ref.float().to(torch.bfloat16), exp)                         # on the reference alone
        assert torch.equal(out.cpu(), exp), (regime, int((out.cpu().float() != exp.float()).sum()))
    else:
        err = float((out.double().cpu() - ref).abs().max())
        differ = int((kb[blk, :, slot] != ref_kb).sum())
        print(f"kv8 prefill chain, random regime: max|out - ref| = {err:.5f} (bound {bound:.5f}); "
              f"{differ} of {ref_kb.numel()} K bytes differ from the reference bytes")
        assert bool(out.float().isfinite().all()) and err <= bound, err
    # the last token of each chunk through the decode reader, on the same caches
    for name, q_out, starts, ctx in (("prefix", q_out1, start1, ctx1), ("chunk", q_out2, start2, ctx2)):
        live = [s for s in range(len(SEQS)) if starts[s + 1] > starts[s]]
        last = torch.tensor([int(starts[s + 1]) - 1 for s in live])
        sel = torch.tensor(live)
        q = q_out[last.cuda()]
        dec = lg().paged_decode_attention_kv8(q, kc, vc, tab[sel.cuda()].contiguous(), ctx[sel].cuda(), **sc)
        dref = ATT.reference(q.cpu(), kd, vd, table[sel], ctx[sel])
        err = float((dec.double().cpu() - dref).abs().max())
        print(f"kv8 prefill chain, {regime}, the {name}'s last tokens through the decode reader: max|out - ref| = {err:.5f} "
              f"(bound {bound:.5f})")
        assert err <= bound, (name, err)
        if name == "chunk":
            gap = float((dec.double() - out[last.cuda()].double()).abs().max())
            print(f"kv8 prefill chain, {regime}: max|decode - prefill| on those rows = {gap:.5f}")
            assert gap <= 2 * bound


# ------------------------------------------------------------------------------------------------
# the two workloads
# ------------------------------------------------------------------------------------------------
WORKLOADS = ["llm_kv8_layer_prefill_2048", "llm_kv8_chunk_prefill_64"]


@pytest.mark.parametrize("workload", WORKLOADS)
def test_podrun_llm_kv8_prefill(workload):
    p = subprocess.run([sys.executable, "-m", "k8s_gpu_scheduler_amd.ops.podrun", "--workload", workload,
                        "--iters", "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    assert res["workload"] == workload and res["iters"] == 2 and res["throughput"] > 0


@pytest.mark.parametrize("workload", WORKLOADS)
def test_executor_llm_kv8_prefill_buffers_and_outputs(workload):
    from k8s_gpu_scheduler_amd.models import workloads as W
    from k8s_gpu_scheduler_amd.parallel import executor as E
    dev = torch.device("cuda", 0)
    w = W.get(workload)
    a = E._Buffers(w, dev)
    (oa, ta), (ot, tt) = a.ops[1], a.ops[2]
    q_out, qkv, cos_sin, kc, vc, table, ctx, q_start, ks, vs = ta
    nb = oa.M * oa.K // T
    cache_bytes = (16 << 20) if workload == WORKLOADS[0] else (1 << 30)
    assert oa.kind == "rope_append_kv8" and E.op_output(oa, ta) is q_out
    assert kc.dtype == vc.dtype == FP8 and kc.shape == (nb, oa.rows, T, D) and vc.shape == (nb, oa.rows, D, T)
    assert kc.numel() + vc.numel() == cache_bytes and not bool(kc.view(U8).any())
    assert ks.dtype == torch.float32 and ks.tolist() == [E.KV8_K_SCALE] * oa.rows and vs.tolist() == [E.KV8_V_SCALE] * oa.rows
    assert qkv.shape == (oa.M * oa.q, oa.N + 2 * oa.rows, D) and cos_sin.shape == (oa.K, D)
    assert torch.equal(table.flatten().sort().values, torch.arange(nb, dtype=torch.int32, device=dev))
    assert len(tt) == 9
    out, q, kc2, vc2, table2, ctx2, q_start2, ks2, vs2 = tt
    assert ot.kind == "prefill_kv8" and E.op_output(ot, tt) is out and kc2.dtype == vc2.dtype == FP8
    assert out.shape == q.shape == (ot.M * ot.q, ot.N, D)
    assert kc2.numel() + vc2.numel() == cache_bytes and kc2.data_ptr() != kc.data_ptr()
    assert not bool(((kc2.view(U8)[:64] & 0x7F) > 0x40).any()) and not bool(((vc2.view(U8)[:64] & 0x7F) > 0x40).any())   # finite, |value| <= 2
    assert bool((ctx2 == ot.K).all()) and q_start2.tolist() == [s * ot.q for s in range(ot.M + 1)]
    assert ks2.tolist() == [E.KV8_K_SCALE] * ot.rows and vs2.tolist() == [E.KV8_V_SCALE] * ot.rows
    kc.view(U8).fill_(SENT8)
    vc.view(U8).fill_(SENT8)
    q_out.view(torch.int16).fill_(0x5A5A)
    out.view(torch.int16).fill_(0x5A5A)
    E.enqueue_ops(a, 1, torch.cuda.current_stream(), 0)
    torch.cuda.synchronize()
    # the append: 8 rows
    M, ql = oa.M, oa.q
    picks = [(0, 0), (M - 1, 0), (M // 2, ql // 2), (M - 1, ql - 1), (0, ql - 1), (M // 3, 1), (M - 2 if M > 2 else 0, 5), (1, ql - 2)]
    assert len(set(picks)) == 8
    rows = torch.tensor([s * ql + i for s, i in picks], device=dev)
    pos = torch.tensor([oa.K - ql + i for _, i in picks], device=dev)
    seq = torch.tensor([s for s, _ in picks], device=dev)
    x = qkv[rows].double().cpu()
    ref = ROPE.rotate(x[:, :oa.N + oa.rows], cos_sin[pos].double().cpu()[:, None, :])
    blk = table[seq, pos // T].long()
    xa = x[:, :oa.N + oa.rows].abs()
    x12 = torch.cat([xa[..., :HALF] + xa[..., HALF:]] * 2, dim=-1)
    err_q = (q_out[rows].double().cpu() - ref[:, :oa.N]).abs()
    assert bool((err_q <= ROPE.TRUE_BOUND * x12[:, :oa.N]).all())
    kcpu, vcpu = kc.view(U8)[blk, :, pos % T].cpu(), vc.view(U8)[blk, :, :, pos % T].cpu()
    z = ref[:, oa.N:] / E.KV8_K_SCALE
    assert float(z.abs().max()) < 448
    err_k = (lg().dequantize_kv8_reference(kcpu, E.KV8_K_SCALE) - ref[:, oa.N:]).abs()
    bound_k = E.KV8_K_SCALE * torch.maximum(2.0 ** -4 * z.abs(), torch.tensor(2.0 ** -10, dtype=torch.float64)) + 2.0 ** -20 * x12[:, oa.N:]
    print(f"{workload} append, 8 rows: K max err / bound = {float((err_k / bound_k).max()):.4f}, "
          f"q_out {float((err_q / (ROPE.TRUE_BOUND * x12[:, :oa.N]).clamp_min(1e-300)).max()):.4f}")
    assert bool((err_k <= bound_k).all())
    assert torch.equal(vcpu, lg().quantize_kv8_reference(qkv[rows, oa.N + oa.rows:].float().cpu() / E.KV8_V_SCALE))
    written = M * ql * oa.rows * D
    assert int((kc.view(U8) != SENT8).sum()) <= written and int((vc.view(U8) != SENT8).sum()) <= written
    assert not bool((q_out.view(torch.int16) == 0x5A5A).all(-1).any())
    # the attention: 8 rows; a picked row at position p is a one-token chunk of a sequence of p + 1 tokens
    M, ql = ot.M, ot.q
    picks = [(0, 0), (0, ql - 1), (M - 1, 0), (M - 1, ql - 1), (M // 2, T - (ot.K - ql) % T if ql > T else 1), (M // 2, ql // 2 + 1),
             (1, 17), (M - 1, ql - 2)]
    assert len(set(picks)) == 8
    worst = 0.0
    one = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    for s, i in picks:
        p = ot.K - ql + i
        ids = table2[s, :p // T + 1].long()
        kd = kc2[ids].to(torch.float32).double() * E.KV8_K_SCALE
        vd = vc2[ids].to(torch.float32).double() * E.KV8_V_SCALE
        local = torch.arange(len(ids), dtype=torch.int32, device=dev)[None, :]
        row = s * ql + i
        ref = PRE.reference(q[row:row + 1], kd, vd, local, torch.tensor([p + 1], dtype=torch.int32, device=dev), one)
        worst = max(worst, float((out[row:row + 1].double() - ref).abs().max()))
        del kd, vd
    bound = ATT.RANDOM_BOUND * E.KV8_V_SCALE * 2.0
    print(f"{workload} attention, 8 rows: max|out - ref| = {worst:.5f} (bound {bound:.5f})")
    assert worst <= bound
    assert not bool((out.view(torch.int16) == 0x5A5A).all(-1).any())
    del a, ta, tt, kc, vc, kc2, vc2
    torch.cuda.empty_cache()
