"""The FP8 paged-KV cache's writer and its two readers in a row (run with `-m gpu` on an MI355X): 8 ragged sequences
are appended with rope_append into float8_e4m3fn caches whose every byte is SENT8 before, then attended with the
decode attention and the split-KV decode attention (2 and 4 splits) on the same caches.  The reference is
ATT.reference (float64) on loadgen.dequantize_kv8_reference of the caches READ BACK from the device, with the scales
applied per KV head, and the device's q_out: whatever the writer stored is what the readers must have seen.

  onehot, pair   identity rotation table (c = 1, s = 0), q = 8 H, K = +-4 H (stored +-16 and +-32 under k_scale =
                 (2^-2, 2^-3)), V = v_scale * (an e4m3fn value of six binades) with v_scale = (4, 2^-3): the append is
                 exact -- the cache bytes are asserted against the operands -- and so is the attention: `torch.equal`
                 after float64 -> fp32 -> bf16.
  random         the true rope_table, q and K randn (k_scale = 1/16), V uniform in [-1, 1] (v_scale = 2^-8: the stored
                 magnitudes reach 256): |out - ref| <= 2^-7 * max|V_deq|, the decode modules' bound.

The deviation of the FP8 chain from the all-bf16 chain on the same inputs (bf16 caches, the same kernels' bf16
siblings) is printed and recorded below; it is NOT asserted: no bound is derived for it -- it is the quantisation
error of K and V, about 2^-4 relative per element, carried through a softmax.

The two LLM_KV8 workloads run through podrun and through the executor, whose buffers are checked and whose append
and attention outputs are spot-checked on 8 rows against the references.
"""
import json
import subprocess
import sys

import pytest
import torch

import test_gpu_decode_attn_exact as ATT
import test_gpu_prefill_attn_exact as PRE
import test_gpu_rope_append_exact as ROPE
from test_gpu_kernels_exact import NAN

pytestmark = pytest.mark.gpu

# MEASURED on an MI355X (printed by the tests):
MEASURED = """
  random regime: max|out - ref| = 0.00133 at 1, 2 and 4 splits (bound 0.00781); 0 of 274,176 K bytes differ from the
  reference bytes.  Deviation of the FP8 chain from the all-bf16 chain (not asserted): 0.03125 of outputs up to 1.0 in
  the random regime, at every split count; 0 in the onehot and pair regimes, whose K and V are e4m3fn values.
  llm_kv8_layer_decode_256: append K 0.9612 and q_out 0.9089 of their bounds on 8 rows, attention max|out - ref| =
  0.00008 (bound 0.00391); llm_kv8_decode_long_8: 0.9772, 0.8928, 0.00004.  The module: 7 tests in 8.7 s, 5 s of them
  the two podrun processes.
"""

D, T, HALF = ATT.D, ATT.T, ROPE.HALF
FP8, U8 = torch.float8_e4m3fn, torch.uint8
SENT8 = 0x5A
GROUP, HKV = 4, 2
HQ, HT = GROUP * HKV, GROUP * HKV + 2 * HKV
CTXS = (257, 33, 64, 290, 129, 1, 97, 200)
SPLITS = (2, 4)


def lg():
    from k8s_gpu_scheduler_amd.ops import loadgen
    return loadgen


def operands(regime, g):
    """(qkv bf16 [sum ctx, Ht, 128] -- every sequence one chunk --, cos_sin, k_scale, v_scale)."""
    if regime == "random":
        x = [torch.cat([torch.randn(c, HQ + HKV, D, generator=g), torch.rand(c, HKV, D, generator=g) * 2 - 1], dim=1) for c in CTXS]
        return torch.cat(x).to(torch.bfloat16), lg().rope_table(max(CTXS)), torch.tensor([1 / 16, 1 / 16]), torch.tensor([2.0 ** -8] * 2)
    ks, vs = torch.tensor([2.0 ** -2, 2.0 ** -3]), torch.tensor([4.0, 2.0 ** -3])
    q, kl, _ = ATT.logical_operands(regime, GROUP, HKV, CTXS, g)                     # q [S, Hq, D]; K per sequence [Hkv, ctx, D]
    rows = []
    for s, c in enumerate(CTXS):
        code = torch.randint(0x18, 0x48, (c, HKV, D), generator=g) | (torch.randint(0, 2, (c, HKV, D), generator=g) << 7)
        v = code.to(U8).view(FP8).float() * vs.view(1, HKV, 1)
        qs = torch.randn(c, HQ, D, generator=g)                                       # earlier tokens' q rows: not attended with
        qs[-1] = q[s]                                                                 # the decode query is the last token's
        rows.append(torch.cat([qs, kl[s].transpose(0, 1), v], dim=1))
    x = torch.cat(rows).to(torch.bfloat16)
    cs = torch.cat([torch.ones(max(CTXS), HALF), torch.zeros(max(CTXS), HALF)], dim=1)
    return x, cs, ks, vs


def attend(q, kc, vc, table, ctx, **sc):
    fn = lg().paged_decode_attention_kv8 if sc else lg().paged_decode_attention
    outs = {1: fn(q, kc, vc, table, ctx, **sc)}
    for k in SPLITS:
        ws = torch.full((lg().decode_split_workspace_floats(len(CTXS), HQ, k),), NAN, device="cuda")
        outs[k] = fn(q, kc, vc, table, ctx, kv_splits=k, workspace=ws, **sc)
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("regime", ["onehot", "pair", "random"])
def test_append_then_attend(regime):
    g = torch.Generator().manual_seed(9700 + len(regime))
    table, nb = PRE.block_tables(CTXS, g)
    qkv, cs, ks, vs = operands(regime, g)
    ctx = torch.tensor(CTXS, dtype=torch.int32)
    q_start = torch.tensor((0,) + CTXS).cumsum(0).to(torch.int32)
    last = (q_start[1:] - 1).long()                                                  # the row of each sequence's last token
    dev = dict(table=table.cuda(), ctx=ctx.cuda())
    kc = torch.full((nb, HKV, T, D), SENT8, dtype=U8, device="cuda").view(FP8)
    vc = torch.full((nb, HKV, D, T), SENT8, dtype=U8, device="cuda").view(FP8)
    sc = dict(k_scale=ks.cuda(), v_scale=vs.cuda())
    q_out = lg().rope_append(qkv.cuda(), cs.cuda(), kc, vc, dev["table"], dev["ctx"], q_start.cuda(), **sc)
    torch.cuda.synchronize()
    kb, vb = kc.view(U8).cpu(), vc.view(U8).cpu()
    ref_kb, ref_vb = lg().rope_append_kv8_reference(qkv, cs, ctx, q_start, ks, vs)
    _, _, pos, seq = ROPE.reference(qkv, cs, ctx, q_start, HKV)
    blk, slot = table[seq, pos // T].long(), pos % T
    assert torch.equal(vb[blk, :, :, slot], ref_vb)
    rest_k, rest_v = kb.clone(), vb.clone()
    rest_k[blk, :, slot] = SENT8
    rest_v[blk, :, :, slot] = SENT8
    assert bool((rest_k == SENT8).all()) and bool((rest_v == SENT8).all())          # nothing but the tokens' slots
    q = q_out[last.cuda()]                                                           # [S, Hq, D]: the decode queries
    kd = lg().dequantize_kv8_reference(kb, ks.view(1, HKV, 1, 1))
    vd = lg().dequantize_kv8_reference(vb, vs.view(1, HKV, 1, 1))
    ref = ATT.reference(q.cpu(), kd, vd, table, ctx)
    outs = attend(q, kc, vc, dev["table"], dev["ctx"], **sc)
    if regime != "random":
        assert torch.equal(kb[blk, :, slot], ref_kb)                                 # the append is exact here
        assert torch.equal(q.cpu(), qkv[last, :HQ])                                  # identity rotation
        x = qkv.float()
        assert torch.equal(kd[blk, :, slot].float(), x[:, HQ:HQ + HKV]) and torch.equal(vd[blk, :, :, slot].float(), x[:, HQ + HKV:])
        f = ref.float()
        big = ref.abs() > 2.0 ** -20
        assert torch.equal(f.double()[big], ref[big])
        exp = f.to(torch.bfloat16)
        for k, out in outs.items():
            assert torch.equal(out.cpu(), exp), (regime, k, int((out.cpu().float() != exp.float()).sum()))
    else:
        inside = torch.zeros(nb, T, dtype=torch.bool)
        inside[blk, slot] = True
        vmax = float(vd.abs()[inside[:, None, None, :].expand(-1, HKV, D, -1)].max())
        differ = int((kb[blk, :, slot] != ref_kb).sum())
        for k, out in outs.items():
            err = float((out.double().cpu() - ref).abs().max())
            print(f"kv8 chain, random regime, kv_splits {k}: max|out - ref| = {err:.5f} (bound {ATT.RANDOM_BOUND * vmax:.5f}); "
                  f"{differ} of {ref_kb.numel()} K bytes differ from the reference bytes")
            assert bool(out.float().isfinite().all()) and err <= ATT.RANDOM_BOUND * vmax, (k, err)
    # the all-bf16 chain on the same inputs: printed, not asserted
    kc16 = torch.zeros((nb, HKV, T, D), dtype=torch.bfloat16, device="cuda")
    vc16 = torch.zeros((nb, HKV, D, T), dtype=torch.bfloat16, device="cuda")
    q16 = lg().rope_append(qkv.cuda(), cs.cuda(), kc16, vc16, dev["table"], dev["ctx"], q_start.cuda())
    assert torch.equal(q16.view(torch.int16), q_out.view(torch.int16))               # q_out does not depend on the cache dtype
    out16 = attend(q16[last.cuda()], kc16, vc16, dev["table"], dev["ctx"])
    for k in outs:
        dev_ = float((outs[k].double() - out16[k].double()).abs().max())
        print(f"kv8 chain, {regime}, kv_splits {k}: max|FP8 chain - bf16 chain| = {dev_:.5f} "
              f"(max|bf16 chain| = {float(out16[k].float().abs().max()):.4f})")


# ------------------------------------------------------------------------------------------------
# the two workloads
# ------------------------------------------------------------------------------------------------
WORKLOADS = ["llm_kv8_layer_decode_256", "llm_kv8_decode_long_8"]


@pytest.mark.parametrize("workload", WORKLOADS)
def test_podrun_llm_kv8(workload):
    p = subprocess.run([sys.executable, "-m", "k8s_gpu_scheduler_amd.ops.podrun", "--workload", workload,
                        "--iters", "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    assert res["workload"] == workload and res["iters"] == 2 and res["throughput"] > 0


@pytest.mark.parametrize("workload", WORKLOADS)
def test_executor_llm_kv8_buffers_and_outputs(workload):
    from k8s_gpu_scheduler_amd.models import workloads as W
    from k8s_gpu_scheduler_amd.parallel import executor as E
    dev = torch.device("cuda", 0)
    w = W.get(workload)
    a = E._Buffers(w, dev)
    (oa, ta), (ot, tt) = a.ops[1], a.ops[2]
    q_out, qkv, cos_sin, kc, vc, table, ctx, q_start, ks, vs = ta
    nb = oa.M * oa.K // T
    assert oa.kind == "rope_append_kv8" and E.op_output(oa, ta) is q_out
    assert kc.dtype == vc.dtype == FP8 and kc.shape == (nb, oa.rows, T, D) and vc.shape == (nb, oa.rows, D, T)
    assert kc.numel() + vc.numel() == 512 << 20 and not bool(kc.view(U8).any())
    assert ks.dtype == torch.float32 and ks.tolist() == [E.KV8_K_SCALE] * oa.rows and vs.tolist() == [E.KV8_V_SCALE] * oa.rows
    assert qkv.shape == (oa.M * oa.q, oa.N + 2 * oa.rows, D) and cos_sin.shape == (oa.K, D)
    assert torch.equal(table.flatten().sort().values, torch.arange(nb, dtype=torch.int32, device=dev))
    out, q, kc2, vc2, table2, ctx2 = tt[:6]
    ks2, vs2 = tt[-2:]
    assert ot.kind == ("attn_kv8" if workload == WORKLOADS[0] else "attn_split_kv8") and E.op_output(ot, tt) is out
    assert len(tt) == (8 if ot.kind == "attn_kv8" else 9) and kc2.dtype == vc2.dtype == FP8
    assert kc2.numel() + vc2.numel() == 512 << 20 and kc2.data_ptr() != kc.data_ptr()
    assert not bool(((kc2.view(U8)[:64] & 0x7F) > 0x40).any()) and not bool(((vc2.view(U8)[:64] & 0x7F) > 0x40).any())   # finite, |value| <= 2
    kc.view(U8).fill_(SENT8)
    vc.view(U8).fill_(SENT8)
    q_out.view(torch.int16).fill_(0x5A5A)
    out.view(torch.int16).fill_(0x5A5A)
    E.enqueue_ops(a, 1, torch.cuda.current_stream(), 0)
    torch.cuda.synchronize()
    # the append: 8 rows
    M, ql = oa.M, oa.q
    picks = [(0, 0), (1, 0), (M // 2, 0), (M - 1, ql - 1), (2, 0), (M // 3, 0), (M - 2, 0), (3, ql - 1)]
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
    # the attention: 8 rows (sequences), the float64 reference on the device, one sequence at a time
    worst = 0.0
    for s in sorted({0, 1, 2, 3, ot.M // 2, ot.M - 3, ot.M - 2, ot.M - 1}):
        ids = table2[s].long()
        kd = kc2[ids].to(torch.float32).double() * E.KV8_K_SCALE
        vd = vc2[ids].to(torch.float32).double() * E.KV8_V_SCALE
        local = torch.arange(len(ids), dtype=torch.int32, device=dev)[None, :]
        ref = ATT.reference(q[s:s + 1], kd, vd, local, ctx2[s:s + 1])
        worst = max(worst, float((out[s:s + 1].double() - ref).abs().max()))
        del kd, vd
    bound = ATT.RANDOM_BOUND * E.KV8_V_SCALE * 2.0
    print(f"{workload} attention, 8 rows: max|out - ref| = {worst:.5f} (bound {bound:.5f})")
    assert worst <= bound
    assert not bool((out.view(torch.int16) == 0x5A5A).all(-1).any())
    del a, ta, tt, kc, vc, kc2, vc2
    torch.cuda.empty_cache()
