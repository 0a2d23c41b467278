"""CPU-only tests of the builders of test_gpu_paged_chain.py: the host model of the cache against the rope
module's expected_caches on the same tokens fed as one whole-sequence chunk per sequence, the step-by-step
model against the whole one, and what the prompts and the scores are claimed to cover."""
import pytest
import torch

import test_gpu_attn_numeric_edges as EDG
import test_gpu_paged_chain as C
import test_gpu_rope_append_exact as ROPE
from test_gpu_kernels_exact import SENT16


def whole_model():
    tok = C.tokens()
    m = C.HostCache(tok)
    ref_q, bound_q = m.append(*tok.whole())
    return tok, m, ref_q, bound_q


def test_host_cache_model_is_expected_caches_on_whole_sequences():
    tok, m, ref_q, bound_q = whole_model()
    qkv, ctx, q_start = tok.whole()
    want_q, ref_k, pos, seq = ROPE.reference(qkv, tok.cs, ctx, q_start, C.HKV)
    assert torch.equal(ref_q, want_q) and ref_q.shape == bound_q.shape == (sum(C.FINAL), C.HQ, C.D)
    exp_kc, exp_vc, _, _ = ROPE.expected_caches(tok.nb, C.HKV, ROPE.bits(ref_k.float().to(torch.bfloat16)),
                                                ROPE.bits(qkv[:, C.HQ + C.HKV:]), pos, seq, tok.table)
    nk, nv = m.masks()
    assert int(m.named.sum()) == sum(C.FINAL) and int(nk.sum()) == int(nv.sum()) == sum(C.FINAL) * C.HKV * C.D
    sent = torch.tensor(SENT16, dtype=torch.int16)
    assert torch.equal(torch.where(nv, m.v, sent), exp_vc)
    assert torch.equal(torch.where(nk, ROPE.bits(m.k.float().to(torch.bfloat16)), sent), exp_kc)
    assert bool((m.v[~nv] == C.NAN_BITS).all()) and bool(m.k[~nk].isnan().all()) and bool(m.k[nk].isfinite().all())
    # the bound is the rope module's, on the token's own K head
    x = qkv[:, C.HQ:C.HQ + C.HKV].double().abs()
    b = ROPE.TRUE_BOUND * (x[..., :C.HALF] + x[..., C.HALF:])
    blk, slot = tok.table[seq, pos // C.T].long(), pos % C.T
    assert torch.equal(m.kbound[blk, :, slot], torch.cat([b, b], dim=-1))
    # the model accepts the bf16 rounding of its own K and refuses a neighbour's slot, a changed fill and a V bit
    kc, vc = torch.where(nk, ROPE.bits(m.k.float().to(torch.bfloat16)), torch.tensor(C.NAN_BITS, dtype=torch.int16)), m.v.clone()
    assert 0.0 < m.check(kc, vc, "own rounding") <= 1.0
    for breakage in ("fill", "v", "k"):
        k2, v2 = kc.clone(), vc.clone()
        if breakage == "fill":
            k2[(~nk).nonzero()[0].unbind()] = 0
        elif breakage == "v":
            v2[nv.nonzero()[5].unbind()] ^= 1
        else:
            i = nk.nonzero()[7]
            k2[i.unbind()] = ROPE.bits((m.k[i.unbind()] + 1.0).float().to(torch.bfloat16).reshape(1))[0]
        with pytest.raises(AssertionError):
            m.check(k2, v2, breakage)


def test_step_by_step_appends_build_the_whole_model():
    tok, whole, _, _ = whole_model()
    m = C.HostCache(tok)
    seen = 0
    for k in range(C.STEPS + 1):
        qkv, ctx, q_start = tok.step(k)
        assert ctx.tolist() == [p + k for p in C.PROMPTS] and qkv.shape[0] == (sum(C.PROMPTS) if k == 0 else C.S)
        m.append(qkv, ctx, q_start)
        seen += qkv.shape[0]
        assert int(m.named.sum()) == seen
    assert torch.equal(m.named, whole.named) and torch.equal(m.v, whole.v)
    assert torch.equal(m.k.nan_to_num(7.0), whole.k.nan_to_num(7.0)) and torch.equal(m.kbound, whole.kbound)
    with pytest.raises(AssertionError, match="appended once"):
        m.append(*tok.step(C.STEPS))


def test_the_chain_covers_what_it_claims():
    C.assert_the_steps_cross_block_boundaries()
    assert C.PROMPTS == (1, 31, 32, 33, 63, 64, 95, 0) and C.STEPS == 34 and (C.GROUP, C.HKV, C.S) == (4, 2, 8)
    tok = C.tokens()
    worst = C.max_abs_score(tok)
    print(f"generation chain: max|score| = {worst:.3f}")
    assert 2.0 < worst <= EDG.SCORE_CAP
    vmax = max(float(x[:, C.HQ + C.HKV:].float().abs().max()) for x in tok.x)
    assert vmax <= 1.0 and all(bool(x.float().isfinite().all()) for x in tok.x)
    assert tok.cs.shape == (C.MAX_POS, C.D) and tok.cs.dtype == torch.float32
