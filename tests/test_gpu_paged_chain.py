"""The paged KV cache's one writer and three readers run the way a server runs them (run with `-m gpu` on
an MI355X): 8 sequences are prefilled, then generate 34 tokens one at a time -- rope_append of one token
per sequence into caches whose unwritten slots are NaN, then decode attention, split-KV decode attention
(2 and 4 splits) and one-token prefill attention on the same caches, after every append.  A second pass
captures one append-and-attend step in a graph and replays it 34 times while ctx_lens advances on the
device and the step's qkv is copied into the captured buffer: a value baked at capture, or a missing
writer-to-reader edge inside the graph, shows as a difference from the eager pass.

group 4, two KV heads; prompts PROMPTS = (1, 31, 32, 33, 63, 64, 95, 0): every sequence opens at least one
new cache block during its 34 steps, one starts from an empty context, and the slots 31 and 0 on both
sides of a block boundary are each some sequence's first decode token.  The block table is
PRE.block_tables over the final context lengths; cos_sin is the true rope_table.  q and K are randn, V
uniform in [-1, 1], all rounded to bf16 and drawn up front for every step: no output feeds back, so the
float64 references do not compound.

After every eager step (every launch with check=True):
  * the caches against a host model (HostCache, CPU-tested in test_paged_chain_cpu.py against the rope
    module's expected_caches): V slots bit-equal, K slots within the rope module's TRUE_BOUND * (|x1| + |x2|)
    of the float64 rotation, every other cell still the NaN fill bit for bit;
  * every attention output finite and within RANDOM_BOUND * max|V| (the decode module's derivation; max|score|
    <= SCORE_CAP is asserted on the CPU) of ATT.reference / PRE.reference evaluated on the cache contents
    read back from the device and the device's q_out;
  * one-token prefill against decode: the relation test_chunks_of_one_token_are_the_decode_attention asserts
    -- the one-token chunks meet the decode launch's expectation on its operands, here the decode reference
    under the decode bound (the two float64 references are asserted equal to 1e-12).

After the graph pass: every step's decode and split outputs and the final caches are bit-equal to the eager
pass's, and the caches are still NaN outside the named slots.
"""
import functools

import pytest
import torch

import test_gpu_attn_numeric_edges as EDG
import test_gpu_decode_attn_exact as ATT
import test_gpu_prefill_attn_exact as PRE
import test_gpu_rope_append_exact as ROPE
from test_gpu_kernels_exact import NAN, SENT16

pytestmark = pytest.mark.gpu

# MEASURED on an MI355X (printed by the test):
MEASURED = """
  max|score| = 4.38.  Maxima of |out - ref| / bound over the 35 steps: K slots 0.9746 and q_out 0.9694 (of TRUE_BOUND *
  (|x1| + |x2|)); prompts' prefill attention 0.3682, decode 0.3516, split decode at 2 and at 4 splits 0.3516, one-token
  prefill 0.3516 against either reference (of RANDOM_BOUND * max|V|).  The 34 replays and the final caches were
  bit-equal to the eager pass.  The test: 0.4 s inside the whole suite, 1.1 s alone.
  A float NaN written by a device-side fill of a bf16 tensor is not the host's 0x7FC0: the caches are filled
  through their int16 view.
"""

D, T, HALF = ATT.D, ATT.T, ROPE.HALF
S, GROUP, HKV = 8, 4, 2
HQ, HT = GROUP * HKV, GROUP * HKV + 2 * HKV
PROMPTS = (1, 31, 32, 33, 63, 64, 95, 0)
STEPS = 34
FINAL = tuple(p + STEPS for p in PROMPTS)
MAX_POS = 160
NAN_BITS = int(torch.tensor([NAN]).to(torch.bfloat16).view(torch.int16)[0])
SPLITS = (2, 4)


# ------------------------------------------------------------------------------------------------
# the tokens of every step, and the host model of the cache (CPU-tested in test_paged_chain_cpu.py)
# ------------------------------------------------------------------------------------------------
class Tokens:
    """Everything drawn up front: per sequence x [final ctx, Hq + 2 Hkv, 128] bf16 (q | K | V heads), the
    block table over the final context lengths and the true rope table."""

    def __init__(self, seed=9500):
        from k8s_gpu_scheduler_amd.ops import loadgen
        g = torch.Generator().manual_seed(seed)
        self.table, self.nb = PRE.block_tables(FINAL, g)
        self.x = []
        for c in FINAL:
            qk = torch.randn(c, HQ + HKV, D, generator=g)
            v = torch.rand(c, HKV, D, generator=g) * 2 - 1
            self.x.append(torch.cat([qk, v], dim=1).to(torch.bfloat16))
        self.cs = loadgen.rope_table(MAX_POS)
        assert max(FINAL) <= MAX_POS

    def step(self, k):
        """(qkv [n, Ht, 128] bf16, ctx_lens int32 [S], q_start int32 [S + 1]) of step k: the whole prompts
        for k == 0, then one token per sequence."""
        if k == 0:
            rows, lens = [x[:p] for x, p in zip(self.x, PROMPTS)], list(PROMPTS)
        else:
            rows, lens = [x[p + k - 1:p + k] for x, p in zip(self.x, PROMPTS)], [1] * S
        ctx = torch.tensor([p + k for p in PROMPTS], dtype=torch.int32)
        return torch.cat(rows), ctx, torch.tensor([0] + lens).cumsum(0).to(torch.int32)

    def whole(self):
        """Every sequence as one chunk."""
        return torch.cat(self.x), torch.tensor(FINAL, dtype=torch.int32), torch.tensor((0,) + FINAL).cumsum(0).to(torch.int32)


@functools.lru_cache(maxsize=None)
def tokens():
    return Tokens()


def assert_the_steps_cross_block_boundaries():
    for p in PROMPTS:
        assert p // T < (p + STEPS - 1) // T or p % T == 0                  # a decode token opens a new block
    assert 0 in PROMPTS and len(PROMPTS) == S == 8
    first = {p % T for p in PROMPTS}
    assert {31, 0, 1} <= first                                              # first decode token in slots 31, 0 and 1
    need = sorted(-(-c // T) for c in FINAL)
    assert need[-1] != need[-2]                                             # block_tables requires it


def max_abs_score(tok):
    """max |scale * q . k| over every query of the chain (every token is one, at its own position) and
    every token at or below it, on the float64 rotation."""
    worst = 0.0
    for x in tok.x:
        c = x.shape[0]
        y = ROPE.rotate(x[:, :HQ + HKV].double(), tok.cs[:c].double()[:, None, :])
        q, k = y[:, :HQ].view(c, HKV, GROUP, D), y[:, HQ:]
        sc = torch.einsum("ngcd,tgd->ngct", q, k) * ATT.SCALE
        seen = torch.arange(c)[None, :] <= torch.arange(c)[:, None]
        worst = max(worst, float(sc.abs().masked_fill(~seen[:, None, None, :], 0).max()))
    return worst


class HostCache:
    """What the caches must hold after a sequence of appends: per cell of K the float64 rotation and its
    bound, per cell of V the bits, and which (block, slot) pairs are named.  Everything else is the fill."""

    def __init__(self, tok):
        self.table, nb = tok.table, tok.nb
        self.cs = tok.cs
        self.k = torch.full((nb, HKV, T, D), NAN, dtype=torch.float64)
        self.kbound = torch.zeros(nb, HKV, T, D, dtype=torch.float64)
        self.v = torch.full((nb, HKV, D, T), NAN_BITS, dtype=torch.int16)
        self.named = torch.zeros(nb, T, dtype=torch.bool)

    def append(self, qkv, ctx, q_start):
        """Appends the chunks; returns (the float64 rotated q [n, Hq, 128], its bound)."""
        ref_q, ref_k, pos, seq = ROPE.reference(qkv, self.cs, ctx, q_start, HKV)
        blk, slot = self.table[seq, pos // T].long(), pos % T
        assert bool((pos >= 0).all()) and not bool(self.named[blk, slot].any()), "a slot is appended once"
        xa = qkv[:, :HQ + HKV].double().abs()
        b = ROPE.TRUE_BOUND * (xa[..., :HALF] + xa[..., HALF:])
        b = torch.cat([b, b], dim=-1)
        self.k[blk, :, slot], self.kbound[blk, :, slot] = ref_k, b[:, HQ:]
        self.v[blk, :, :, slot] = ROPE.bits(qkv[:, HQ + HKV:])
        self.named[blk, slot] = True
        return ref_q, b[:, :HQ]

    def masks(self):
        return (self.named[:, None, :, None].expand(-1, HKV, -1, D), self.named[:, None, None, :].expand(-1, HKV, D, -1))

    def check(self, kc_bits, vc_bits, what):
        """The caches (int16, on the CPU) against the model; returns max |K - ref| / bound."""
        nk, nv = self.masks()
        for name, got, named in (("k_cache", kc_bits, nk), ("v_cache", vc_bits, nv)):
            bad = ((got != NAN_BITS) & ~named).nonzero()
            assert not len(bad), (what, name, f"{len(bad)} cells outside the named slots changed, first at "
                                              f"{bad[0].tolist()}: {int(got[tuple(bad[0])]) & 0xFFFF:#06x}")
        assert torch.equal(vc_bits[nv], self.v[nv]), (what, "v_cache")
        err = (kc_bits.view(torch.bfloat16).double() - self.k).abs()[nk]
        assert bool((err <= self.kbound[nk]).all()), (what, "k_cache")
        return float((err / self.kbound[nk].clamp_min(1e-300)).max()) if err.numel() else 0.0

    def vmax(self):
        _, nv = self.masks()
        return float(self.v.view(torch.bfloat16)[nv].float().abs().max()) if bool(nv.any()) else 0.0


# ------------------------------------------------------------------------------------------------
# the two passes
# ------------------------------------------------------------------------------------------------
def nan_caches(nb):
    return (torch.full((nb, HKV, T, D), NAN_BITS, dtype=torch.int16, device="cuda").view(torch.bfloat16),
            torch.full((nb, HKV, D, T), NAN_BITS, dtype=torch.int16, device="cuda").view(torch.bfloat16))


def workspace(kv_splits):
    from k8s_gpu_scheduler_amd.ops import loadgen
    return torch.full((loadgen.decode_split_workspace_floats(S, HQ, kv_splits),), NAN, device="cuda")


def eager_pass(tok):
    """Returns (decode outputs [STEPS, S, Hq, 128] bf16, split-4 outputs, k_cache, v_cache, the model, the
    maxima of |out - ref| / bound by kind)."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    kc, vc = nan_caches(tok.nb)
    model = HostCache(tok)
    cs, table = tok.cs.cuda(), tok.table.cuda()
    one = torch.arange(S + 1, dtype=torch.int32)
    ws = {k: workspace(k) for k in SPLITS}
    worst = {}
    keep = {"decode": [], "split-4": []}

    def note(kind, ratio):
        worst[kind] = max(worst.get(kind, 0.0), ratio)

    def within(kind, out, ref, bound, step):
        got = out.double().cpu()
        assert bool(got.isfinite().all()), (kind, step, "a non-finite output")
        err = float((got - ref).abs().max()) if got.numel() else 0.0
        assert err <= bound, (kind, step, err, bound)
        note(kind, err / bound)

    for step in range(STEPS + 1):
        qkv, ctx, q_start = tok.step(step)
        ctx_d, q_start_d = ctx.cuda(), q_start.cuda()
        q_out = loadgen.rope_append(qkv.cuda(), cs, kc, vc, table, ctx_d, q_start_d)
        ref_q, bound_q = model.append(qkv, ctx, q_start)
        torch.cuda.synchronize()
        kc_cpu, vc_cpu, q_cpu = kc.cpu(), vc.cpu(), q_out.cpu()
        note("K", model.check(ROPE.bits(kc_cpu), ROPE.bits(vc_cpu), step))
        err_q = (q_cpu.double() - ref_q).abs()
        assert bool((err_q <= bound_q).all()), ("q_out", step)
        note("q_out", float((err_q / bound_q.clamp_min(1e-300)).max()))
        bound = ATT.RANDOM_BOUND * model.vmax()
        if step == 0:
            out = loadgen.paged_prefill_attention(q_out, kc, vc, table, ctx_d, q_start_d)
            within("prefill, prompts", out, PRE.reference(q_cpu, kc_cpu, vc_cpu, tok.table, ctx, q_start), bound, step)
            continue
        ref = ATT.reference(q_cpu, kc_cpu, vc_cpu, tok.table, ctx)
        ref_p = PRE.reference(q_cpu, kc_cpu, vc_cpu, tok.table, ctx, one)
        assert float((ref - ref_p).abs().max()) <= 1e-12                    # one-token chunks ARE the decode attention
        dec = loadgen.paged_decode_attention(q_out, kc, vc, table, ctx_d)
        within("decode", dec, ref, bound, step)
        keep["decode"].append(dec)
        for k in SPLITS:
            ws[k].fill_(NAN)
            out = loadgen.paged_decode_attention(q_out, kc, vc, table, ctx_d, kv_splits=k, workspace=ws[k])
            within(f"split-{k}", out, ref, bound, step)
            if k == 4:
                keep["split-4"].append(out)
        pre = loadgen.paged_prefill_attention(q_out, kc, vc, table, ctx_d, one.cuda())
        within("prefill, one token", pre, ref_p, bound, step)
        within("prefill, one token, against the decode reference", pre, ref, bound, step)
    torch.cuda.synchronize()
    return torch.stack(keep["decode"]), torch.stack(keep["split-4"]), kc, vc, model, worst


def graph_pass(tok):
    """Returns (decode outputs [STEPS, S, Hq, 128], split-4 outputs, k_cache, v_cache) of 34 replays of one
    captured step."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    kc, vc = nan_caches(tok.nb)
    cs, table = tok.cs.cuda(), tok.table.cuda()
    qkv, ctx, q_start = tok.step(0)
    ctx_d = ctx.cuda()
    loadgen.rope_append(qkv.cuda(), cs, kc, vc, table, ctx_d, q_start.cuda())       # the post-prompt state, eagerly
    steps = torch.stack([tok.step(k)[0] for k in range(1, STEPS + 1)]).cuda()       # [STEPS, S, Ht, 128]
    one = torch.arange(S + 1, dtype=torch.int32).cuda()
    qkv_buf = torch.empty_like(steps[0])
    q_out = torch.empty((S, HQ, D), dtype=torch.bfloat16, device="cuda")
    out_d, out_s = torch.empty_like(q_out), torch.empty_like(q_out)
    got_d = torch.empty((STEPS, S, HQ, D), dtype=torch.bfloat16, device="cuda")
    got_s = torch.empty_like(got_d)
    ws = workspace(4)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        loadgen.rope_append(qkv_buf, cs, kc, vc, table, ctx_d, one, max_q_len=1, q_out=q_out, stream=st, check=False)
        loadgen.paged_decode_attention(q_out, kc, vc, table, ctx_d, out=out_d, stream=st, check=False)
        loadgen.paged_decode_attention(q_out, kc, vc, table, ctx_d, out=out_s, stream=st, check=False, kv_splits=4,
                                       workspace=ws)
    with torch.cuda.stream(st):
        for k in range(STEPS):
            qkv_buf.copy_(steps[k])
            ctx_d.add_(1)
            out_d.view(torch.int16).fill_(SENT16)
            out_s.view(torch.int16).fill_(SENT16)
            ws.fill_(NAN)
            g.replay()
            got_d[k].copy_(out_d)
            got_s[k].copy_(out_s)
    st.synchronize()
    assert ctx_d.tolist() == list(FINAL)
    return got_d, got_s, kc, vc


def test_generation_chain_eager_and_replayed():
    tok = tokens()
    assert_the_steps_cross_block_boundaries()
    cap = max_abs_score(tok)
    assert cap <= EDG.SCORE_CAP, cap
    dec, split, kc, vc, model, worst = eager_pass(tok)
    assert bool(model.named.sum() == sum(FINAL))
    print(f"generation chain, {STEPS} steps, max|score| = {cap:.2f}; max |out - ref| / bound: "
          + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    g_dec, g_split, g_kc, g_vc = graph_pass(tok)
    bits = ROPE.bits
    for name, a, b in (("decode", dec, g_dec), ("split-4", split, g_split)):
        same = (bits(a) == bits(b)).flatten(1).all(1)
        assert bool(same.all()), (name, "replays differ from the eager steps", (~same).nonzero().flatten().tolist())
    assert torch.equal(bits(kc), bits(g_kc)) and torch.equal(bits(vc), bits(g_vc)), "the replayed caches differ"
    nk, nv = model.masks()
    assert bool((bits(g_kc).cpu()[~nk] == NAN_BITS).all()) and bool((bits(g_vc).cpu()[~nv] == NAN_BITS).all())
