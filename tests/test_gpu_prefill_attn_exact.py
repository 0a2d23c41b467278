"""Exact-arithmetic, guarded-buffer tests of the paged-KV prefill (append) attention (run with `-m gpu`
on an MI355X), in the style of test_gpu_decode_attn_exact.py, whose block-table and cache builders
are used, and of test_gpu_kernels_exact.py, whose guard helpers and sentinels are used.

A launch holds 8 sequences given as (ctx, q_len): the chunk of a sequence is its last q_len tokens,
query i of it has position p = ctx - q_len + i and attends tokens [0, p].  SEQS_A (one KV head) and
SEQS_B (two) hold ctx == q_len (no prefix), q_len == 1 (decode), q_len == 0 (an empty chunk, also
with ctx == 0), chunks that start and end inside a block, and chunks of more than 128 columns
(several workgroups) at every group size.  All ctx are at most 256.

Three value regimes make the result independent of the summation order and of the accuracy of exp;
the comparison is `torch.equal`:

  match    K of token t is 4 H[t % 128], H the 128 x 128 Sylvester-Hadamard sign matrix, for every KV
           head; V is k / 64, |k| <= 255, random per (KV head, token); q of column (chunk token i,
           head h) is 8 H[(p - d) % 128], d = DELTAS[(h + i) % len(DELTAS)] reduced mod p + 1 (the
           entry P stands for p itself: token 0), so that every head meets every entry.  The
           column's matches are the tokens t <= p with t = p - d (mod 128): one or two, because
           ctx <= 256.  A matched score is 4096 * scale = 362 and every other score 0, so the
           probabilities are exactly 1 or 1/2 and 0 (exp(-362) is below fp32's range) and out is
           V[t] or bf16((V[t1] + V[t2]) / 2).  Tokens with the matched sign row at t > p are traps:
           a kernel that leaks a future token averages a wrong V in.  d = 0 is the diagonal; d = 127
           has the sign row of token p + 1, the nearest future token; d = 0 and 128 that of token
           p + 128.  Asserted on the reference alone: every column has 1 or 2 matches, every launch
           has a column with a trap at p + 1, every launch of SEQS_B one with a trap at p + 128
           (SEQS_A has no position with p + 128 < ctx: that needs a chunk of more than 128 tokens
           in front of 128 more, and its longest chunk is 65), some expected value is a bf16
           rounding tie, and the float64 softmax reference below, rounded float64 -> fp32 -> bf16,
           equals the exact mean in every column.
  uniform  q = 0, K random, V integers in [-4, 4]: every probability of a column is 1 / (p + 1) and
           out = bf16(fp32(sum_{t <= p} V) / fp32(p + 1)), the fp32 IEEE quotient taken in torch on
           the CPU from the exact cumulative sums -- exact for every position under the kernel's
           numeric contract (the sum and the count are exact, one IEEE division, one rounding).  The
           float64 softmax is not used as the expectation here: it returns about 1e-17 where the
           exact sum is 0.  That the two agree wherever the exact sum is nonzero is asserted on the
           reference alone.  An off-by-one in the causal limit shows at every position.
  random   q and K randn, V uniform in [-1, 1], all rounded to bf16: |out - ref| <= 2^-7 max|V|, the
           decode module's RANDOM_BOUND, whose derivation holds unchanged under the same numeric
           contract.  The measured maximum is printed; on an MI355X it was 0.00301 over these shapes
           (MEASURED below).

Every launch runs guarded: q is a window (token stride Hq * 128 + 8, column offset 8) of a NaN-filled
allocation and holds LEAD NaN rows before q_start[0] and TRAIL after q_start[S]; out is a window of
the same shape in a SENT16-filled allocation that is compared bitwise afterwards, the rows of the
window outside [q_start[0], q_start[S]) included; the cache blocks no table entry names are NaN, and
so are the slots past ctx of each sequence's last block, in K and in V; the table entries at or
beyond ceil(ctx / 32) hold SENT32; block_table, ctx_lens and q_start start one element into
SENT32-filled allocations.
"""
import functools
import json
import subprocess
import sys

import pytest
import torch

import test_gpu_corun_exact as CO
import test_gpu_decode_attn_exact as ATT
from test_gpu_kernels_exact import NAN, SENT16, SENT32, guarded_input, guarded_output, guards_intact

pytestmark = pytest.mark.gpu

# MEASURED on an MI355X (printed by the tests):
MEASURED = """
  random regime, max|out - ref| per (group, KV heads): 0.00234 .. 0.00301, the largest at (16, 2), against the
  bound 0.00781 (max|V| = 1.0); llm_prefill_2048 attention, 8 picked rows: 0.00063 against 0.01550.
  Co-run (4 launches per victim): the victim's slowdown 0.57 .. 1.44, and 5.3 / 7.2 on the stream aggressor's
  own 32 CUs; every output bit-exact.  The module: 52 tests in 7 s.
  Reference alone, over the 35,743 columns of the match cases: the float64 softmax rounded
  float64 -> fp32 -> bf16 equals the exact mean in every column; 10,876 columns have two matches.
"""

D, T, SCALE, C0 = ATT.D, ATT.T, ATT.SCALE, ATT.C0
R0 = 2                      # guard rows in front of the q and out windows (guarded_input / guarded_output)
LEAD, TRAIL = 3, 2          # rows of the windows before q_start[0] and after q_start[S]
SEQS_A = ((1, 1), (32, 32), (33, 33), (97, 40), (256, 1), (64, 0), (130, 65), (200, 7))
SEQS_B = ((256, 256), (255, 100), (31, 31), (65, 2), (0, 0), (129, 1), (96, 64), (160, 33))
P = -1                      # the DELTAS entry that stands for p itself
DELTAS = (0, 127, 1, 31, 32, 33, P, 64, 128, 129, 200, 2, 95, 96, 160, 255, 126)
GROUPS = (1, 2, 4, 8, 16)
SHAPES = [(group, hkv) for group in GROUPS for hkv in (1, 2)]
REGIMES = ("match", "uniform", "random")
RANDOM_BOUND = ATT.RANDOM_BOUND
COLUMNS = 128               # query columns per workgroup


@pytest.fixture(scope="module")
def hip():
    from k8s_gpu_scheduler_amd import _native
    return _native.hip(required=True)


# ------------------------------------------------------------------------------------------------
# the float64 reference (also imported by test_prefill_attn_cpu.py)
# ------------------------------------------------------------------------------------------------
def reference(q, k_cache, v_cache, block_table, ctx_lens, q_start, scale=SCALE):
    """float64 [Tq, Hq, D]: per sequence, the tokens [0, ctx) gathered through the block table --
    nothing else of the caches or the table is looked at -- and for the chunk's rows of q a softmax
    over the tokens at or below each row's position, then the weighted sum of their V rows.  Rows
    of no chunk are zeros."""
    Tq, Hq, _ = q.shape
    Hkv = k_cache.shape[1]
    out = torch.zeros(Tq, Hq, D, dtype=torch.float64, device=q.device)
    starts = q_start.tolist()
    for s, ctx in enumerate(ctx_lens.tolist()):
        r0, r1 = starts[s], starts[s + 1]
        n = r1 - r0
        if n == 0:
            continue
        blocks = block_table[s, :-(-ctx // T)].long()
        k = k_cache[blocks].double().permute(1, 0, 2, 3).reshape(Hkv, -1, D)[:, :ctx]            # [Hkv, ctx, D]
        v = v_cache[blocks].double().permute(1, 0, 3, 2).reshape(Hkv, -1, D)[:, :ctx]
        qs = q[r0:r1].double().view(n, Hkv, Hq // Hkv, D)
        sc = torch.einsum("ngcd,gtd->ngct", qs, k) * scale
        pos = ctx - n + torch.arange(n, device=q.device)
        above = torch.arange(ctx, device=q.device)[None, :] > pos[:, None]                        # [n, ctx]
        p = torch.softmax(sc.masked_fill(above[:, None, None, :], float("-inf")), dim=-1)
        out[r0:r1] = torch.einsum("ngct,gtd->ngcd", p, v).reshape(n, Hq, D)
    return out


# ------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------
def match_columns(ctx, n, Hq):
    """Per column (chunk token i, head h) of a sequence: the position p [n, 1], the first match
    t1 [n, Hq] (always at or below p), the second t2 = t1 + 128 and whether it is at or below p."""
    i = torch.arange(n)[:, None]
    p = ctx - n + i
    d = torch.tensor(DELTAS)[(torch.arange(Hq)[None, :] + i) % len(DELTAS)]
    d = torch.where(d == P, p.expand_as(d), d) % (p + 1)
    t1 = (p - d) % 128
    assert bool((t1 <= p - d).all()) and bool((t1 + 256 > p).all())          # never a third match
    return p, t1, t1 + 128, t1 + 128 <= p


def logical_operands(regime, group, hkv, seqs, g):
    """q [sum q_len, Hq, D] and per sequence K, V [Hkv, ctx, D] as fp32 tensors of bf16 values."""
    Hq = group * hkv
    H = ATT.hadamard()
    n_all = sum(n for _, n in seqs)
    if regime == "random":
        q = torch.randn(n_all, Hq, D, generator=g).to(torch.bfloat16).float()
        ks = [torch.randn(hkv, c, D, generator=g).to(torch.bfloat16).float() for c, _ in seqs]
        vs = [(torch.rand(hkv, c, D, generator=g) * 2 - 1).to(torch.bfloat16).float() for c, _ in seqs]
        return q, ks, vs
    if regime == "uniform":
        q = torch.zeros(n_all, Hq, D)
        ks = [torch.randn(hkv, c, D, generator=g).to(torch.bfloat16).float() for c, _ in seqs]
        vs = [torch.randint(-4, 5, (hkv, c, D), generator=g).float() for c, _ in seqs]
        return q, ks, vs
    ks = [(4 * H[torch.arange(c) % 128])[None].repeat(hkv, 1, 1) for c, _ in seqs]
    vs = [torch.randint(-255, 256, (hkv, c, D), generator=g).float() / 64 for c, _ in seqs]
    q = torch.cat([8 * H[match_columns(c, n, Hq)[1]] for c, n in seqs if n])
    return q, ks, vs


def exact_expectation(regime, group, hkv, seqs, vs):
    """float64 [sum q_len, Hq, D] without a softmax, and for `match` the facts asserted on it."""
    Hq = group * hkv
    kv = torch.arange(Hq) // group
    rows, facts = [], {"trap1": False, "trap128": False}
    for (ctx, n), v in zip(seqs, vs):
        if n == 0:
            continue
        v = v.double()
        if regime == "uniform":
            sums = v.cumsum(1)[:, ctx - n:]                                   # [Hkv, n, D], exact
            assert torch.equal(sums.float().double(), sums)
            count = torch.arange(ctx - n + 1, ctx + 1, dtype=torch.float32)
            rows.append((sums.float() / count[None, :, None]).double()[kv].transpose(0, 1))
            continue
        p, t1, t2, two = match_columns(ctx, n, Hq)
        v1 = v[kv[None, :], t1]                                               # [n, Hq, D]
        v2 = v[kv[None, :], t2.clamp_max(ctx - 1)]
        rows.append(torch.where(two[:, :, None], (v1 + v2) / 2, v1))
        facts["trap1"] |= bool(((p + 1 < ctx) & ((p + 1) % 128 == t1)).any())
        facts["trap128"] |= bool(((p + 128 < ctx) & (p % 128 == t1)).any())
        facts["two"] = facts.get("two", 0) + int(two.sum())
    return torch.cat(rows), facts


def block_tables(ctxs, g):
    """ATT.block_tables.  It interleaves the two longest sequences' blocks and asserts that the
    longer one's ids enclose the other's first, which needs them to differ in length: where they
    tie (SEQS_B: 256 and 255 tokens), the first is dealt one block more, and that entry is then
    taken out of its row again -- one more block that no entry names."""
    need = [-(-c // T) for c in ctxs]
    a, b = sorted(range(len(ctxs)), key=lambda s: -need[s])[:2]
    if need[a] != need[b]:
        return ATT.block_tables(ctxs, g)
    table, nb = ATT.block_tables(tuple(c + T * (s == a) for s, c in enumerate(ctxs)), g)
    table[a, need[a]] = SENT32
    return table, nb


def guarded_ints(t):
    """(raw, view): the int32 vector t starting one element into a SENT32-filled allocation."""
    raw = torch.full((1 + t.numel() + 3,), SENT32, dtype=torch.int32, device="cuda")
    view = raw[1:1 + t.numel()]
    view.copy_(t)
    return raw, view


class Case:
    def __init__(self, regime, group, hkv, seqs, seed):
        g = torch.Generator().manual_seed(seed)
        self.regime, self.S, self.Hq, self.hkv, self.seqs = regime, len(seqs), group * hkv, hkv, seqs
        ctxs = tuple(c for c, _ in seqs)
        self.n = sum(n for _, n in seqs)
        self.Tq = LEAD + self.n + TRAIL
        table, nb = block_tables(ctxs, g)
        q, ks, vs = logical_operands(regime, group, hkv, seqs, g)
        kc, vc = ATT.paged_caches(ks, vs, table, nb, hkv)
        ctx = torch.tensor(ctxs, dtype=torch.int32)
        q_start = torch.tensor([LEAD] + [n for _, n in seqs]).cumsum(0).to(torch.int32)
        assert int(q_start[0]) == LEAD > 0 and int(q_start[-1]) == self.Tq - TRAIL
        qfull = torch.full((self.Tq, self.Hq, D), NAN)
        qfull[LEAD:LEAD + self.n] = q
        qb = qfull.to(torch.bfloat16)
        assert torch.equal(qb[LEAD:LEAD + self.n].float(), q)                      # the operands are exact
        self.ref = reference(qb, kc, vc, table, ctx, q_start)[LEAD:LEAD + self.n]
        assert bool(self.ref.isfinite().all())
        self.vmax = max([float(v.abs().max()) for v in vs if v.numel()] + [0.0])
        self.NB, self.max_blocks, self.max_q_len = nb, table.shape[1], max(n for _, n in seqs)
        W = self.W = self.Hq * D
        self.q = guarded_input(qb.view(self.Tq, W).cuda(), W + C0, c0=C0).unflatten(1, (self.Hq, D))
        self.kc, self.vc = kc.cuda(), vc.cuda()
        self.table_raw, self.table = ATT.guarded_ints_2d(table, self.max_blocks + 2)
        self.ctx_raw, self.ctx = guarded_ints(ctx)
        self.q_start_raw, self.q_start = guarded_ints(q_start)
        self.raw, self.out = self.new_output()
        assert self.q.data_ptr() % 16 == 0 and self.out.data_ptr() % 16 == 0 and self.q.stride(0) == W + C0
        if regime != "random":
            exact, facts = exact_expectation(regime, group, hkv, seqs, vs)
            f = exact.float()
            if regime == "match":
                assert facts["trap1"] and facts["two"] > 0 and (facts["trap128"] or seqs is SEQS_A), facts
                assert torch.equal(f.double(), exact)
                assert bool(((f.view(torch.int32) & 0xFFFF) == 0x8000).any()), "no tie in the expectation"
                assert torch.equal(self.ref.float().to(torch.bfloat16), f.to(torch.bfloat16))     # softmax == exact mean
            else:
                nz = exact != 0
                assert torch.equal(self.ref.float().to(torch.bfloat16)[nz], f.to(torch.bfloat16)[nz])
            self.exp = f.to(torch.bfloat16).cuda()

    def new_output(self):
        """(raw, out): a [Tq, Hq, D] window for the kernel in a SENT16-filled allocation of its own."""
        raw, out2d = guarded_output(self.Tq, self.W, self.W + C0, C0, "cuda")
        return raw, out2d.unflatten(1, (self.Hq, D))

    def resentinel(self):
        self.raw.fill_(SENT16)

    def launch(self, out, **kw):
        from k8s_gpu_scheduler_amd.ops import loadgen
        return loadgen.paged_prefill_attention(self.q, self.kc, self.vc, self.table, self.ctx, self.q_start, out=out, **kw)

    def run(self, **kw):
        return self.launch(self.out, **kw)

    def check(self, what, raw=None, out=None):
        raw, out = (self.raw, self.out) if raw is None else (raw, out)
        torch.cuda.synchronize()
        written = (slice(R0 + LEAD, R0 + LEAD + self.n), slice(C0, C0 + self.W))
        assert guards_intact(raw, written, SENT16), ("write outside the chunks' rows", what)
        got = out[LEAD:LEAD + self.n]
        if self.regime == "random":
            err = (got.double().cpu() - self.ref).abs().max().item()
            print(f"prefill attention, random regime {what}: max|out - ref| = {err:.5f} "
                  f"(bound {RANDOM_BOUND * self.vmax:.5f}, max|V| = {self.vmax:.4f})")
            assert err <= RANDOM_BOUND * self.vmax, (what, err)
            return
        if not torch.equal(got, self.exp):
            bad = (got.float() != self.exp.float()).nonzero()
            r, h, d = bad[0].tolist()
            raise AssertionError((what, f"{len(bad)} elements differ, first at chunk row {r}, head {h}, d {d}: "
                                        f"got {got[r, h, d].item()}, expected {self.exp[r, h, d].item()}"))

    def untouched(self):
        torch.cuda.synchronize()
        return guards_intact(self.raw, (slice(0, 0), slice(0, 0)), SENT16)


@functools.lru_cache(maxsize=None)
def case(regime, group, hkv):
    return Case(regime, group, hkv, SEQS_A if hkv == 1 else SEQS_B, seed=5000 + 1000 * REGIMES.index(regime) + 10 * group + hkv)


# ------------------------------------------------------------------------------------------------
# 1. the regimes over every group size
# ------------------------------------------------------------------------------------------------
def test_the_cases_cover_the_chunk_shapes():
    for seqs in (SEQS_A, SEQS_B):
        assert len(seqs) == 8 and all(0 <= n <= c <= 256 for c, n in seqs)
        assert any(n == 0 for _, n in seqs) and any(n == 1 < c for c, n in seqs) and any(n == c > T for c, n in seqs)
        assert any((c - n) % T and c % T for c, n in seqs if n)                # a chunk that starts and ends inside a block
    assert max(n for _, n in SEQS_A) <= COLUMNS < 2 * max(n for _, n in SEQS_A)      # one column tile at group 1, two at 2
    assert max(n for _, n in SEQS_B) > COLUMNS                                        # two tiles already at group 1
    assert {0, 127, 1, 31, 32, 33, P, 64, 128, 129, 200} <= set(DELTAS)


@pytest.mark.parametrize("group,hkv", SHAPES)
@pytest.mark.parametrize("regime", REGIMES)
def test_regimes(hip, regime, group, hkv):
    c = case(regime, group, hkv)
    c.resentinel()
    c.run()
    c.check((regime, group, hkv))


@pytest.mark.parametrize("name,group,hkv", [("pair", 4, 2), ("uniform", 8, 1)])
def test_chunks_of_one_token_are_the_decode_attention(name, group, hkv):
    """q_len == 1 wherever ctx > 0 (0 where ctx == 0): the decode case's expectation, on its operands."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    a = ATT.case(name, group, hkv)
    live = torch.tensor([c > 0 for c in a.ctxs])
    q_start = torch.cat([torch.zeros(1, dtype=torch.int64), live.long().cumsum(0)]).to(torch.int32).cuda()
    n, W = int(live.sum()), a.Hq * D
    q = guarded_input(a.q[live.cuda()].reshape(n, W), W + C0, c0=C0).unflatten(1, (a.Hq, D))
    raw, out2d = guarded_output(n, W, W + C0, C0, "cuda")
    out = loadgen.paged_prefill_attention(q, a.kc, a.vc, a.table, a.ctx, q_start, out=out2d.unflatten(1, (a.Hq, D)))
    torch.cuda.synchronize()
    assert guards_intact(raw, (slice(R0, R0 + n), slice(C0, C0 + W)), SENT16)
    assert torch.equal(out, a.exp[live.cuda()]), (name, int((out.float() != a.exp[live.cuda()].float()).sum()))


def test_no_check_and_a_larger_max_q_len_give_the_same():
    c = case("match", 4, 2)
    for kw in (dict(check=False, max_q_len=c.max_q_len), dict(check=False, max_q_len=c.max_q_len + 3 * COLUMNS + 5),
               dict(max_q_len=c.max_q_len + 1000)):
        c.resentinel()
        c.run(**kw)
        c.check(kw)


# ------------------------------------------------------------------------------------------------
# 2. check=True stops bad operands on the host
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("breakage", ["block-NB", "block-minus-1", "ctx-past-table", "q_len-above-ctx",
                                      "q_start-decreasing", "max_q_len-too-small"])
def test_check_raises_and_launches_nothing(breakage):
    from k8s_gpu_scheduler_amd.ops import loadgen
    c = case("match", 4, 1)
    s = [x[0] for x in c.seqs].index(256)
    table, ctx, q_start, kw = c.table.clone(), c.ctx.clone(), c.q_start.clone(), {}
    if breakage == "block-NB":
        table[s, 7] = c.NB                       # the sequence's last named entry
    elif breakage == "block-minus-1":
        table[s, 0] = -1
    elif breakage == "ctx-past-table":
        ctx[s] = T * c.max_blocks + 1
    elif breakage == "q_len-above-ctx":
        ctx[c.seqs.index((33, 33))] = 32
    elif breakage == "q_start-decreasing":
        q_start[3] = q_start[2] - 1
    else:
        kw["max_q_len"] = c.max_q_len - 1
    c.resentinel()
    with pytest.raises(ValueError):
        loadgen.paged_prefill_attention(c.q, c.kc, c.vc, table, ctx, q_start, out=c.out, **kw)
    assert c.untouched()


# ------------------------------------------------------------------------------------------------
# 3. side stream and graph replay
# ------------------------------------------------------------------------------------------------
def test_side_stream_and_graph_replay():
    c = case("match", 8, 1)
    s = torch.cuda.Stream()
    c.resentinel()
    torch.cuda.synchronize()
    c.run(stream=s)
    s.synchronize()
    c.check("side stream")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        c.run(stream=s, check=False, max_q_len=c.max_q_len)
    for k in range(2):
        c.resentinel()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        s.synchronize()
        c.check(("replay", k))


# ------------------------------------------------------------------------------------------------
# 4. the grid rule
# ------------------------------------------------------------------------------------------------
def test_workgroups_match_the_python_rule(hip):
    from k8s_gpu_scheduler_amd.models import workloads as W
    for S, hq, hkv, mq in ((1, 1, 1, 1), (8, 8, 2, 33), (2, 32, 8, 1024), (16, 128, 8, 128), (3, 16, 1, 9), (5, 4, 4, 0)):
        assert hip.paged_prefill_workgroups(S, hq, hkv, mq) == W.default_prefill_workgroups(S, hq, hkv, mq)
    assert hip.paged_prefill_workgroups(2, 32, 8, 1024) == 2 * 8 * 32


# ------------------------------------------------------------------------------------------------
# 5. beside a co-running load
# ------------------------------------------------------------------------------------------------
class PrefillLaunch:
    """One launch on a Case's inputs into an output of its own (reset / enqueue / check, as the
    co-run module's CaseLaunch has)."""

    def __init__(self, c, what):
        self.case, self.what = c, what
        self.raw, self.out = c.new_output()

    def reset(self):
        self.raw.fill_(SENT16)

    def enqueue(self, st):
        self.case.launch(self.out, stream=st, check=False, max_q_len=self.case.max_q_len)

    def check(self, tag):
        self.case.check((tag, self.what), self.raw, self.out)


@pytest.mark.parametrize("aggressor,mode", [pytest.param(a, m, id=f"{a}-{m}") for a, m in CO.BASE_PAIRS])
@pytest.mark.parametrize("regime,group,hkv", [("match", 4, 2), ("uniform", 8, 1)])
def test_prefill_attention_corun(hip, regime, group, hkv, aggressor, mode):
    c = case(regime, group, hkv)
    victim = CO.Load(f"prefill-{regime}", {}, [PrefillLaunch(c, (regime, group, hkv, r)) for r in range(CO.R)])
    try:
        CO.corun(hip, victim, CO.aggressor_for(aggressor, mode), mode)
    finally:
        CO.restore_knobs(hip)


# ------------------------------------------------------------------------------------------------
# 6. pod path
# ------------------------------------------------------------------------------------------------
def test_podrun_llm_prefill():
    p = subprocess.run([sys.executable, "-m", "k8s_gpu_scheduler_amd.ops.podrun", "--workload", "llm_prefill_2048",
                        "--iters", "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    assert res["workload"] == "llm_prefill_2048" and res["iters"] == 2 and res["throughput"] > 0


def test_executor_llm_prefill_buffers_and_attention_output():
    """The executor's operands are reproducible, and one iteration's attention output is within the
    random-regime bound of the float64 reference on 4 query rows per sequence: the chunk's first and
    last, the first whose diagonal sits in a new block, and one mid-chunk."""
    from k8s_gpu_scheduler_amd.models import workloads as W
    from k8s_gpu_scheduler_amd.parallel.executor import _Buffers, enqueue_ops
    dev = torch.device("cuda", 0)
    w = W.get("llm_prefill_2048")
    a, b = _Buffers(w, dev), _Buffers(w, dev)
    o, (out, q, kc, vc, table, ctx, q_start) = a.ops[1]
    _, (_, q_b, kc_b, vc_b, table_b, ctx_b, q_start_b) = b.ops[1]
    nb = o.M * o.K // T
    assert o.kind == "prefill" and q.shape == out.shape == (o.M * o.q, o.N, D)
    assert kc.shape == (nb, o.rows, T, D) and vc.shape == (nb, o.rows, D, T) and (kc.numel() + vc.numel()) * 2 == 32 << 20
    assert torch.equal(q.view(torch.int16), q_b.view(torch.int16)) and torch.equal(table, table_b)
    assert torch.equal(ctx, ctx_b) and torch.equal(q_start, q_start_b)
    assert torch.equal(kc.view(torch.int16), kc_b.view(torch.int16)) and torch.equal(vc.view(torch.int16), vc_b.view(torch.int16))
    assert torch.equal(table.flatten().sort().values, torch.arange(nb, dtype=torch.int32, device=dev))     # a permutation
    assert not torch.equal(table.flatten(), torch.arange(nb, dtype=torch.int32, device=dev))
    assert bool((ctx == o.K).all()) and q_start.tolist() == [s * o.q for s in range(o.M + 1)]
    del b, q_b, kc_b, vc_b, table_b, ctx_b, q_start_b
    out.view(torch.int16).fill_(SENT16)
    enqueue_ops(a, 1, torch.cuda.current_stream(), 0)
    torch.cuda.synchronize()
    # a picked row at position p is a one-token chunk of a sequence of p + 1 tokens
    picks = [(s, i) for s in range(o.M) for i in (0, o.q - 1, T - (o.K - o.q) % T, 517)]
    rows = torch.tensor([s * o.q + i for s, i in picks], device=dev)
    ref = reference(q[rows], kc, vc, table[[s for s, _ in picks]],
                    torch.tensor([o.K - o.q + i + 1 for _, i in picks], dtype=torch.int32, device=dev),
                    torch.arange(len(picks) + 1, dtype=torch.int32, device=dev))
    assert any((o.K - o.q + i) % T == 0 for _, i in picks)
    err = (out[rows].double() - ref).abs().max().item()
    vmax = float(vc.abs().max())
    print(f"llm_prefill_2048 attention: max|out - ref| = {err:.5f} (bound {RANDOM_BOUND * vmax:.5f})")
    assert err <= RANDOM_BOUND * vmax
    assert not bool((out.view(torch.int16) == SENT16).all(-1).any())             # every row was written
    del a
    torch.cuda.empty_cache()
