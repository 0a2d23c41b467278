"""Exact-arithmetic, guarded-buffer tests of the paged-KV decode attention (run with `-m gpu` on an
MI355X), in the style of test_gpu_kernels_exact.py, whose guard helpers and sentinels are used.

Three value regimes make the result independent of the summation order, of the accuracy of exp and
of the order in which the four waves' partial results are merged; the comparison with the float64
reference below, rounded float64 -> fp32 -> bf16 (nearest even), is `torch.equal`:

  onehot   q[h] = 8 H[r], H the 128 x 128 Sylvester-Hadamard sign matrix; the K row of the head's
           target token is 4 H[r], every other K row 4 H[64 + random], orthogonal to every head.
           The target's score is 4096 * scale = 362, all others are 0, so the probabilities are
           exactly 1 and 0 (exp(-362) is below fp32's range) and out == V[target].  Each head of a
           group has its own target token (r = h); only where ctx < group heads share a target,
           and then its sign row.  The targets sit in the first block, the last block, the last
           slot inside ctx and in blocks of different waves.  V is k / 64, |k| <= 127.
  pair     as onehot with two targets per head, in blocks that different waves take (where ctx
           gives the sequence two blocks; a shorter one keeps a single target): p = 0.5 each and
           out = bf16((v1 + v2) / 2).  V is k / 64 with |k| <= 255 here -- still bf16 values, but
           with |k| <= 127 no sum of two could need a ninth bit and no output would be a rounding
           tie; that one is, is asserted on the reference alone.
  uniform  q = 0, K random, V integers in [-4, 4], ctx a power of two <= 256: every probability is
           1 / ctx and out = bf16(sum / ctx), the sum exact in fp32.

The random regime (q, K randn, V uniform in [-1, 1], all rounded to bf16) is compared with
|out - ref| <= 2^-7 max|V|: the bf16 probabilities cost at most 2^-9 max|V|, the output rounding
at most 2^-9 max|V|, fp32 score and exp error at |score| <~ 10 less than 4e-4 max|V|; the sum is
0.0043 max|V|.  The measured maximum is printed; on an MI355X it was 0.00196 over these shapes.

Every launch runs guarded: q is a window (sequence stride Hq * 128 + 8, column offset 8) of a
NaN-filled allocation; out a window of the same shape in a SENT16-filled allocation whose guard
cells are compared bitwise afterwards; the cache blocks no table entry names are NaN, and so are
the slots past ctx of each sequence's last block, in K and in V; the table entries at or beyond
ceil(ctx / 32) hold SENT32 (no valid block); block_table (row stride max_blocks + 2, max_blocks
wider than any sequence needs) and ctx_lens start one element into SENT32-filled allocations.
"""
import functools
import json
import subprocess
import sys

import pytest
import torch

from test_gpu_kernels_exact import NAN, SENT16, SENT32, guarded_input, guarded_output, guards_intact, out_window

pytestmark = pytest.mark.gpu

D, T = 128, 32
SCALE = D ** -0.5
C0 = 8                      # column offset of the q and out windows; sequence stride Hq * D + C0
SPARE_BLOCKS = 3            # cache blocks no table entry names
WIDER = 3                   # table columns past the longest sequence's blocks
CTX_A = (0, 1, 31, 32, 33, 63, 64, 257)
CTX_B = (65, 127, 128, 129, 257, 0, 33, 1)
CTX_UNIFORM = (1, 2, 16, 32, 64, 128, 256, 8)
GROUPS = (1, 2, 4, 8, 16)
SHAPES = [(group, hkv) for group in GROUPS for hkv in (1, 2)]
REGIMES = ("onehot", "pair", "uniform", "random")
RANDOM_BOUND = 2.0 ** -7


@pytest.fixture(scope="module")
def hip():
    from k8s_gpu_scheduler_amd import _native
    return _native.hip(required=True)


# ------------------------------------------------------------------------------------------------
# the float64 reference (also imported by test_decode_attn_cpu.py)
# ------------------------------------------------------------------------------------------------
def reference(q, k_cache, v_cache, block_table, ctx_lens, scale=SCALE):
    """float64 [S, Hq, D]: per sequence, the tokens [0, ctx) gathered through the block table --
    nothing else of the caches or the table is looked at -- a softmax over them per query head,
    and the weighted sum of their V rows.  ctx == 0 gives zeros."""
    S, Hq, _ = q.shape
    Hkv = k_cache.shape[1]
    out = torch.zeros(S, Hq, D, dtype=torch.float64, device=q.device)
    for s, ctx in enumerate(ctx_lens.tolist()):
        if ctx == 0:
            continue
        blocks = block_table[s, :-(-ctx // T)].long()
        k = k_cache[blocks].double().permute(1, 0, 2, 3).reshape(Hkv, -1, D)[:, :ctx]            # [Hkv, ctx, D]
        v = v_cache[blocks].double().permute(1, 0, 3, 2).reshape(Hkv, -1, D)[:, :ctx]
        qs = q[s].double().view(Hkv, Hq // Hkv, D)
        p = torch.softmax(torch.einsum("gcd,gtd->gct", qs, k) * scale, dim=-1)
        out[s] = torch.einsum("gct,gtd->gcd", p, v).reshape(Hq, D)
    return out


# ------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hadamard():
    i = torch.arange(D)
    bits = i[:, None] & i[None, :]
    par = torch.zeros_like(bits)
    for b in range(7):
        par ^= (bits >> b) & 1
    h = (1 - 2 * par).float()
    assert torch.equal(h @ h.T, D * torch.eye(D))
    return h


def block_tables(ctxs, g):
    """(table [S, max_blocks] with SENT32 past each sequence's blocks, NB).  The physical blocks
    are dealt out by a random permutation, except that the two longest sequences alternate over one
    run of ids, one ascending and one descending: interleaved in memory, and not monotone."""
    need = [-(-c // T) for c in ctxs]
    max_blocks = max(need) + WIDER
    nb = sum(need) + SPARE_BLOCKS
    perm = torch.randperm(nb, generator=g).tolist()
    a, b = sorted(range(len(ctxs)), key=lambda s: -need[s])[:2]          # need[a] >= need[b]
    run = sorted(perm[:need[a] + need[b]])
    rest = perm[need[a] + need[b]:]
    n = need[b]
    ids = {a: run[0:2 * n:2] + run[2 * n:], b: run[1:2 * n:2][::-1]}
    table = torch.full((len(ctxs), max_blocks), SENT32, dtype=torch.int32)
    for s in range(len(ctxs)):
        mine = ids[s] if s in ids else [rest.pop() for _ in range(need[s])]
        assert len(mine) == need[s]
        table[s, :need[s]] = torch.tensor(mine, dtype=torch.int32)
    named = table[table != SENT32]
    assert named.numel() == nb - SPARE_BLOCKS == named.unique().numel()
    if n >= 2:
        ra, rb = table[a, :need[a]].tolist(), table[b, :need[b]].tolist()
        assert min(ra) < rb[0] < max(ra) and rb != sorted(rb)             # interleaved; not monotone
        assert not torch.equal(named, torch.arange(named.numel(), dtype=torch.int32))
    return table, nb


def targets_for(ctx, count, g):
    """`count` distinct tokens of [0, ctx) (ctx >= count): the first block's first slot, the last
    slot inside ctx, the last block's first slot, slots of the blocks the other waves take, then
    random ones."""
    last_block = (ctx - 1) // T
    want = [0, ctx - 1, T * last_block, T + 5, 2 * T + 7, 3 * T + 31, 4 * T + 1, T * max(last_block - 1, 0) + 9]
    want += torch.randperm(ctx, generator=g).tolist()
    seen = []
    for t in want:
        if 0 <= t < ctx and t not in seen:
            seen.append(t)
    return seen[:count]


def partner_for(t, ctx, taken):
    """A token in another block than t's, which another wave takes, and which no head of the group
    uses yet; None where ctx has a single block."""
    nblk = -(-ctx // T)
    for j in range(nblk):
        if j % 4 != (t // T) % 4:
            for slot in (3, 0, 17, 30, 1, 2):
                u = T * j + slot
                if u < ctx and u not in taken:
                    return u
    return None


def logical_operands(regime, group, hkv, ctxs, g):
    """q [S, Hq, D] and per sequence K, V [Hkv, ctx, D] as fp32 tensors of bf16 values."""
    S, Hq = len(ctxs), group * hkv
    H = hadamard()
    if regime == "random":
        q = torch.randn(S, Hq, D, generator=g).to(torch.bfloat16).float()
        ks = [torch.randn(hkv, c, D, generator=g).to(torch.bfloat16).float() for c in ctxs]
        vs = [(torch.rand(hkv, c, D, generator=g) * 2 - 1).to(torch.bfloat16).float() for c in ctxs]
        return q, ks, vs
    if regime == "uniform":
        q = torch.zeros(S, Hq, D)
        ks = [torch.randn(hkv, c, D, generator=g).to(torch.bfloat16).float() for c in ctxs]
        vs = [torch.randint(-4, 5, (hkv, c, D), generator=g).float() for c in ctxs]
        return q, ks, vs
    vmax = 127 if regime == "onehot" else 255
    q = torch.zeros(S, Hq, D)
    ks, vs = [], []
    for s, ctx in enumerate(ctxs):
        k = 4 * H[64 + torch.randint(0, 64, (hkv, ctx), generator=g)]                 # orthogonal to every head
        v = torch.randint(-vmax, vmax + 1, (hkv, ctx, D), generator=g).float() / 64
        for kv in range(hkv):
            if ctx == 0:
                q[s, kv * group:(kv + 1) * group] = 8 * H[kv * group:(kv + 1) * group]
                continue
            tg = targets_for(ctx, min(group, ctx), g)
            taken = set(tg)
            for c in range(group):
                r = kv * group + c % len(tg)            # heads share a target and its sign row only if ctx < group
                t = tg[c % len(tg)]
                q[s, kv * group + c] = 8 * H[r]
                k[kv, t] = 4 * H[r]
                if regime == "pair" and c < len(tg):
                    u = partner_for(t, ctx, taken)
                    if u is not None:
                        taken.add(u)
                        k[kv, u] = 4 * H[r]
        ks.append(k)
        vs.append(v)
    return q, ks, vs


def paged_caches(ks, vs, table, nb, hkv):
    """bf16 k_cache [NB, Hkv, 32, 128] and v_cache [NB, Hkv, 128, 32], NaN wherever no token of a
    sequence lives: the blocks no table entry names and the slots past ctx of the last blocks."""
    kc = torch.full((nb, hkv, T, D), NAN)
    vc = torch.full((nb, hkv, D, T), NAN)
    for s, (k, v) in enumerate(zip(ks, vs)):
        ctx = k.shape[1]
        for j in range(-(-ctx // T)):
            blk, n = int(table[s, j]), min(T, ctx - T * j)
            kc[blk, :, :n] = k[:, T * j:T * j + n]
            vc[blk, :, :, :n] = v[:, T * j:T * j + n].transpose(1, 2)
    kb, vb = kc.to(torch.bfloat16), vc.to(torch.bfloat16)
    assert torch.equal(kb.float().nan_to_num(7.0), kc.nan_to_num(7.0)) and torch.equal(vb.float().nan_to_num(7.0), vc.nan_to_num(7.0))
    return kb, vb


def guarded_ints_2d(t, ld):
    """(raw, view): the int32 matrix t with row stride ld, starting one element into a SENT32-filled
    allocation."""
    rows, cols = t.shape
    raw = torch.full((1 + rows * ld + 3,), SENT32, dtype=torch.int32, device="cuda")
    view = raw[1:1 + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(t)
    assert view.data_ptr() % 8 == 4 and view.stride(0) == ld
    return raw, view


class Case:
    def __init__(self, regime, group, hkv, ctxs, seed):
        g = torch.Generator().manual_seed(seed)
        self.regime, self.S, self.Hq, self.hkv, self.ctxs = regime, len(ctxs), group * hkv, hkv, ctxs
        table, nb = block_tables(ctxs, g)
        q, ks, vs = logical_operands(regime, group, hkv, ctxs, g)
        kc, vc = paged_caches(ks, vs, table, nb, hkv)
        ctx = torch.tensor(ctxs, dtype=torch.int32)
        qb = q.to(torch.bfloat16)
        assert torch.equal(qb.float(), q)                                          # the operands are exact
        self.ref = reference(qb, kc, vc, table, ctx)
        self.vmax = max([float(v.abs().max()) for v in vs if v.numel()] + [0.0])
        self.NB, self.max_blocks = nb, table.shape[1]
        W = self.Hq * D
        self.q = guarded_input(qb.view(self.S, W).cuda(), W + C0, c0=C0).unflatten(1, (self.Hq, D))
        self.kc, self.vc = kc.cuda(), vc.cuda()
        self.table_raw, self.table = guarded_ints_2d(table, self.max_blocks + 2)
        self.ctx_raw = torch.full((1 + self.S + 3,), SENT32, dtype=torch.int32, device="cuda")
        self.ctx = self.ctx_raw[1:1 + self.S]
        self.ctx.copy_(ctx)
        self.raw, out2d = guarded_output(self.S, W, W + C0, C0, "cuda")
        self.out = out2d.unflatten(1, (self.Hq, D))
        assert self.q.data_ptr() % 16 == 0 and self.out.data_ptr() % 16 == 0 and self.q.stride(0) == W + C0
        if regime != "random":
            f = self.ref.float()
            if regime == "pair":      # exactly half-way between two bf16: the 16 dropped bits are 0x8000
                big = self.ref.abs() > 2.0 ** -20          # (an exact 0 carries the other tokens' exp(-362) weights)
                assert torch.equal(f.double()[big], self.ref[big])
                assert bool(((f.view(torch.int32) & 0xFFFF) == 0x8000).any()), "no tie in the reference"
            self.exp = f.to(torch.bfloat16).cuda()

    def resentinel(self):
        self.raw.fill_(SENT16)

    def run(self, **kw):
        from k8s_gpu_scheduler_amd.ops import loadgen
        return loadgen.paged_decode_attention(self.q, self.kc, self.vc, self.table, self.ctx, out=self.out, **kw)

    def check(self, what):
        torch.cuda.synchronize()
        out = self.out
        assert guards_intact(self.raw, out_window(self.S, self.Hq * D, C0), SENT16), ("write outside the window", what)
        if self.regime == "random":
            err = (out.double().cpu() - self.ref).abs().max().item()
            print(f"decode attention, random regime {what}: max|out - ref| = {err:.5f} "
                  f"(bound {RANDOM_BOUND * self.vmax:.5f}, max|V| = {self.vmax:.4f})")
            assert err <= RANDOM_BOUND * self.vmax, (what, err)
            return
        if not torch.equal(out, self.exp):
            bad = (out.float() != self.exp.float()).nonzero()
            s, h, d = bad[0].tolist()
            raise AssertionError((what, f"{len(bad)} elements differ, first at [{s}, {h}, {d}] (ctx {self.ctxs[s]}): "
                                        f"got {out[s, h, d].item()}, expected {self.exp[s, h, d].item()}"))
        for s, c in enumerate(self.ctxs):
            if c == 0:
                assert not out[s].view(torch.int16).any(), "ctx == 0 must give +0.0"

    def untouched(self):
        torch.cuda.synchronize()
        return guards_intact(self.raw, (slice(0, 0), slice(0, 0)), SENT16)


@functools.lru_cache(maxsize=None)
def case(regime, group, hkv):
    ctxs = CTX_UNIFORM if regime == "uniform" else (CTX_A if hkv == 1 else CTX_B)
    return Case(regime, group, hkv, ctxs, seed=1000 * REGIMES.index(regime) + 10 * group + hkv)


# ------------------------------------------------------------------------------------------------
# 1. the four regimes over every group size
# ------------------------------------------------------------------------------------------------
def test_the_cases_cover_the_context_lengths():
    assert set(CTX_A) | set(CTX_B) >= {0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257}
    assert all(c & (c - 1) == 0 and 0 < c <= 256 for c in CTX_UNIFORM)
    assert len(CTX_A) <= 8 and len(CTX_B) <= 8 and len(CTX_UNIFORM) <= 8
    # a launch mixes sequences whose waves all have blocks with ones that leave waves without any
    assert min(CTX_A) == 0 and max(CTX_A) > 4 * T and min(CTX_B) == 0 and max(CTX_B) > 4 * T


@pytest.mark.parametrize("group,hkv", SHAPES)
@pytest.mark.parametrize("regime", REGIMES)
def test_regimes(hip, regime, group, hkv):
    c = case(regime, group, hkv)
    assert hip.paged_decode_workgroups(c.S, hkv) == c.S * hkv
    c.resentinel()
    c.run()
    c.check((regime, group, hkv))


def test_no_check_gives_the_same(hip):
    c = case("pair", 4, 2)
    c.resentinel()
    c.run(check=False)
    c.check("check=False")


# ------------------------------------------------------------------------------------------------
# 2. check=True stops bad context lengths and block ids on the host
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("breakage", ["block-NB", "block-minus-1", "ctx-past-table", "ctx-negative"])
def test_check_raises_and_launches_nothing(breakage):
    from k8s_gpu_scheduler_amd.ops import loadgen
    c = case("onehot", 4, 1)
    s = c.ctxs.index(257)
    table, ctx = c.table.clone(), c.ctx.clone()
    if breakage == "block-NB":
        table[s, 8] = c.NB                       # the sequence's last named entry
    elif breakage == "block-minus-1":
        table[s, 0] = -1
    elif breakage == "ctx-past-table":
        ctx[c.ctxs.index(1)] = T * c.max_blocks + 1
    else:
        ctx[c.ctxs.index(1)] = -1
    c.resentinel()
    with pytest.raises(ValueError):
        loadgen.paged_decode_attention(c.q, c.kc, c.vc, table, ctx, out=c.out)
    assert c.untouched()


# ------------------------------------------------------------------------------------------------
# 3. side stream and graph replay
# ------------------------------------------------------------------------------------------------
def test_side_stream_and_graph_replay():
    c = case("pair", 8, 1)
    s = torch.cuda.Stream()
    c.resentinel()
    torch.cuda.synchronize()
    c.run(stream=s)
    s.synchronize()
    c.check("side stream")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        c.run(stream=s, check=False)
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
    for S, hkv in ((1, 1), (8, 2), (256, 8), (2048, 1)):
        assert hip.paged_decode_workgroups(S, hkv) == W.default_attn_workgroups(S, hkv)


# ------------------------------------------------------------------------------------------------
# 5. pod path
# ------------------------------------------------------------------------------------------------
def test_podrun_llm_decode():
    p = subprocess.run([sys.executable, "-m", "k8s_gpu_scheduler_amd.ops.podrun", "--workload", "llm_decode_256",
                        "--iters", "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    assert res["workload"] == "llm_decode_256" and res["iters"] == 2 and res["throughput"] > 0


def test_executor_llm_decode_buffers_and_attention_output():
    """The executor's operands are reproducible, and one iteration's attention output is within
    the random-regime bound of the float64 reference on 4 sequences gathered through the table."""
    from k8s_gpu_scheduler_amd.models import workloads as W
    from k8s_gpu_scheduler_amd.parallel.executor import _Buffers, enqueue_ops
    dev = torch.device("cuda", 0)
    w = W.get("llm_decode_256")
    a, b = _Buffers(w, dev), _Buffers(w, dev)
    o, (out, q, kc, vc, table, ctx) = a.ops[1]
    _, (_, q_b, kc_b, vc_b, table_b, ctx_b) = b.ops[1]
    nb = o.M * o.K // T
    assert o.kind == "attn" and q.shape == (o.M, o.N, D) and kc.shape == (nb, o.rows, T, D) and vc.shape == (nb, o.rows, D, T)
    assert (kc.numel() + vc.numel()) * 2 == 1 << 30
    assert torch.equal(q.view(torch.int16), q_b.view(torch.int16)) and torch.equal(table, table_b) and torch.equal(ctx, ctx_b)
    assert torch.equal(kc.view(torch.int16), kc_b.view(torch.int16)) and torch.equal(vc.view(torch.int16), vc_b.view(torch.int16))
    assert torch.equal(table.flatten().sort().values, torch.arange(nb, dtype=torch.int32, device=dev))     # a permutation
    assert not torch.equal(table.flatten(), torch.arange(nb, dtype=torch.int32, device=dev))
    assert bool((ctx == o.K).all()) and float(vc.abs().max()) <= 127 / 64
    del b, q_b, kc_b, vc_b, table_b, ctx_b
    out.view(torch.int16).fill_(SENT16)
    enqueue_ops(a, 1, torch.cuda.current_stream(), 0)
    torch.cuda.synchronize()
    pick = [0, 1, o.M // 2, o.M - 1]
    ref = reference(q[pick], kc, vc, table[pick], ctx[pick])
    err = (out[pick].double() - ref).abs().max().item()
    vmax = float(vc.abs().max())
    print(f"llm_decode_256 attention: max|out - ref| = {err:.5f} (bound {RANDOM_BOUND * vmax:.5f})")
    assert err <= RANDOM_BOUND * vmax
    assert not bool((out.view(torch.int16) == SENT16).all(-1).any())             # every row was written
    del a
    torch.cuda.empty_cache()
