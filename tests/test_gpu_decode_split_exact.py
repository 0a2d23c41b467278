"""Exact-arithmetic, guarded-buffer tests of the split-KV paged decode attention
(loadgen.paged_decode_attention with kv_splits >= 2; run with `-m gpu` on an MI355X), in the style
of test_gpu_decode_attn_exact.py, whose reference, operands and regimes are used.

The four regimes of that module carry over, and the three exact ones stay `torch.equal`: the split
launch adds one fp32 merge level, and

  onehot   probabilities exactly 1 and 0 make every split's partial exact; a split without a
           target has every score 0, so m = 0, and its merge weight exp2(-362 log2 e) is exactly 0
           beside the target's split (m = 362); an empty split has m = -inf and weight 0;
  pair     two targets per head with p = 0.5 each: in two DIFFERENT splits (both have m = 362 and
           l = 1, merge weights exactly 1) or in ONE split in blocks that different waves take;
  uniform  q = 0: every split has m = 0 and merge weight 1, its normaliser is its exact token
           count, the sums of V integers in [-4, 4] over at most 1,024 tokens are exact in fp32.

The random regime keeps |out - ref| <= 2^-7 max|V|: that module's derivation of the bound does not
depend on the number of fp32 merge levels (each costs a few 2^-24 relative).

split_range below is a Python copy of the kernel's partition rule, which is part of its contract;
the targets are placed by it (place), and test_decode_split_cpu.py asserts on the CPU what the
placement and the context lengths cover.

Every launch runs guarded as in the decode module (q, out, the caches, the table and ctx_lens), and
the workspace is a 16-byte aligned window of exactly decode_split_workspace_floats elements inside
a SENT32-filled allocation, filled with NaN before every launch: a word of it that the merge read
without the split kernel having written it would make the output NaN, and the cells outside the
window are compared bitwise afterwards.

MEASURED on an MI355X (printed by the tests):
  Co-run (4 + 4 launch pairs per victim, each with its own workspace): the victim's slowdown 0.52 .. 0.99, and
  1.66 .. 1.80 beside the unmasked stream aggressor; every output bit-exact.  The module: 121 tests in 4 s.
"""
import functools
import json
import subprocess
import sys

import pytest
import torch

import test_gpu_corun_exact as CO
from test_gpu_decode_attn_exact import (RANDOM_BOUND, block_tables, guarded_ints_2d, hadamard, paged_caches,
                                        reference)
from test_gpu_decode_attn_exact import logical_operands as unplaced_operands      # uniform and random: no targets
from test_gpu_kernels_exact import (NAN, SENT16, SENT32, guarded_input, guarded_output, guarded_vector, guards_intact,
                                    out_window)

pytestmark = pytest.mark.gpu

D, T = 128, 32
C0 = 8                      # column offset of the q and out windows; sequence stride Hq * D + C0
WS_BEFORE, WS_AFTER = 4, 8  # SENT32 cells around the workspace window (4 keep it 16-byte aligned)
CTX_A = (0, 1, 33, 257, 320, 1025, 1121, 97)
CTX_B = (1153, 64, 0, 129, 31, 640, 2, 513)
CTX_UNIFORM = (1, 2, 32, 64, 256, 512, 1024, 128)
CTX_SHORT = (0, 1, 33, 97, 64, 31, 65, 2)          # no sequence has more than 4 blocks
KV_SPLITS = (2, 3, 4, 8, 16)
SHAPES = ((1, 2), (2, 1), (4, 1), (8, 2), (16, 1))          # (group, Hkv)
REGIMES = ("onehot", "pair", "uniform", "random")
SLOTS = (3, 0, 17, 30, 1, 2, 9, 21, 12, 26, 6, 14)          # where a partner token may sit in its block


@pytest.fixture(scope="module")
def hip():
    from k8s_gpu_scheduler_amd import _native
    return _native.hip(required=True)


# ------------------------------------------------------------------------------------------------
# the partition rule and the placement of the targets (asserted in test_decode_split_cpu.py)
# ------------------------------------------------------------------------------------------------
def split_range(ctx, kv_splits, p):
    """The blocks [lo, hi) of split p: with nblk = ceil(ctx / 32) and bps = ceil(nblk / kv_splits),
    [p * bps, min(nblk, (p + 1) * bps)); empty (lo == hi) where p * bps >= nblk."""
    nblk = -(-ctx // T)
    bps = -(-nblk // kv_splits)
    return min(p * bps, nblk), min((p + 1) * bps, nblk)


def nonempty_splits(ctx, kv_splits):
    return [p for p in range(kv_splits) if split_range(ctx, kv_splits, p)[0] < split_range(ctx, kv_splits, p)[1]]


def split_of(t, ctx, kv_splits):
    """The split that takes token t."""
    for p in range(kv_splits):
        lo, hi = split_range(ctx, kv_splits, p)
        if lo <= t // T < hi:
            return p
    raise AssertionError((t, ctx, kv_splits))


def wave_of(t, ctx, kv_splits):
    """The wave of its split's workgroup that takes token t's block (round-robin from the range's start)."""
    return (t // T - split_range(ctx, kv_splits, split_of(t, ctx, kv_splits))[0]) % 4


def place(ctx, group, kv_splits, g, rot=0, pair=False):
    """Per head of a group, its target tokens in a sequence of ctx > 0 tokens: [t], or [t, u] with
    pair=True where ctx has a second block.  All tokens are distinct; heads share (cyclically) only
    where ctx < group.  The first targets are, in this order rotated by `rot` (the KV head: a group
    of one head gets a different one per KV head): the first token of the second non-empty split,
    the last token inside ctx (it lies in the last non-empty split), the first token of the last
    non-empty split, token 0; then slots of further blocks and random tokens.  With pair=True an
    even head's partner lies in another split than its target; an odd head's in the target's
    split, in a block another wave takes -- and where the target's split has no such block with a
    free token but the rule gives two blocks to split 0 (bps >= 2), the odd head's target moves into
    split 0's first block."""
    ne = nonempty_splits(ctx, kv_splits)
    firsts = [T * split_range(ctx, kv_splits, p)[0] for p in ne]
    lead = [firsts[1], ctx - 1, firsts[-1], 0] if len(ne) >= 2 else [0, ctx - 1, T * ((ctx - 1) // T)]
    lead = lead[rot % len(lead):] + lead[:rot % len(lead)]
    want = lead + [T + 5, 2 * T + 7, 3 * T + 31, 4 * T + 1, T * max((ctx - 1) // T - 1, 0) + 9]
    want += torch.randperm(ctx, generator=g).tolist()
    seen = []
    for t in want:
        if 0 <= t < ctx and t not in seen:
            seen.append(t)
    tg = seen[:min(group, ctx)]
    if not pair:
        return [[t] for t in tg]
    taken, out = set(tg), []

    def free(blocks):
        for j in blocks:
            for slot in SLOTS:
                u = T * j + slot
                if u < ctx and u not in taken:
                    return u
        return None
    nblk = -(-ctx // T)
    bps = -(-nblk // kv_splits)
    for c, t in enumerate(tg):
        p = split_of(t, ctx, kv_splits)
        lo, hi = split_range(ctx, kv_splits, p)
        u = None
        if c % 2:
            u = free([j for j in range(lo, hi) if (j - lo) % 4 != (t // T - lo) % 4])
            moved = free([0]) if u is None and p != 0 and bps >= 2 else None
            if moved is not None:                      # the target moves into split 0, which has bps full blocks
                taken.discard(t)
                t, p = moved, 0
                taken.add(t)
                u = free([j for j in range(1, bps) if j % 4])
        if u is None:                                  # another split's block, the next non-empty split first
            others = [q for q in ne[ne.index(p) + 1:] + ne[:ne.index(p)]]
            u = free([j for q in others for j in range(*split_range(ctx, kv_splits, q))])
        if u is None:                                  # a single split: any block another wave takes
            u = free([j for j in range(nblk) if j % 4 != (t // T) % 4])
        if u is not None:
            taken.add(u)
        out.append([t] if u is None else [t, u])
    return out


def placed_operands(regime, group, hkv, ctxs, kv_splits, g):
    """q [S, Hq, D] and per sequence K, V [Hkv, ctx, D] as fp32 tensors of bf16 values, as the decode
    module's onehot and pair regimes build them, the targets placed by `place`; and the placement,
    targets[s][kv][c] = the tokens of head kv * group + c."""
    S, Hq = len(ctxs), group * hkv
    H = hadamard()
    vmax = 127 if regime == "onehot" else 255
    q = torch.zeros(S, Hq, D)
    ks, vs, targets = [], [], []
    for s, ctx in enumerate(ctxs):
        k = 4 * H[64 + torch.randint(0, 64, (hkv, ctx), generator=g)]                 # orthogonal to every head
        v = torch.randint(-vmax, vmax + 1, (hkv, ctx, D), generator=g).float() / 64
        targets.append([])
        for kv in range(hkv):
            if ctx == 0:
                q[s, kv * group:(kv + 1) * group] = 8 * H[kv * group:(kv + 1) * group]
                targets[s].append([[] for _ in range(group)])
                continue
            tg = place(ctx, group, kv_splits, g, rot=kv, pair=regime == "pair")
            for c in range(group):
                r = kv * group + c % len(tg)            # heads share a target and its sign row only if ctx < group
                q[s, kv * group + c] = 8 * H[r]
                for t in tg[c % len(tg)]:
                    k[kv, t] = 4 * H[r]
            targets[s].append([tg[c % len(tg)] for c in range(group)])
        ks.append(k)
        vs.append(v)
    return q, ks, vs, targets


class Case:
    """One launch's operands, guarded, with the float64 reference.  kv_splits places the targets
    of the onehot and pair regimes; the uniform and random regimes do not depend on it."""

    def __init__(self, regime, group, hkv, ctxs, kv_splits, seed):
        g = torch.Generator().manual_seed(seed)
        self.regime, self.S, self.Hq, self.hkv, self.ctxs = regime, len(ctxs), group * hkv, hkv, ctxs
        self.group = group
        table, nb = block_tables(ctxs, g)
        if regime in ("onehot", "pair"):
            q, ks, vs, self.targets = placed_operands(regime, group, hkv, ctxs, kv_splits, g)
        else:
            q, ks, vs = unplaced_operands(regime, group, hkv, ctxs, g)
        kc, vc = paged_caches(ks, vs, table, nb, hkv)
        ctx = torch.tensor(ctxs, dtype=torch.int32)
        qb = q.to(torch.bfloat16)
        assert torch.equal(qb.float(), q)                                          # the operands are exact
        self.ref = reference(qb, kc, vc, table, ctx)
        self.vmax = max([float(v.abs().max()) for v in vs if v.numel()] + [0.0])
        self.NB, self.max_blocks, self.host_table = nb, table.shape[1], table
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
        self.ws_raw = {}
        if regime != "random":
            f = self.ref.float()
            if regime == "pair":      # exactly half-way between two bf16: the 16 dropped bits are 0x8000
                big = self.ref.abs() > 2.0 ** -20          # (an exact 0 carries the other tokens' exp(-362) weights)
                assert torch.equal(f.double()[big], self.ref[big])
                assert bool(((f.view(torch.int32) & 0xFFFF) == 0x8000).any()), "no tie in the reference"
            self.exp = f.to(torch.bfloat16).cuda()

    def workspace(self, kv_splits):
        """The guarded workspace window for kv_splits (for 1: the window of 2 splits), all NaN."""
        from k8s_gpu_scheduler_amd.ops import loadgen
        n = loadgen.decode_split_workspace_floats(self.S, self.Hq, max(kv_splits, 2))
        if kv_splits not in self.ws_raw:
            self.ws_raw[kv_splits] = guarded_vector(n, WS_BEFORE, WS_AFTER, "cuda")
        raw, ws = self.ws_raw[kv_splits]
        assert ws.data_ptr() % 16 == 0 and ws.numel() == n
        ws.fill_(NAN)
        return ws

    def resentinel(self):
        self.raw.fill_(SENT16)

    def run(self, kv_splits, q=None, kc=None, vc=None, table=None, ctx=None, **kw):
        from k8s_gpu_scheduler_amd.ops import loadgen
        ws = kw.pop("workspace", None)
        ws = self.workspace(kv_splits) if ws is None else ws
        return loadgen.paged_decode_attention(self.q if q is None else q, self.kc if kc is None else kc,
                                              self.vc if vc is None else vc, self.table if table is None else table,
                                              self.ctx if ctx is None else ctx, out=self.out, kv_splits=kv_splits,
                                              workspace=ws, **kw)

    def guards(self, kv_splits, what, raw=None, ws=None):
        """ws: the (raw, window) workspace of a launch with buffers of its own, as raw is its output's."""
        torch.cuda.synchronize()
        raw = self.raw if raw is None else raw
        assert guards_intact(raw, out_window(self.S, self.Hq * D, C0), SENT16), ("write outside out", what)
        raw, ws = self.ws_raw[kv_splits] if ws is None else ws
        assert guards_intact(raw, slice(WS_BEFORE, WS_BEFORE + ws.numel()), SENT32), ("write outside the workspace", what)

    def check(self, kv_splits, what, raw=None, out=None, ws=None):
        self.guards(kv_splits, what, raw, ws)
        out = self.out if out is None else out
        if self.regime == "random":
            err = (out.double().cpu() - self.ref).abs().max().item()
            print(f"split decode attention, random regime {what}: max|out - ref| = {err:.5f} "
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

    def workspace_still_nan(self, kv_splits):
        torch.cuda.synchronize()
        return bool(self.ws_raw[kv_splits][1].isnan().all())


def ctxs_for(regime, hkv):
    return CTX_UNIFORM if regime == "uniform" else (CTX_A if hkv == 1 else CTX_B)


@functools.lru_cache(maxsize=None)
def _case(regime, group, hkv, placed_for, ctxs):
    return Case(regime, group, hkv, ctxs, placed_for,
                seed=2000 * REGIMES.index(regime) + 100 * group + 10 * hkv + placed_for + len(ctxs) * sum(ctxs) % 7)


def case(regime, group, hkv, kv_splits, ctxs=None):
    """The case of a regime and shape; only the onehot and pair operands depend on kv_splits."""
    return _case(regime, group, hkv, kv_splits if regime in ("onehot", "pair") else 0, ctxs or ctxs_for(regime, hkv))


# ------------------------------------------------------------------------------------------------
# 1. the four regimes over shapes and split counts
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kv_splits", KV_SPLITS)
@pytest.mark.parametrize("group,hkv", SHAPES)
@pytest.mark.parametrize("regime", REGIMES)
def test_regimes(hip, regime, group, hkv, kv_splits):
    c = case(regime, group, hkv, kv_splits)
    assert hip.paged_decode_split_workgroups(c.S, hkv, kv_splits) == c.S * hkv * kv_splits
    c.resentinel()
    c.run(kv_splits)
    c.check(kv_splits, (regime, group, hkv, kv_splits))


def test_one_split_is_the_unsplit_launch_and_leaves_the_workspace_alone():
    from test_gpu_decode_attn_exact import case as unsplit_case
    c = case("pair", 4, 1, 4)
    c.resentinel()
    c.run(1)
    c.check(1, "kv_splits=1")
    assert c.workspace_still_nan(1)
    # and on the decode module's own case: bit for bit what the call without the keywords gives
    u = unsplit_case("random", 4, 2)
    u.resentinel()
    u.run()
    torch.cuda.synchronize()
    base = u.out.clone()
    u.resentinel()
    ws = torch.full((8,), NAN, device="cuda")
    u.run(kv_splits=1, workspace=ws)
    torch.cuda.synchronize()
    assert torch.equal(u.out.view(torch.int16), base.view(torch.int16)) and bool(ws.isnan().all())


def test_no_check_gives_the_same():
    c = case("pair", 4, 1, 3)
    c.resentinel()
    c.run(3, check=False)
    c.check(3, "check=False")


def test_workspace_is_allocated_when_none_is_given():
    from k8s_gpu_scheduler_amd.ops import loadgen
    c = case("onehot", 8, 2, 4)
    c.resentinel()
    loadgen.paged_decode_attention(c.q, c.kc, c.vc, c.table, c.ctx, out=c.out, kv_splits=4)
    c.workspace(4)
    c.check(4, "workspace=None")


# ------------------------------------------------------------------------------------------------
# 2. check=True stops bad context lengths and block ids on the host
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("breakage", ["block-NB", "block-minus-1", "ctx-past-table", "ctx-negative"])
def test_check_raises_and_launches_nothing(breakage):
    c = case("onehot", 4, 1, 4)
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
        c.run(4, table=table, ctx=ctx)
    assert c.untouched() and c.workspace_still_nan(4)


# ------------------------------------------------------------------------------------------------
# 3. side stream and graph replay, the caller's workspace
# ------------------------------------------------------------------------------------------------
def test_side_stream_and_graph_replay():
    c = case("pair", 8, 2, 4)
    s = torch.cuda.Stream()
    c.resentinel()
    ws = c.workspace(4)
    torch.cuda.synchronize()
    c.run(4, stream=s, workspace=ws)
    s.synchronize()
    c.check(4, "side stream")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        c.run(4, stream=s, check=False, workspace=ws)
    for k in range(2):
        c.resentinel()
        ws.fill_(NAN)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        s.synchronize()
        c.check(4, ("replay", k))


# ------------------------------------------------------------------------------------------------
# 4. more splits than any sequence has blocks; the grid and workspace rules
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["onehot", "pair"])
def test_more_splits_than_blocks(regime):
    assert max(-(-x // T) for x in CTX_SHORT) == 4
    for kv_splits in (8, 32):
        c = case(regime, 4, 1, kv_splits, CTX_SHORT)
        c.resentinel()
        c.run(kv_splits)
        c.check(kv_splits, ("short", regime, kv_splits))


def test_workgroups_and_workspace_match_the_python_rules(hip):
    from k8s_gpu_scheduler_amd.models import workloads as W
    for S, hkv, k in ((1, 1, 2), (8, 2, 3), (8, 8, 16), (32, 8, 32)):
        assert hip.paged_decode_split_workgroups(S, hkv, k) == W.default_attn_split_workgroups(S, hkv, k)
        assert hip.paged_decode_split_workspace_floats(S, 4 * hkv, k) == W.decode_split_workspace_floats(S, 4 * hkv, k)


# ------------------------------------------------------------------------------------------------
# 5. non-finite values on the one-hot base: compared with the unplanted run outside the dependants
# ------------------------------------------------------------------------------------------------
NF_SPLITS, NF_GROUP, NF_HKV = 4, 4, 2


@pytest.fixture(scope="module")
def nf_base():
    """(case, its output, the sequence planted in: the longest -- 1153 tokens, 37 blocks, four
    non-empty splits of 10, 10, 10 and 7 blocks)."""
    c = case("onehot", NF_GROUP, NF_HKV, NF_SPLITS)
    c.resentinel()
    c.run(NF_SPLITS)
    c.check(NF_SPLITS, "non-finite base")
    s = c.ctxs.index(max(c.ctxs))
    assert len(nonempty_splits(c.ctxs[s], NF_SPLITS)) == NF_SPLITS
    return c, c.out.clone(), s


def _same_bits_outside(out, base, mask):
    return torch.equal(out.view(torch.int16)[~mask], base.view(torch.int16)[~mask])


def _v_cell(c, s, kv, t, d):
    """Index of V[token t of sequence s, KV head kv, d] in the paged cache."""
    return int(c.host_table[s, t // T]), kv, d, t % T


def test_nan_in_q_poisons_its_head_only(nf_base):
    c, base, s = nf_base
    h = NF_GROUP + 1                                    # a head of the second KV head
    q = c.q.clone()
    q[s, h, 77] = NAN
    c.resentinel()
    c.run(NF_SPLITS, q=q)
    c.guards(NF_SPLITS, "NaN in q")
    mask = torch.zeros_like(base, dtype=torch.bool)
    mask[s, h] = True
    assert bool(c.out[s, h].isnan().all()) and _same_bits_outside(c.out, base, mask)


@pytest.mark.parametrize("value", [NAN, float("inf")])
def test_non_finite_v_at_a_non_target_poisons_its_d_for_the_group(nf_base, value):
    c, base, s = nf_base
    kv, d, ctx = 1, 41, c.ctxs[s]
    tgs = [t for head in c.targets[s][kv] for t in head]
    # a token no head of the KV head targets, in a split other than head 0's target's
    p0 = split_of(c.targets[s][kv][0][0], ctx, NF_SPLITS)
    t = next(u for u in range(ctx - 2, -1, -1) if u not in tgs and split_of(u, ctx, NF_SPLITS) != p0)
    vc = c.vc.clone()
    vc[_v_cell(c, s, kv, t, d)] = value
    c.resentinel()
    c.run(NF_SPLITS, vc=vc)
    c.guards(NF_SPLITS, "non-finite V, probability 0")
    mask = torch.zeros_like(base, dtype=torch.bool)
    mask[s, kv * NF_GROUP:(kv + 1) * NF_GROUP, d] = True
    assert bool(c.out[mask].isnan().all()) and _same_bits_outside(c.out, base, mask)


def test_inf_in_v_at_a_target_is_inf_for_its_head_and_nan_for_the_others(nf_base):
    c, base, s = nf_base
    kv, d, head = 0, 100, 2
    t = c.targets[s][kv][head][0]
    vc = c.vc.clone()
    vc[_v_cell(c, s, kv, t, d)] = float("inf")
    c.resentinel()
    c.run(NF_SPLITS, vc=vc)
    c.guards(NF_SPLITS, "+Inf in V at a target")
    mask = torch.zeros_like(base, dtype=torch.bool)
    mask[s, kv * NF_GROUP:(kv + 1) * NF_GROUP, d] = True
    col = c.out[s, kv * NF_GROUP:(kv + 1) * NF_GROUP, d].float()
    assert col[head].item() == float("inf") and bool(col[[0, 1, 3]].isnan().all())
    assert _same_bits_outside(c.out, base, mask)


# ------------------------------------------------------------------------------------------------
# 6. beside a co-running load
# ------------------------------------------------------------------------------------------------
class SplitLaunch:
    """One split launch pair on a Case's inputs into an output and a workspace of its own (reset / enqueue /
    check, as the co-run module's CaseLaunch has): one workspace serves one launch in flight.  The
    workspace is NaN before the launch, so a merge that ran ahead of its split kernel, or read another
    launch's rows, poisons the output."""

    def __init__(self, c, kv_splits, what):
        from k8s_gpu_scheduler_amd.ops import loadgen
        self.case, self.kv_splits, self.what = c, kv_splits, what
        W = c.Hq * D
        self.raw, out2d = guarded_output(c.S, W, W + C0, C0, "cuda")
        self.out = out2d.unflatten(1, (c.Hq, D))
        self.ws = guarded_vector(loadgen.decode_split_workspace_floats(c.S, c.Hq, kv_splits), WS_BEFORE, WS_AFTER, "cuda")
        assert self.out.data_ptr() % 16 == 0 and self.ws[1].data_ptr() % 16 == 0

    def reset(self):
        self.raw.fill_(SENT16)
        self.ws[1].fill_(NAN)

    def enqueue(self, st):
        from k8s_gpu_scheduler_amd.ops import loadgen
        c = self.case
        loadgen.paged_decode_attention(c.q, c.kc, c.vc, c.table, c.ctx, out=self.out, kv_splits=self.kv_splits,
                                       workspace=self.ws[1], stream=st, check=False)

    def check(self, tag):
        self.case.check(self.kv_splits, (tag, self.what), self.raw, self.out, self.ws)


@pytest.mark.parametrize("aggressor,mode", [pytest.param(a, m, id=f"{a}-{m}") for a, m in CO.BASE_PAIRS])
def test_decode_split_corun(hip, aggressor, mode):
    """The split kernel and its merge are two launches through a global-memory workspace: the victim is R
    launch pairs of a pair-regime case at 4 splits and R of a uniform one at 3, every output bit-exact."""
    launches = [SplitLaunch(case("pair", 4, 1, 4), 4, ("pair", 4, 1, 4, r)) for r in range(CO.R)]
    launches += [SplitLaunch(case("uniform", 8, 2, 3), 3, ("uniform", 8, 2, 3, r)) for r in range(CO.R)]
    assert len({x.ws[1].data_ptr() for x in launches}) == len(launches) == 2 * CO.R
    victim = CO.Load("decode-split", {}, launches)
    try:
        CO.corun(hip, victim, CO.aggressor_for(aggressor, mode), mode)
    finally:
        CO.restore_knobs(hip)


# ------------------------------------------------------------------------------------------------
# 7. pod path
# ------------------------------------------------------------------------------------------------
def test_podrun_llm_decode_long():
    p = subprocess.run([sys.executable, "-m", "k8s_gpu_scheduler_amd.ops.podrun", "--workload", "llm_decode_long_8",
                        "--iters", "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    assert res["workload"] == "llm_decode_long_8" and res["iters"] == 2 and res["throughput"] > 0


def test_executor_llm_decode_long_buffers_and_attention_output():
    """The executor's operands are reproducible, and one iteration's attention output is within
    the random-regime bound of the float64 reference on 2 of the 8 sequences (each gathered through
    the table on its own: 32,768 tokens of 8 KV heads are 512 MiB of float64 K and V)."""
    from k8s_gpu_scheduler_amd.models import workloads as W
    from k8s_gpu_scheduler_amd.ops import loadgen
    from k8s_gpu_scheduler_amd.parallel.executor import _Buffers, enqueue_ops
    dev = torch.device("cuda", 0)
    w = W.get("llm_decode_long_8")
    a, b = _Buffers(w, dev), _Buffers(w, dev)
    o, (out, q, kc, vc, table, ctx, ws) = a.ops[1]
    _, (_, q_b, kc_b, vc_b, table_b, ctx_b, ws_b) = b.ops[1]
    nb = o.M * o.K // T
    assert o.kind == "attn_split" and 2 <= o.splits <= loadgen.ATTN_MAX_KV_SPLITS
    assert q.shape == (o.M, o.N, D) and kc.shape == (nb, o.rows, T, D) and vc.shape == (nb, o.rows, D, T)
    assert (kc.numel() + vc.numel()) * 2 == 1 << 30
    assert ws.dtype == torch.float32 and ws.numel() == loadgen.decode_split_workspace_floats(o.M, o.N, o.splits)
    assert ws.data_ptr() % 16 == 0 and ws.data_ptr() != ws_b.data_ptr()
    assert torch.equal(q.view(torch.int16), q_b.view(torch.int16)) and torch.equal(table, table_b) and torch.equal(ctx, ctx_b)
    assert torch.equal(kc.view(torch.int16), kc_b.view(torch.int16)) and torch.equal(vc.view(torch.int16), vc_b.view(torch.int16))
    assert torch.equal(table.flatten().sort().values, torch.arange(nb, dtype=torch.int32, device=dev))     # a permutation
    assert not torch.equal(table.flatten(), torch.arange(nb, dtype=torch.int32, device=dev))
    assert bool((ctx == o.K).all()) and float(vc.abs().max()) <= 127 / 64
    del b, q_b, kc_b, vc_b, table_b, ctx_b, ws_b
    out.view(torch.int16).fill_(SENT16)
    ws.fill_(NAN)
    enqueue_ops(a, 1, torch.cuda.current_stream(), 0)
    torch.cuda.synchronize()
    vmax = float(vc.abs().max())
    for s in (0, o.M - 1):
        ref = reference(q[s:s + 1], kc, vc, table[s:s + 1], ctx[s:s + 1])
        err = (out[s:s + 1].double() - ref).abs().max().item()
        print(f"llm_decode_long_8 attention, sequence {s}: max|out - ref| = {err:.5f} (bound {RANDOM_BOUND * vmax:.5f})")
        assert err <= RANDOM_BOUND * vmax
        del ref
    assert not bool((out.view(torch.int16) == SENT16).all(-1).any())             # every row was written
    del a
    torch.cuda.empty_cache()
