"""Exact-arithmetic, guarded-buffer tests of the RoPE + paged-KV append (run with `-m gpu` on an MI355X),
in the style of test_gpu_prefill_attn_exact.py, whose (ctx, q_len) lists and block-table builder (the
decode module's, with its tie rule) are used, and of test_gpu_kernels_exact.py, whose guard helpers and
sentinels are used.

A launch holds 8 sequences given as (ctx, q_len): the chunk of a sequence is its last q_len tokens, row i
of it is token p = ctx - q_len + i and goes to slot p % 32 of block block_table[s, p // 32].  SEQS_A (one
KV head) and SEQS_B (two) are the prefill module's; SEQS_C (one KV head) adds what they lack: chunks that
span 9 cache blocks (257 tokens from slot 15, 256 from slot 12), decode tokens (32, 1) and (33, 1), a
3-token chunk inside one block.  test_the_cases_cover_the_chunk_shapes asserts the coverage.

Value regimes (q_out and K compared with `torch.equal` unless said otherwise; V always as int16):

  quarter  row p of the table is (cos, sin) of ((p + i) % 4) quarter turns at pair i, written as the
           literals 0 and +-1; x is a random arrangement of distinct integers of [-256, 256] in every
           (row, head) vector: the outputs are +-x1 or +-x2 exactly.  Pins the pairing i <-> i + 64, both
           signs, the position formula, the table row, the head order q | K | V and every slot address.
  dyadic   c = a / 8 and s = b / 8 with |a|, |b| <= 8, x = k / 64 with |k| <= 127: every product and sum
           is exact in fp32, so the output is the single bf16 rounding of the float64 value.  Asserted on
           the reference alone: that exactness, and that some expected value is a rounding tie.
  true     rope_table(257) (longer where SEQS_C needs it), randn q / K:
           |out - ref| <= (2^-8 + 2^-21) * (|x1| + |x2|) against float64 on the same fp32 table -- one bf16
           rounding is at most 2^-8 relative, |y| <= |x1| + |x2| because |c|, |s| <= 1, and the fp32
           product and FMA roundings are below 2^-22 of that each.  The measured maximum of
           |out - ref| / bound is printed (MEASURED below).

V holds random bf16 bit patterns in every regime, among them -0.0, subnormals, 0x7F7F, +-Inf and NaNs
with payloads.

Every launch runs guarded: qkv is a window (token stride (Hq + 2 Hkv) * 128 + 8, column offset 8) of a
NaN-filled allocation and holds LEAD NaN rows before q_start[0] and TRAIL after q_start[S]; q_out is a
window of a SENT16-filled allocation that is compared bitwise afterwards, guards included; both caches
are wholly SENT16 before the launch, spare blocks that no table entry names included, and wholly
compared afterwards with a host-built expectation: SENT16 everywhere but the chunks' slots; the table
entries at or beyond ceil(ctx / 32) hold SENT32; block_table, ctx_lens and q_start start one element
into SENT32-filled allocations; cos_sin is a window of a NaN-filled fp32 allocation: NaN rows before
row 0 and from max_pos on.
"""
import functools
import json
import subprocess
import sys

import pytest
import torch

import test_gpu_corun_exact as CO
import test_gpu_decode_attn_exact as ATT
import test_gpu_prefill_attn_exact as PRE
from test_gpu_kernels_exact import NAN, SENT16, SENT32, guarded_input, guarded_output, guards_intact

pytestmark = pytest.mark.gpu

# MEASURED on an MI355X (printed by the tests):
MEASURED = """
  true regime, max |out - ref| / bound per (group, sequences): 0.8899 .. 0.9876, the largest at (4, C), where
  max |out - ref| = 0.014824; llm_layer_decode_256 append, 8 picked rows: 0.9231; llm_layer_prefill_2048: 0.8961.
  Co-run (4 launches per victim): the victim's slowdown 0.22 .. 0.89; every output bit-exact.
  The module: 60 tests in 11 s.
"""

D, T, C0 = ATT.D, ATT.T, ATT.C0
HALF = D // 2
R0 = PRE.R0                 # guard rows in front of the windows (guarded_input / guarded_output)
LEAD, TRAIL = PRE.LEAD, PRE.TRAIL
SEQS_A, SEQS_B = PRE.SEQS_A, PRE.SEQS_B
SEQS_C = ((272, 257), (32, 1), (33, 1), (300, 256), (0, 0), (40, 3), (64, 64), (95, 0))
SEQS = {"A": (SEQS_A, 1), "B": (SEQS_B, 2), "C": (SEQS_C, 1)}          # name -> ((ctx, q_len) list, KV heads)
GROUPS = (1, 2, 4, 8, 16)
SHAPES = [(group, name) for group in GROUPS for name in ("A", "B")] + [(1, "C"), (4, "C")]
REGIMES = ("quarter", "dyadic", "true")
TRUE_BOUND = 2.0 ** -8 + 2.0 ** -21
# bf16 bit patterns every V carries: -0.0, the smallest and a negative subnormal, the largest finite, +-Inf, NaNs with payloads
V_SPECIALS = (0x8000, 0x0001, 0x807F, 0x7F7F, 0x7F80, 0xFF80, 0x7FC1, 0xFFA5, 0x7F81)


@pytest.fixture(scope="module")
def hip():
    from k8s_gpu_scheduler_amd import _native
    return _native.hip(required=True)


# ------------------------------------------------------------------------------------------------
# the float64 reference (also imported by test_rope_append_cpu.py)
# ------------------------------------------------------------------------------------------------
def rotate(x, cs):
    """float64 rotate-half of x [..., 128] by cs [..., 128] (64 cosines, then 64 sines)."""
    x1, x2, c, s = x[..., :HALF], x[..., HALF:], cs[..., :HALF], cs[..., HALF:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


def reference(qkv, cos_sin, ctx_lens, q_start, hkv):
    """(q_out float64 [Tq, Hq, 128], k float64 [Tq, Hkv, 128], pos int64 [Tq], seq int64 [Tq]): the
    rotated q and K heads of every chunk row, its position and its sequence; rows of no chunk are
    zeros with position -1."""
    Tq, Ht, _ = qkv.shape
    Hq = Ht - 2 * hkv
    q_out = torch.zeros(Tq, Hq, D, dtype=torch.float64)
    k = torch.zeros(Tq, hkv, D, dtype=torch.float64)
    pos = torch.full((Tq,), -1, dtype=torch.int64)
    seq = torch.zeros(Tq, dtype=torch.int64)
    starts = q_start.tolist()
    for s, ctx in enumerate(ctx_lens.tolist()):
        r0, r1 = starts[s], starts[s + 1]
        if r1 == r0:
            continue
        p = ctx - (r1 - r0) + torch.arange(r1 - r0)
        cs = cos_sin[p].double()[:, None, :]
        x = qkv[r0:r1].double()
        q_out[r0:r1] = rotate(x[:, :Hq], cs)
        k[r0:r1] = rotate(x[:, Hq:Hq + hkv], cs)
        pos[r0:r1], seq[r0:r1] = p, s
    return q_out, k, pos, seq


def expected_caches(nb, hkv, k_bits, v_bits, pos, seq, table):
    """int16 k_cache [NB, Hkv, 32, 128] and v_cache [NB, Hkv, 128, 32]: SENT16 everywhere but the slots of
    the rows with pos >= 0, which hold k_bits / v_bits [Tq, Hkv, 128] of the row."""
    kc = torch.full((nb, hkv, T, D), SENT16, dtype=torch.int16)
    vc = torch.full((nb, hkv, D, T), SENT16, dtype=torch.int16)
    rows = (pos >= 0).nonzero().flatten()
    blk, slot = table[seq[rows], pos[rows] // T].long(), pos[rows] % T
    kc[blk, :, slot] = k_bits[rows]
    vc[blk, :, :, slot] = v_bits[rows]
    return kc, vc, blk, slot


def bits(t):
    return t.contiguous().view(torch.int16)


def unsigned_zero(b):
    """int16 bf16 bits with -0.0 as +0.0 (torch.equal on bf16 does not tell them apart either)."""
    return torch.where(b == -32768, torch.zeros_like(b), b)


# ------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------
def quarter_table(max_pos):
    k = (torch.arange(max_pos)[:, None] + torch.arange(HALF)[None, :]) % 4
    return torch.cat([torch.tensor([1.0, 0.0, -1.0, 0.0])[k], torch.tensor([0.0, 1.0, 0.0, -1.0])[k]], dim=1)


def logical_operands(regime, n, Ht, hkv, max_pos, g, finite_v=False):
    """(x fp32 [n, Ht, 128] of bf16 values -- the V heads are replaced by v_bits --, v_bits int16
    [n, Hkv, 128]: random bit patterns, or with finite_v values of [-1, 1], cos_sin fp32 [max_pos, 128])."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    if regime == "quarter":
        x = (torch.rand(n, Ht, 513, generator=g).argsort(-1)[..., :D] - 256).float()
        cs = quarter_table(max_pos)
    elif regime == "dyadic":
        x = torch.randint(-127, 128, (n, Ht, D), generator=g).float() / 64
        cs = torch.randint(-8, 9, (max_pos, D), generator=g).float() / 8
    else:
        x = torch.randn(n, Ht, D, generator=g).to(torch.bfloat16).float()
        cs = loadgen.rope_table(max_pos)
    if finite_v:
        return x, bits((torch.rand(n, hkv, D, generator=g) * 2 - 1).to(torch.bfloat16)), cs
    v_bits = torch.randint(0, 1 << 16, (n, hkv, D), generator=g).to(torch.int16)
    if n:
        v_bits[0, 0, :len(V_SPECIALS)] = torch.tensor(V_SPECIALS, dtype=torch.int32).to(torch.int16)
        v_bits[-1, -1, -len(V_SPECIALS):] = torch.tensor(V_SPECIALS, dtype=torch.int32).to(torch.int16)
    return x, v_bits, cs


class Case:
    def __init__(self, regime, group, name, seed, plant=None, identity=False):
        """name: a key of SEQS, or ((ctx, q_len) list, KV heads).  plant(x, cos_sin, seqs) may change the
        logical operands in place; identity replaces the table by c = 1, s = 0 and draws a finite V."""
        g = torch.Generator().manual_seed(seed)
        seqs, hkv = SEQS[name] if isinstance(name, str) else name
        self.regime, self.S, self.hkv, self.seqs = regime, len(seqs), hkv, seqs
        Hq = self.Hq = group * hkv
        Ht = self.Ht = Hq + 2 * hkv
        ctxs = tuple(c for c, _ in seqs)
        n = self.n = sum(q for _, q in seqs)
        self.Tq = LEAD + n + TRAIL
        self.max_pos = max(257, max(ctxs))
        table, nb = PRE.block_tables(ctxs, g)
        x, v_bits, cs = logical_operands(regime, n, Ht, hkv, self.max_pos, g, finite_v=identity)
        if identity:
            cs = torch.cat([torch.ones(self.max_pos, HALF), torch.zeros(self.max_pos, HALF)], dim=1)
        ctx = torch.tensor(ctxs, dtype=torch.int32)
        q_start = torch.tensor([LEAD] + [q for _, q in seqs]).cumsum(0).to(torch.int32)
        self.planted = plant(x, cs, seqs) if plant else None
        qfull = torch.full((self.Tq, Ht, D), NAN)
        qfull[LEAD:LEAD + n] = x
        qb = qfull.to(torch.bfloat16)
        assert torch.equal(qb[LEAD:LEAD + n].float().nan_to_num(7.0, 8.0, 9.0), x.nan_to_num(7.0, 8.0, 9.0))   # the operands are exact
        bits(qb)[LEAD:LEAD + n, Hq + hkv:] = v_bits
        self.qkv_host, self.cs_host, self.table_host, self.ctx_host, self.q_start_host = qb, cs, table, ctx, q_start
        ref_q, ref_k, pos, seq = reference(qb, cs, ctx, q_start, hkv)
        self.ref_q, self.ref_k, self.pos, self.seq = ref_q[LEAD:LEAD + n], ref_k, pos, seq
        self.NB, self.max_blocks, self.max_q_len = nb, table.shape[1], max(q for _, q in seqs)
        vfull = torch.zeros(self.Tq, hkv, D, dtype=torch.int16)
        vfull[LEAD:LEAD + n] = v_bits
        if regime != "true":
            if not plant:
                assert bool(ref_q.isfinite().all()) and bool(ref_k.isfinite().all())
                for r in (ref_q, ref_k):
                    assert torch.equal(r.float().double(), r)                            # exact in fp32, sums ...
                xs = qb[:, :Hq + hkv].double()
                csd = torch.zeros(self.Tq, 1, D, dtype=torch.float64)
                csd[pos >= 0, 0] = cs[pos[pos >= 0]].double()
                for prod in (xs[..., :HALF] * csd[..., HALF:], xs[..., HALF:] * csd[..., HALF:]):
                    assert torch.equal(prod.float().double().nan_to_num(7.0), prod.nan_to_num(7.0))   # ... and products
                if regime == "dyadic":
                    f = torch.cat([self.ref_q.flatten(), ref_k.flatten()]).float()
                    assert bool(((f.view(torch.int32) & 0xFFFF) == 0x8000).any()), "no tie in the expectation"
            self.exp_q = self.ref_q.float().to(torch.bfloat16)
            self.exp_kc, self.exp_vc, self.blk, self.slot = expected_caches(
                nb, hkv, bits(ref_k.float().to(torch.bfloat16)), vfull, pos, seq, table)
        else:
            self.exp_kc, self.exp_vc, self.blk, self.slot = expected_caches(nb, hkv, vfull, vfull, pos, seq, table)
            xa = qb[LEAD:LEAD + n, :Hq + hkv].double().abs()
            b = TRUE_BOUND * (xa[..., :HALF] + xa[..., HALF:])
            self.bound = torch.cat([b, b], dim=-1)                                       # [n, Hq + Hkv, 128]
        W = Ht * D
        self.qkv = guarded_input(qb.view(self.Tq, W).cuda(), W + C0, c0=C0).unflatten(1, (Ht, D))
        self.cos_sin = guarded_input(cs.cuda(), D, c0=0)
        self.table_raw, self.table = ATT.guarded_ints_2d(table, self.max_blocks + 2)
        self.ctx_raw, self.ctx = PRE.guarded_ints(ctx)
        self.q_start_raw, self.q_start = PRE.guarded_ints(q_start)
        self.outs = self.new_outputs()
        assert self.qkv.data_ptr() % 16 == 0 and self.qkv.stride(0) == W + C0 and self.cos_sin.is_contiguous()
        assert self.cos_sin.data_ptr() % 16 == 0 and self.cos_sin.shape == (self.max_pos, D)

    def new_outputs(self):
        """(raw, q_out, k_cache, v_cache): a [Tq, Hq, D] window in a SENT16-filled allocation of its own and two
        caches wholly SENT16."""
        W = self.Hq * D
        raw, out2d = guarded_output(self.Tq, W, W + C0, C0, "cuda")
        kc = torch.full((self.NB, self.hkv, T, D), SENT16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
        vc = torch.full((self.NB, self.hkv, D, T), SENT16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
        return raw, out2d.unflatten(1, (self.Hq, D)), kc, vc

    @staticmethod
    def resentinel(outs):
        raw, _, kc, vc = outs
        raw.fill_(SENT16)
        kc.view(torch.int16).fill_(SENT16)
        vc.view(torch.int16).fill_(SENT16)

    def launch(self, outs, table=None, ctx=None, q_start=None, **kw):
        from k8s_gpu_scheduler_amd.ops import loadgen
        _, q_out, kc, vc = outs
        return loadgen.rope_append(self.qkv, self.cos_sin, kc, vc, self.table if table is None else table,
                                   self.ctx if ctx is None else ctx, self.q_start if q_start is None else q_start,
                                   q_out=q_out, **kw)

    def run(self, **kw):
        self.resentinel(self.outs)
        return self.launch(self.outs, **kw)

    def results(self, outs=None):
        """(chunk rows of q_out bf16, k_cache int16, v_cache int16) on the CPU, the guards of q_out checked."""
        raw, q_out, kc, vc = self.outs if outs is None else outs
        torch.cuda.synchronize()
        written = (slice(R0 + LEAD, R0 + LEAD + self.n), slice(C0, C0 + self.Hq * D))
        assert guards_intact(raw, written, SENT16), "write outside the chunks' rows of q_out"
        return q_out[LEAD:LEAD + self.n].cpu(), bits(kc).cpu(), bits(vc).cpu()

    def check(self, what, outs=None):
        got_q, got_kc, got_vc = self.results(outs)
        assert torch.equal(got_vc, self.exp_vc), (what, "v_cache", int((got_vc != self.exp_vc).sum()))
        if self.regime != "true":
            if not torch.equal(got_q, self.exp_q):
                bad = (got_q.float() != self.exp_q.float()).nonzero()
                r, h, d = bad[0].tolist()
                raise AssertionError((what, f"q_out: {len(bad)} elements differ, first at chunk row {r}, head {h}, d {d}: "
                                            f"got {got_q[r, h, d].item()}, expected {self.exp_q[r, h, d].item()}"))
            same = unsigned_zero(got_kc) == unsigned_zero(self.exp_kc)
            assert bool(same.all()), (what, "k_cache", int((~same).sum()), (~same).nonzero()[0].tolist())
            return
        # K: the chunks' slots within the bound, every other cell SENT16
        rows = (self.pos >= 0).nonzero().flatten()
        got_k = got_kc.view(torch.bfloat16)[self.blk, :, self.slot].double()              # [n, Hkv, 128]
        rest = got_kc.clone()
        rest[self.blk, :, self.slot] = SENT16
        assert bool((rest == SENT16).all()), (what, "k_cache written outside the chunks' slots")
        err = torch.cat([(got_q.double() - self.ref_q).abs(), (got_k - self.ref_k[rows]).abs()], dim=1)
        ratio = (err / self.bound.clamp_min(1e-300)).max().item() if self.n else 0.0
        print(f"rope_append, true regime {what}: max |out - ref| / bound = {ratio:.4f}, max |out - ref| = {err.max().item() if self.n else 0.0:.6f}")
        assert bool((err <= self.bound).all()), (what, ratio)

    def untouched(self, outs=None):
        raw, _, kc, vc = self.outs if outs is None else outs
        torch.cuda.synchronize()
        return (guards_intact(raw, (slice(0, 0), slice(0, 0)), SENT16) and bool((bits(kc) == SENT16).all())
                and bool((bits(vc) == SENT16).all()))


@functools.lru_cache(maxsize=None)
def case(regime, group, name):
    return Case(regime, group, name, seed=7000 + 1000 * REGIMES.index(regime) + 10 * group + "ABC".index(name))


# ------------------------------------------------------------------------------------------------
# 1. the regimes over every group size
# ------------------------------------------------------------------------------------------------
def test_the_cases_cover_the_chunk_shapes():
    every = [sq for seqs, _ in SEQS.values() for sq in seqs]
    for seqs, _ in SEQS.values():
        assert len(seqs) == 8 and all(0 <= n <= c for c, n in seqs)
    blocks = lambda c, n: (c - 1) // T - (c - n) // T + 1            # noqa: E731  cache blocks a chunk touches
    assert any(n and (c - n) % T and c % T and blocks(c, n) > 1 for c, n in every)      # starts and ends mid-block
    assert any(n > 1 and blocks(c, n) == 1 for c, n in every)                             # inside one block
    assert any(blocks(c, n) == 9 == (n + 30) // T + 1 for c, n in every if n)             # 9 blocks: the grid's whole width
    assert any(n == 0 < c for c, n in every) and any(c == 0 for c, n in every)
    assert any(n == 1 and (c - 1) % T == 31 for c, n in every)                            # a decode token in slot 31
    assert any(n == 1 and (c - 1) % T == 0 and c > 1 for c, n in every)                   # ... and in slot 0 of a later block
    assert any(n and (c - n) % 8 for c, n in every) and any(n and c % 8 for c, n in every)  # ragged 16-byte vectors
    assert any(n and (c - n) % T == 0 and c % T == 0 for c, n in every)                   # whole blocks only
    for name in "ABC":                                                                    # every launch has both V paths
        seqs = SEQS[name][0]
        assert any(n and ((c - n) % 8 or c % 8) for c, n in seqs) and any(n >= 16 for c, n in seqs)
    assert set(GROUPS) == {g for g, _ in SHAPES} and len(set(V_SPECIALS)) == len(V_SPECIALS)


@pytest.mark.parametrize("group,name", SHAPES)
@pytest.mark.parametrize("regime", REGIMES)
def test_regimes(hip, regime, group, name):
    c = case(regime, group, name)
    c.run()
    c.check((regime, group, name))


# ------------------------------------------------------------------------------------------------
# 2. the NaN rule
# ------------------------------------------------------------------------------------------------
INF = float("inf")


def plant_nonfinite(x, cs, seqs, dirty=True):
    """Plants NaN and +-Inf in single x1, x2, c and s cells of the (255, 100) sequence of SEQS_B (group 4,
    two KV heads: heads 0-7 q, 8-9 K) and returns the expected hits: (chunk row, heads, pair).  With
    dirty=False only the finite coefficients that two of the plants want beside them are set: the clean
    twin of the planted case."""
    s = seqs.index((255, 100))
    r0 = sum(n for _, n in seqs[:s])
    p0 = 255 - 100
    hits = []

    def cell(r, h, i, second, v):
        if dirty:
            x[r0 + r, h, i + HALF * second] = v
        hits.append((r0 + r, [h], i))

    def coefficient(r, col, v):
        """A table cell hits its pair in every q and K head of every chunk token at that position: the
        (256, 256) sequence has one too."""
        if dirty or v == 0.0:            # the finite ones always
            cs[p0 + r, col] = v
        if v != 0.0:
            first = 0
            for c, n in seqs:
                if c - n <= p0 + r < c:
                    hits.append((first + p0 + r - (c - n), list(range(10)), col % HALF))
                first += n

    cell(3, 1, 5, False, NAN)            # x1 of a q head
    cell(7, 9, 63, True, NAN)            # x2 of a K head
    cell(11, 8, 0, False, INF)           # x1 of a K head
    cell(13, 6, 17, True, -INF)          # x2 of a q head
    coefficient(20, HALF + 9, 0.0)       # Inf in x2 where the partner coefficient s is 0: 0 * Inf is NaN
    cell(20, 2, 9, True, INF)
    coefficient(30, 40, NAN)
    coefficient(41, HALF + 2, INF)
    coefficient(52, HALF + 33, 0.0)      # -Inf as the cosine beside a sine of 0
    coefficient(52, 33, -INF)
    return hits


def test_nan_rule():
    seed = 7000 + 1000 * REGIMES.index("dyadic") + 10 * 4 + 1
    dirty = Case("dyadic", 4, "B", seed=seed, plant=plant_nonfinite)
    twin = Case("dyadic", 4, "B", seed=seed, plant=functools.partial(plant_nonfinite, dirty=False))
    assert bool(twin.ref_q.isfinite().all()) and bool(twin.ref_k.isfinite().all()) and dirty.planted == twin.planted
    twin.run()
    dirty.run()
    cq, ckc, cvc = twin.results()
    dq, dkc, dvc = dirty.results()
    assert torch.equal(cvc, twin.exp_vc) and torch.equal(dvc, cvc)
    assert torch.equal(cq, twin.exp_q) and bool((unsigned_zero(ckc) == unsigned_zero(twin.exp_kc)).all())
    # the heads of a row as one [n, Hq + Hkv, 128] tensor: q_out, then K from the cache
    rows = (dirty.pos >= 0).nonzero().flatten()
    both = lambda q, kc: torch.cat([q, kc.view(torch.bfloat16)[dirty.blk, :, dirty.slot]], dim=1)      # noqa: E731
    got, was = both(dq, dkc), both(cq, ckc)
    ref = torch.cat([dirty.ref_q, dirty.ref_k[rows]], dim=1)
    hit = torch.zeros(got.shape, dtype=torch.bool)
    for r, heads, i in dirty.planted:
        for h in heads:
            hit[r, h, i] = hit[r, h, i + HALF] = True
    assert torch.equal(bits(got)[~hit], bits(was)[~hit]), "a non-finite value reached another element"
    assert not bool(got[hit].float().isfinite().any()), "a planted value did not reach both outputs of its pair"
    assert torch.equal(got.float().isnan(), ref.isnan()) and bool(ref.isnan()[hit].any()) and bool(ref.isinf()[hit].any())
    inf = ref.isinf()
    assert torch.equal(got.double()[inf], ref[inf])
    r0 = sum(n for _, n in SEQS_B[:SEQS_B.index((255, 100))])
    assert bool(got[r0 + 20, 2, 9].isnan()), "0 * Inf skipped"
    assert len(dirty.planted) == 5 + 3 * 2                                                # a table cell hits two sequences
    for r, heads, i in dirty.planted[:2] + dirty.planted[5:7]:                            # the NaN plants: NaN in both outputs
        assert bool(got[r, heads, i].float().isnan().all()) and bool(got[r, heads, i + HALF].float().isnan().all())
    # the rest of the K cache is untouched
    rest = dkc.clone()
    rest[dirty.blk, :, dirty.slot] = SENT16
    assert bool((rest == SENT16).all())


# ------------------------------------------------------------------------------------------------
# 3. append, then attend; chunked == whole
# ------------------------------------------------------------------------------------------------
def test_append_then_attend():
    """Identity table, q_len == ctx: the caches rope_append builds from packed K / V are, on the named slots,
    those of the decode module's paged_caches, and the prefill attention gives the same bits on both."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    group, hkv = 4, 2
    seqs = tuple((c, c) for c in (1, 32, 33, 97, 64, 130, 200, 0))
    c = Case("true", group, (seqs, hkv), seed=7901, identity=True)
    # the logical K and V per sequence, as the prefill module's builders want them: [Hkv, ctx, D]
    x = c.qkv_host[LEAD:LEAD + c.n]
    starts = [0] + torch.tensor([n for _, n in seqs]).cumsum(0).tolist()
    ks = [x[starts[s]:starts[s + 1], c.Hq:c.Hq + hkv].transpose(0, 1).float() for s in range(len(seqs))]
    vs = [x[starts[s]:starts[s + 1], c.Hq + hkv:].transpose(0, 1).float() for s in range(len(seqs))]
    kb, vb = ATT.paged_caches(ks, vs, c.table_host, c.NB, hkv)                    # NaN wherever no token lives
    named_k, named_v = ~kb.float().isnan(), ~vb.float().isnan()
    assert int(named_k.sum()) == int(named_v.sum()) == c.n * hkv * D
    c.run()
    got_q, got_kc, got_vc = c.results()
    assert torch.equal(got_q, x[:, :c.Hq])                                        # x1 * 1 - x2 * 0
    assert torch.equal(unsigned_zero(got_kc[named_k]), unsigned_zero(bits(kb)[named_k]))
    assert torch.equal(got_vc[named_v], bits(vb)[named_v])
    assert bool((got_kc[~named_k] == SENT16).all()) and bool((got_vc[~named_v] == SENT16).all())
    # the attention over the appended caches (SENT16 past ctx) and over paged_caches' (NaN past ctx)
    _, q_out, kc, vc = c.outs
    q, q_start = q_out[LEAD:LEAD + c.n], c.q_start - LEAD
    out_a = loadgen.paged_prefill_attention(q, kc, vc, c.table, c.ctx, q_start)
    out_b = loadgen.paged_prefill_attention(q, kb.cuda(), vb.cuda(), c.table, c.ctx, q_start)
    torch.cuda.synchronize()
    assert torch.equal(bits(out_a), bits(out_b)) and bool(out_a.float().isfinite().all())


def test_chunked_append_equals_whole():
    """True table: a prefix and then a chunk, in two launches, build the caches of one launch."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    group, hkv = 2, 2
    Hq, Ht = group * hkv, group * hkv + 2 * hkv
    seqs = SEQS_B
    g = torch.Generator().manual_seed(7902)
    ctxs = [c for c, _ in seqs]
    table, nb = PRE.block_tables(tuple(ctxs), g)
    full = torch.randn(sum(ctxs), Ht, D, generator=g).to(torch.bfloat16).cuda()
    cs = loadgen.rope_table(257).cuda()
    table, ctx = table.cuda(), torch.tensor(ctxs, dtype=torch.int32).cuda()
    starts = [0] + torch.tensor(ctxs).cumsum(0).tolist()
    csr = lambda lens: torch.tensor([0] + lens).cumsum(0).to(torch.int32).cuda()          # noqa: E731

    def caches():
        return (torch.full((nb, hkv, T, D), SENT16, dtype=torch.int16, device="cuda").view(torch.bfloat16),
                torch.full((nb, hkv, D, T), SENT16, dtype=torch.int16, device="cuda").view(torch.bfloat16))
    kc1, vc1 = caches()
    q1 = loadgen.rope_append(full, cs, kc1, vc1, table, ctx, csr(ctxs))
    kc2, vc2 = caches()
    pre = [c - n for c, n in seqs]
    pre_rows = torch.cat([torch.arange(starts[s], starts[s] + pre[s]) for s in range(len(seqs))]).cuda()
    new_rows = torch.cat([torch.arange(starts[s] + pre[s], starts[s + 1]) for s in range(len(seqs))]).cuda()
    qa = loadgen.rope_append(full[pre_rows], cs, kc2, vc2, table, torch.tensor(pre, dtype=torch.int32).cuda(), csr(pre))
    qb = loadgen.rope_append(full[new_rows], cs, kc2, vc2, table, ctx, csr([n for _, n in seqs]))
    torch.cuda.synchronize()
    assert torch.equal(bits(kc1), bits(kc2)) and torch.equal(bits(vc1), bits(vc2))
    assert torch.equal(bits(q1[pre_rows]), bits(qa)) and torch.equal(bits(q1[new_rows]), bits(qb))
    assert not bool((bits(kc1) == SENT16).all()) and bool((bits(kc1) == SENT16).any())


# ------------------------------------------------------------------------------------------------
# 4. other launch paths
# ------------------------------------------------------------------------------------------------
def test_no_check_and_a_larger_max_q_len_give_the_same():
    c = case("quarter", 4, "B")
    for kw in (dict(check=False, max_q_len=c.max_q_len), dict(check=False, max_q_len=c.max_q_len + 100),
               dict(max_q_len=c.max_q_len + 1000)):
        c.run(**kw)
        c.check(kw)


@pytest.mark.parametrize("breakage", ["block-NB", "block-minus-1", "duplicate-block", "ctx-past-table", "ctx-past-cos_sin",
                                      "q_len-above-ctx", "q_start-decreasing", "max_q_len-too-small"])
def test_check_raises_and_launches_nothing(breakage):
    c = case("quarter", 4, "A")
    s = [x[0] for x in c.seqs].index(256)                   # (256, 1): touches entry 7 only
    table, ctx, q_start, kw = c.table.clone(), c.ctx.clone(), c.q_start.clone(), {}
    if breakage == "block-NB":
        table[s, 7] = c.NB
    elif breakage == "block-minus-1":
        table[s, 7] = -1
    elif breakage == "duplicate-block":
        table[s, 7] = c.table[c.seqs.index((33, 33)), 1]
    elif breakage == "ctx-past-table":
        ctx[s] = T * c.max_blocks + 1
    elif breakage == "ctx-past-cos_sin":
        assert c.max_pos < 288 <= T * c.max_blocks
        ctx[s] = 288
        table[s, 8] = c.NB - 1
    elif breakage == "q_len-above-ctx":
        ctx[c.seqs.index((33, 33))] = 32
    elif breakage == "q_start-decreasing":
        q_start[3] = q_start[2] - 1
    else:
        kw["max_q_len"] = c.max_q_len - 1
    c.resentinel(c.outs)
    with pytest.raises(ValueError):
        c.launch(c.outs, table=table, ctx=ctx, q_start=q_start, **kw)
    assert c.untouched()


def test_untouched_table_entries_are_not_checked():
    """Entries of a row that the chunk does not touch may hold anything, the entries of earlier tokens included."""
    c = case("quarter", 4, "A")
    table = c.table.clone()
    table[[x[0] for x in c.seqs].index(256), :7] = SENT32
    c.resentinel(c.outs)
    c.launch(c.outs, table=table)
    c.check("untouched entries")


def test_side_stream_and_graph_replay():
    c = case("dyadic", 8, "A")
    s = torch.cuda.Stream()
    c.resentinel(c.outs)
    torch.cuda.synchronize()
    c.launch(c.outs, stream=s)
    s.synchronize()
    c.check("side stream")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        c.launch(c.outs, stream=s, check=False, max_q_len=c.max_q_len)
    for k in range(2):
        if k == 0:                       # the second replay writes over the first: idempotent
            c.resentinel(c.outs)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        s.synchronize()
        c.check(("replay", k))


def test_workgroups_match_the_python_rule(hip):
    from k8s_gpu_scheduler_amd.models import workloads as W
    for S, hkv, mq in ((1, 1, 1), (8, 2, 33), (2, 8, 1024), (256, 8, 1), (3, 1, 2), (5, 4, 0), (0, 4, 7), (7, 3, 34),
                       (1, 1, 2 ** 31 - 1)):
        assert hip.rope_append_workgroups(S, hkv, mq) == W.default_rope_append_workgroups(S, hkv, mq)
    assert hip.rope_append_workgroups(2, 8, 1024) == 2 * 8 * 33 and hip.rope_append_workgroups(256, 8, 1) == 256 * 8
    assert [hip.rope_append_workgroups(1, 1, mq) for mq in (1, 2, 3, 33, 34, 35)] == [1, 2, 2, 2, 3, 3]


# ------------------------------------------------------------------------------------------------
# 5. beside a co-running load
# ------------------------------------------------------------------------------------------------
class AppendLaunch:
    """One launch on a Case's inputs into outputs of its own (reset / enqueue / check, as the co-run
    module's CaseLaunch has)."""

    def __init__(self, c, what):
        self.case, self.what = c, what
        self.outs = c.new_outputs()

    def reset(self):
        self.case.resentinel(self.outs)

    def enqueue(self, st):
        self.case.launch(self.outs, stream=st, check=False, max_q_len=self.case.max_q_len)

    def check(self, tag):
        self.case.check((tag, self.what), self.outs)


@pytest.mark.parametrize("aggressor,mode", [pytest.param(a, m, id=f"{a}-{m}") for a, m in CO.BASE_PAIRS])
def test_rope_append_corun(hip, aggressor, mode):
    c = case("dyadic", 4, "B")
    victim = CO.Load("rope-append-dyadic", {}, [AppendLaunch(c, ("dyadic", 4, "B", r)) for r in range(CO.R)])
    try:
        CO.corun(hip, victim, CO.aggressor_for(aggressor, mode), mode)
    finally:
        CO.restore_knobs(hip)


# ------------------------------------------------------------------------------------------------
# 6. pod path
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("workload", ["llm_layer_decode_256", "llm_layer_prefill_2048"])
def test_podrun_llm_layer(workload):
    p = subprocess.run([sys.executable, "-m", "k8s_gpu_scheduler_amd.ops.podrun", "--workload", workload,
                        "--iters", "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    assert res["workload"] == workload and res["iters"] == 2 and res["throughput"] > 0


@pytest.mark.parametrize("workload", ["llm_layer_decode_256", "llm_layer_prefill_2048"])
def test_executor_llm_layer_buffers_and_append_output(workload):
    """The executor's operands, and after one iteration 8 picked rows of q_out (op_output), their K slots and
    their V slots against the reference."""
    from k8s_gpu_scheduler_amd.models import workloads as W
    from k8s_gpu_scheduler_amd.parallel.executor import _Buffers, enqueue_ops, op_output
    dev = torch.device("cuda", 0)
    w = W.get(workload)
    a = _Buffers(w, dev)
    o, t = a.ops[1]
    q_out, qkv, cos_sin, kc, vc, table, ctx, q_start = t
    nb = o.M * o.K // T
    assert o.kind == "rope_append" and op_output(o, t) is q_out
    assert qkv.shape == (o.M * o.q, o.N + 2 * o.rows, D) and q_out.shape == (o.M * o.q, o.N, D)
    assert cos_sin.shape == (o.K, D) and cos_sin.dtype == torch.float32
    assert kc.shape == (nb, o.rows, T, D) and vc.shape == (nb, o.rows, D, T)
    assert torch.equal(table.flatten().sort().values, torch.arange(nb, dtype=torch.int32, device=dev))     # a permutation
    assert bool((ctx == o.K).all()) and q_start.tolist() == [s * o.q for s in range(o.M + 1)]
    q_out.view(torch.int16).fill_(SENT16)
    kc.view(torch.int16).fill_(SENT16)
    vc.view(torch.int16).fill_(SENT16)
    enqueue_ops(a, 1, torch.cuda.current_stream(), 0)
    torch.cuda.synchronize()
    picks = [(0, 0), (0, o.q - 1), (o.M - 1, 0), (o.M - 1, o.q - 1), (1, o.q // 2), (o.M // 2, o.q // 3),
             (1, (T - (o.K - o.q) % T) % o.q), (o.M - 1, o.q * 3 // 4)]
    rows = torch.tensor([s * o.q + i for s, i in picks], device=dev)
    pos = torch.tensor([o.K - o.q + i for _, i in picks], device=dev)
    seq = torch.tensor([s for s, _ in picks], device=dev)
    x = qkv[rows].double().cpu()
    ref = rotate(x[:, :o.N + o.rows], cos_sin[pos].double().cpu()[:, None, :])
    blk = table[seq, pos // T].long()
    got = torch.cat([q_out[rows], kc[blk, :, pos % T]], dim=1).double().cpu()
    xa = x[:, :o.N + o.rows].abs()
    b = TRUE_BOUND * (xa[..., :HALF] + xa[..., HALF:])
    err = (got - ref).abs()
    print(f"{workload} append, 8 rows: max |out - ref| / bound = {(err / torch.cat([b, b], -1).clamp_min(1e-300)).max().item():.4f}")
    assert bool((err <= torch.cat([b, b], dim=-1)).all())
    assert torch.equal(bits(vc[blk, :, :, pos % T]), bits(qkv[rows, o.N + o.rows:]))
    assert not bool((q_out.view(torch.int16) == SENT16).all(-1).any())                   # every row was written
    written = o.M * o.q * o.rows * D                                                     # cells per cache the chunks own
    assert int((kc.view(torch.int16) != SENT16).sum()) <= written and int((vc.view(torch.int16) != SENT16).sum()) <= written
    del a, t, q_out, qkv, kc, vc
    torch.cuda.empty_cache()
