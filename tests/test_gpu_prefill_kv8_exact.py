"""Exact-arithmetic, guarded-buffer tests of the chunked-prefill attention over an FP8 paged-KV cache
(loadgen.paged_prefill_attention_kv8, native/hip/prefill_attn_kv8.hip; run with `-m gpu` on an MI355X).
The sequence lists, shapes, DELTAS, guards and the float64 reference are those of test_gpu_prefill_attn_exact.py
(PRE); the code drawing, the byte conversion, the scale sweep and the NaN byte those of test_gpu_decode_kv8_exact.py
(KV8); neither module is changed.

THE FORMAT (native/hip/api.h): a stored byte c of KV head g stands for e4m3fn(c) * scale[g].  The reference is
PRE.reference on loadgen.dequantize_kv8_reference of the byte caches with the scales applied per head -- float64
logical K and V -- so scale * k_scale and * v_scale are in it by construction.  e4m3fn -> bf16 is exact, the kernel
keeps the bf16 MFMAs and the fp32 softmax, and with power-of-two scales PRE's exact regimes stay exact; the
comparison is `torch.equal`:

  match    the stored K rows are +-16 with k_scale = 2^-2 (+-32 under 2^-3 on the second head): the logical K is
           PRE's 4 H, q is PRE's, a matched score is 362 and every other 0.  V is drawn from the e4m3fn codes of six
           binades (magnitude codes 0x18 .. 0x47).  out = bf16(v_scale V[t]) or bf16(v_scale (V[t1] + V[t2]) / 2).
           Asserted on the reference alone: the float64 softmax rounded float64 -> fp32 -> bf16 equals that value in
           every column, every launch has a trap at p + 1, those of SEQS_B one at p + 128, and some expectation is
           no bf16 value before the rounding.
  uniform  q = 0, K random finite codes (all 254), V integers in [-4, 4]:
           out = bf16(fp32(sum_{t <= p} V) / fp32(p + 1) * v_scale), computed as PRE computes it, v_scale a power of
           two.

Unnamed blocks and the slots past ctx hold the NaN byte 0x7F in both caches; k_scale and v_scale start one element
into NaN-filled allocations; q, out, the table, ctx_lens and q_start are guarded as in PRE.  The exact regimes run
over PRE.SHAPES and both sequence lists with KV8.scales_for's sweep (v_scale cycling through 1, 2^-3, 4; per-head
differing k_scale and v_scale at two KV heads).

The random regimes, |out - ref| <= 2^-7 * v_scale * max|e4m3(V)| (the project's bound: its derivation is in
test_gpu_decode_attn_exact.py and carries over because dequantisation is exact and the two scales are single fp32
multiplies), k_scale = 0.37, v_scale = 1.9, V codes of magnitude <= 1:

  random   KV8's cache values: K codes of magnitude <= 2, q randn.
  wide     K drawn from all 254 finite codes (up to 448: K's conversion over the whole range); q is randn scaled
           down by the power of two that brings the largest |score| of the reference, over every (row, token < ctx)
           pair, to at most 16 -- asserted on the reference alone.

A -0.0 code (0x80) that a column matches alone gives +0.0: the products of the other tokens (probability 0) are
added to it, and the MFMA's accumulator starts at +0.0; (+0.0) + (-0.0) is +0.0.  test_all_codes checks exactly that
bit pattern for 0x80 and the bits of bf16(e4m3(c) * v_scale) for every other finite code.
"""
import functools

import pytest
import torch

import test_gpu_corun_exact as CO
import test_gpu_decode_attn_exact as ATT
import test_gpu_decode_kv8_exact as KV8
import test_gpu_prefill_attn_exact as PRE
from test_gpu_kernels_exact import NAN, SENT16, SENT32, guarded_input, guarded_output, guards_intact

pytestmark = pytest.mark.gpu

# MEASURED on an MI355X (printed by the tests):
MEASURED = """
  max|out - ref| over the shapes: random regime 0.00349 .. 0.00602, wide regime 0.00423 .. 0.00560 (bound 0.01484 =
  2^-7 * 1.9 * 1).  All codes: every finite code exact at both shapes with the one-instruction conversion
  (v_cvt_scalef32_pk_bf16_fp8, scale 1.0), 0x7F and 0xFF NaN, 0x80 gives +0.0.  Co-run (4 launches per victim): the
  victim's slowdown 0.50 .. 1.16; every output bit-exact.  The large-address case (two caches of 4 GiB + 512 KiB
  from torch.empty): 0.14 s.  The module: 78 tests in 5 s.
"""

D, T, C0 = PRE.D, PRE.T, PRE.C0
R0, LEAD, TRAIL = PRE.R0, PRE.LEAD, PRE.TRAIL
FP8, U8 = torch.float8_e4m3fn, torch.uint8
NAN8 = KV8.NAN8
EXACT = ("match", "uniform")
REGIMES = ("match", "uniform", "random", "wide")
SCORE_CAP = 16.0


def lg():
    from k8s_gpu_scheduler_amd.ops import loadgen
    return loadgen


@pytest.fixture(scope="module")
def hip():
    from k8s_gpu_scheduler_amd import _native
    return _native.hip(required=True)


def guarded_scale(values):
    """(raw, view): the fp32 vector starting one element into a NaN-filled allocation."""
    raw = torch.full((1 + len(values) + 3,), NAN, dtype=torch.float32, device="cuda")
    view = raw[1:1 + len(values)]
    view.copy_(torch.tensor(values, dtype=torch.float32))
    return raw, view


class Case:
    """One launch's operands, guarded, with the float64 reference and, in the exact regimes, the expectation."""

    def __init__(self, regime, group, hkv, seqs, k_scale, v_scale, seed):
        g = torch.Generator().manual_seed(seed)
        self.regime, self.S, self.Hq, self.hkv, self.seqs, self.group = regime, len(seqs), group * hkv, hkv, seqs, group
        ctxs = tuple(c for c, _ in seqs)
        self.n = sum(n for _, n in seqs)
        self.Tq = LEAD + self.n + TRAIL
        table, nb = PRE.block_tables(ctxs, g)
        ksc, vsc = torch.tensor(k_scale, dtype=torch.float32), torch.tensor(v_scale, dtype=torch.float32)
        if regime == "match":
            q, ks, _ = PRE.logical_operands("match", group, hkv, seqs, g)
            ks = [k / ksc.view(hkv, 1, 1) for k in ks]                           # logical +-4 -> stored +-4 / k_scale[g]
            assert all(bool((k[0].abs() == 16).all()) and bool((k[-1].abs() == 4 / k_scale[-1]).all()) for k in ks if k.numel())
            vs = [KV8.codes((hkv, c, D), 0x18, 0x48, g) for c in ctxs]           # six binades
        elif regime == "uniform":
            q = torch.zeros(self.n, self.Hq, D)
            ks = [KV8.codes((hkv, c, D), 0, 0x7F, g) for c in ctxs]
            vs = [torch.randint(-4, 5, (hkv, c, D), generator=g).float() for c in ctxs]
        else:
            q = torch.randn(self.n, self.Hq, D, generator=g).to(torch.bfloat16).float()
            ks = [KV8.codes((hkv, c, D), 0, 0x7F if regime == "wide" else 0x41, g) for c in ctxs]
            vs = [KV8.codes((hkv, c, D), 0, 0x39, g) for c in ctxs]              # |value| <= 1
        if regime == "wide":
            assert {int(b) for k in ks for b in KV8.to_bytes(k.to(torch.bfloat16)).unique()} == set(range(256)) - {0x7F, 0xFF}
            q = q * 2.0 ** -self.shift_for(q, ks, ksc)
        kb, vb = ATT.paged_caches(ks, vs, table, nb, hkv)                        # bf16, NaN wherever no token lives
        self.k_bytes, self.v_bytes = KV8.to_bytes(kb), KV8.to_bytes(vb)
        named = torch.zeros(nb, dtype=torch.bool)
        named[table[table != SENT32].long()] = True
        assert bool((self.k_bytes[~named] == NAN8).all()) and bool((self.v_bytes[~named] == NAN8).all())
        for s, c in enumerate(ctxs):
            if c % T:
                blk = int(table[s, c // T])
                assert bool((self.k_bytes[blk, :, c % T:] == NAN8).all()) and bool((self.v_bytes[blk, :, :, c % T:] == NAN8).all())
        ctx = torch.tensor(ctxs, dtype=torch.int32)
        q_start = torch.tensor([LEAD] + [n for _, n in seqs]).cumsum(0).to(torch.int32)
        qfull = torch.full((self.Tq, self.Hq, D), NAN)
        qfull[LEAD:LEAD + self.n] = q
        qb = qfull.to(torch.bfloat16)
        assert torch.equal(qb[LEAD:LEAD + self.n].float(), q)                    # the operands are exact
        kd = lg().dequantize_kv8_reference(self.k_bytes, ksc.view(1, hkv, 1, 1))
        vd = lg().dequantize_kv8_reference(self.v_bytes, vsc.view(1, hkv, 1, 1))
        self.ref = PRE.reference(qb, kd, vd, table, ctx, q_start)[LEAD:LEAD + self.n]
        assert bool(self.ref.isfinite().all())
        if regime == "wide":
            assert self.max_score(qb[LEAD:LEAD + self.n].float(), ks, ksc) <= SCORE_CAP
        self.vmax = max([float((v.abs() * vsc.view(hkv, 1, 1)).max()) for v in vs if v.numel()] + [0.0])
        self.NB, self.max_blocks, self.max_q_len, self.host_table = nb, table.shape[1], max(n for _, n in seqs), table
        W = self.W = self.Hq * D
        self.q = guarded_input(qb.view(self.Tq, W).cuda(), W + C0, c0=C0).unflatten(1, (self.Hq, D))
        self.kc, self.vc = self.k_bytes.cuda().view(FP8), self.v_bytes.cuda().view(FP8)
        self.k_scale_raw, self.k_scale = guarded_scale(k_scale)
        self.v_scale_raw, self.v_scale = guarded_scale(v_scale)
        self.table_raw, self.table = ATT.guarded_ints_2d(table, self.max_blocks + 2)
        self.ctx_raw, self.ctx = PRE.guarded_ints(ctx)
        self.q_start_raw, self.q_start = PRE.guarded_ints(q_start)
        self.raw, self.out = self.new_output()
        assert self.q.data_ptr() % 16 == 0 and self.out.data_ptr() % 16 == 0 and self.k_scale.data_ptr() % 16 == 4
        assert self.table.stride(0) > self.max_blocks
        if regime in EXACT:
            kv = torch.arange(self.Hq) // group
            if regime == "match":
                exact, facts = PRE.exact_expectation("match", group, hkv, seqs, [v * vsc.view(hkv, 1, 1) for v in vs])
                assert facts["trap1"] and facts["two"] > 0 and (facts["trap128"] or seqs is PRE.SEQS_A), facts
                f = exact.float()
                assert torch.equal(f.double(), exact)
                assert bool((f.to(torch.bfloat16).double() != exact).any()), "every expectation is a bf16 value"
                assert torch.equal(self.ref.float().to(torch.bfloat16), f.to(torch.bfloat16))      # softmax == exact mean
            else:
                quot, _ = PRE.exact_expectation("uniform", group, hkv, seqs, vs)                   # fp32 quotients, as float64
                f = quot.float() * vsc[kv].view(1, self.Hq, 1)                                     # a power of two: exact
                nz = quot != 0
                assert torch.equal(self.ref.float().to(torch.bfloat16)[nz], f.to(torch.bfloat16)[nz])
            self.exp = f.to(torch.bfloat16).cuda()

    def scores(self, q, ks, ksc):
        """max |scale * k_scale * q . K| over every (row, token < ctx) pair, per sequence (float64)."""
        r, worst = 0, 0.0
        for (c, n), k in zip(self.seqs, ks):
            if n:
                qs = q[r:r + n].double().view(n, self.hkv, self.group, D)
                sc = torch.einsum("ngcd,gtd->ngct", qs, (k * ksc.view(self.hkv, 1, 1)).double()) * PRE.SCALE
                worst = max(worst, float(sc.abs().max()))
            r += n
        return worst

    max_score = scores

    def shift_for(self, q, ks, ksc):
        worst, shift = self.scores(q, ks, ksc), 0
        while worst * 2.0 ** -shift > SCORE_CAP:
            shift += 1
        return shift

    def new_output(self):
        raw, out2d = guarded_output(self.Tq, self.W, self.W + C0, C0, "cuda")
        return raw, out2d.unflatten(1, (self.Hq, D))

    def resentinel(self):
        self.raw.fill_(SENT16)

    def launch(self, out, **kw):
        args = dict(q=self.q, kc=self.kc, vc=self.vc, table=self.table, ctx=self.ctx, q_start=self.q_start,
                    k_scale=self.k_scale, v_scale=self.v_scale)
        args.update({k: kw.pop(k) for k in list(kw) if k in args})
        return lg().paged_prefill_attention_kv8(args["q"], args["kc"], args["vc"], args["table"], args["ctx"], args["q_start"],
                                                k_scale=args["k_scale"], v_scale=args["v_scale"], out=out, **kw)

    def run(self, **kw):
        return self.launch(self.out, **kw)

    def guards(self, what, raw=None):
        torch.cuda.synchronize()
        written = (slice(R0 + LEAD, R0 + LEAD + self.n), slice(C0, C0 + self.W))
        assert guards_intact(self.raw if raw is None else raw, written, SENT16), ("write outside the chunks' rows", what)

    def check(self, what, raw=None, out=None):
        self.guards(what, raw)
        got = (self.out if out is None else out)[LEAD:LEAD + self.n]
        if self.regime not in EXACT:
            err = (got.double().cpu() - self.ref).abs().max().item()
            print(f"kv8 prefill attention, {self.regime} regime {what}: max|out - ref| = {err:.5f} "
                  f"(bound {ATT.RANDOM_BOUND * self.vmax:.5f}, v_scale * max|V| = {self.vmax:.4f})")
            assert err <= ATT.RANDOM_BOUND * self.vmax, (what, err)
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
def _case(regime, group, hkv, k_scale, v_scale):
    return Case(regime, group, hkv, PRE.SEQS_A if hkv == 1 else PRE.SEQS_B, list(k_scale), list(v_scale),
                seed=9000 + 1000 * REGIMES.index(regime) + 10 * group + hkv)


def case(regime, group, hkv, i=None):
    i = PRE.SHAPES.index((group, hkv)) if i is None else i
    ks, vs = KV8.scales_for("onehot" if regime in EXACT else "random", hkv, i)
    return _case(regime, group, hkv, tuple(ks), tuple(vs))


# ------------------------------------------------------------------------------------------------
# 1. the regimes over every group size
# ------------------------------------------------------------------------------------------------
def test_the_scale_sweep_covers_what_it_claims():
    seen = [tuple(KV8.scales_for("onehot", hkv, i)[1]) for i, (_, hkv) in enumerate(PRE.SHAPES)]
    assert {v for vs in seen for v in vs} == set(KV8.V_SCALES) == {1.0, 2.0 ** -3, 4.0}
    assert any(len(vs) == 2 and vs[0] != vs[1] for vs in seen)
    ks, _ = KV8.scales_for("onehot", 2, 0)
    assert ks == [2.0 ** -2, 2.0 ** -3]


@pytest.mark.parametrize("group,hkv", PRE.SHAPES)
@pytest.mark.parametrize("regime", REGIMES)
def test_regimes(hip, regime, group, hkv):
    c = case(regime, group, hkv)
    c.resentinel()
    c.run()
    c.check((regime, group, hkv))


@pytest.mark.parametrize("group,hkv", [(4, 1), (1, 2)])
def test_all_codes(group, hkv):
    """Two sequences of (ctx, q_len) = (2, 2) and (34, 2): chunk token i at position p matches token p alone (K of
    token t is the sign row t, q of the column the sign row p), and the two chunk tokens' V rows hold the codes
    0 .. 127 and 128 .. 255 -- in the second sequence in slots 0 and 1 of a block whose other slots are past ctx."""
    H = ATT.hadamard()
    seqs = ((2, 2), (34, 2))
    Hq = group * hkv
    k_scale, v_scale = ([0.25], [2.0 ** -3]) if hkv == 1 else ([0.25, 0.125], [1.0, 2.0 ** -3])
    g = torch.Generator().manual_seed(9900 + group)
    table = torch.tensor([[2, SENT32], [3, 0]], dtype=torch.int32)              # block 1 is named by no entry
    kc = torch.full((4, hkv, T, D), NAN8, dtype=U8)
    vc = torch.full((4, hkv, D, T), NAN8, dtype=U8)
    rows = []
    for s, (ctx, n) in enumerate(seqs):
        for t in range(ctx):
            blk = int(table[s, t // T])
            for kv in range(hkv):
                kc[blk, kv, t % T] = lg().quantize_kv8_reference(4 * H[t] / k_scale[kv])
                vc[blk, kv, :, t % T] = (torch.randint(0, 0x7F, (D,), generator=g) | (torch.randint(0, 2, (D,), generator=g) << 7)).to(U8)
        for i in range(n):
            p = ctx - n + i
            blk = int(table[s, p // T])
            vc[blk, :, :, p % T] = torch.arange(128 * i, 128 * i + 128, dtype=torch.int32).to(U8)
            rows.append((8 * H[p])[None].repeat(Hq, 1))
    q = torch.stack(rows).to(torch.bfloat16).cuda()                              # [4, Hq, D]
    q_start = torch.tensor([0, 2, 4], dtype=torch.int32).cuda()
    ctx = torch.tensor([c for c, _ in seqs], dtype=torch.int32).cuda()
    out = lg().paged_prefill_attention_kv8(q, kc.cuda().view(FP8), vc.cuda().view(FP8), table.cuda(), ctx, q_start,
                                           k_scale=torch.tensor(k_scale).cuda(), v_scale=torch.tensor(v_scale).cuda()).cpu()
    all_codes = torch.arange(256, dtype=torch.int32).to(U8)
    seen = 0
    for h in range(Hq):
        want = (lg().dequantize_kv8_reference(all_codes, 1.0) * v_scale[h // group]).float().to(torch.bfloat16)
        want[0x80] = 0.0                                                          # (+0.0) + (-0.0): the module docstring
        fin = ~want.float().isnan()
        assert int(fin.sum()) == 254
        for s in range(2):
            got = out[2 * s:2 * s + 2, h].reshape(256)
            assert bool(got[0x7F].isnan()) and bool(got[0xFF].isnan()) and int(got.float().isnan().sum()) == 2
            bad = (got.view(torch.int16)[fin] != want.view(torch.int16)[fin]).nonzero().flatten().tolist()
            assert not bad, (group, hkv, h, s, [hex(int(all_codes[fin][b])) for b in bad[:8]])
            seen += int(fin.sum())
    assert seen == 254 * 2 * Hq


@pytest.mark.parametrize("group,hkv", PRE.SHAPES)
@pytest.mark.parametrize("regime", EXACT)
def test_chunks_of_one_token_are_the_kv8_decode_attention(regime, group, hkv):
    """The sequences with q_len == 1, through paged_decode_attention_kv8 on the same operands: the same bits."""
    c = case(regime, group, hkv)
    c.resentinel()
    c.run()
    c.check((regime, group, hkv))
    starts = c.q_start.tolist()
    ones = [s for s, (_, n) in enumerate(c.seqs) if n == 1]
    assert ones
    rows = torch.tensor([starts[s] for s in ones]).cuda()
    sel = torch.tensor(ones).cuda()
    dec = lg().paged_decode_attention_kv8(c.q[rows].contiguous(), c.kc, c.vc, c.table[sel].contiguous(), c.ctx[sel].contiguous(),
                                          k_scale=c.k_scale, v_scale=c.v_scale)
    assert torch.equal(dec.view(torch.int16), c.out[rows].view(torch.int16))


def test_no_check_and_a_larger_max_q_len_give_the_same():
    """Strided q / out windows and a table row stride above max_blocks are in every case; here also check=False and a
    max_q_len larger than every chunk, whose extra workgroups exit."""
    c = case("match", 4, 2)
    for kw in (dict(check=False, max_q_len=c.max_q_len), dict(check=False, max_q_len=c.max_q_len + 3 * PRE.COLUMNS + 5),
               dict(max_q_len=c.max_q_len + 1000)):
        c.resentinel()
        c.run(**kw)
        c.check(kw)


def test_empty_launches_leave_out_untouched():
    c = case("match", 2, 2)
    c.resentinel()
    c.run(check=False, max_q_len=0)
    assert c.untouched()
    lg().paged_prefill_attention_kv8(c.q, c.kc, c.vc, c.table[:0], c.ctx[:0], c.q_start[:1], k_scale=c.k_scale,
                                     v_scale=c.v_scale, out=c.out)
    assert c.untouched()
    lg().paged_prefill_attention_kv8(c.q, c.kc, c.vc, c.table[:0], c.ctx[:0], c.q_start[:1], k_scale=c.k_scale,
                                     v_scale=c.v_scale, out=c.out, check=False, max_q_len=7)
    assert c.untouched()


# ------------------------------------------------------------------------------------------------
# 2. NaN bytes inside and past ctx
# ------------------------------------------------------------------------------------------------
def test_nan_inside_ctx_propagates_and_past_ctx_does_not():
    """The 0x7F filler past ctx and in the unnamed blocks never shows (every case's check says so).  A NaN byte in K at
    token 0 of one (sequence, KV head) -- at or below every position -- makes every row of that sequence's chunk NaN
    for the KV head's group; one in V at (token 0, d) makes element d of those rows NaN; nothing else changes."""
    c = case("match", 4, 2)
    c.resentinel()
    c.run()
    c.check("base")
    base = c.out.clone()
    s = c.seqs.index((255, 100))
    kv, d, g = 1, 41, c.group
    starts = c.q_start.tolist()
    blk = int(c.host_table[s, 0])
    rows = slice(starts[s], starts[s + 1])
    vc = c.vc.clone()
    vc.view(U8)[blk, kv, d, 0] = NAN8
    c.resentinel()
    c.run(vc=vc)
    c.guards("NaN in V")
    mask = torch.zeros_like(base, dtype=torch.bool)
    mask[rows, kv * g:(kv + 1) * g, d] = True
    assert bool(c.out[mask].isnan().all()) and torch.equal(c.out.view(torch.int16)[~mask], base.view(torch.int16)[~mask])
    kc = c.kc.clone()
    kc.view(U8)[blk, kv, 0, 5] = NAN8 | 0x80
    c.resentinel()
    c.run(kc=kc)
    c.guards("NaN in K")
    mask = torch.zeros_like(base, dtype=torch.bool)
    mask[rows, kv * g:(kv + 1) * g] = True
    assert bool(c.out[mask].isnan().all()) and torch.equal(c.out.view(torch.int16)[~mask], base.view(torch.int16)[~mask])


# ------------------------------------------------------------------------------------------------
# 3. check=True; side stream and graph replay
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("breakage", ["block-NB", "q_len-above-ctx", "max_q_len-too-small", "k_scale-zero", "v_scale-nan"])
def test_check_raises_and_launches_nothing(breakage):
    c = case("match", 4, 1)
    s = [x[0] for x in c.seqs].index(256)
    kw = {}
    if breakage == "block-NB":
        kw["table"] = c.table.clone()
        kw["table"][s, 7] = c.NB
    elif breakage == "q_len-above-ctx":
        kw["ctx"] = c.ctx.clone()
        kw["ctx"][c.seqs.index((33, 33))] = 32
    elif breakage == "max_q_len-too-small":
        kw["max_q_len"] = c.max_q_len - 1
    else:
        name, value = breakage.split("-")
        kw[name] = torch.tensor([{"zero": 0.0, "nan": NAN}[value]]).cuda()
    c.resentinel()
    with pytest.raises(ValueError):
        c.run(**kw)
    assert c.untouched()


def test_wrapper_raises_on_the_device_too():
    c = case("match", 4, 1)
    with pytest.raises(ValueError, match="need k_scale and v_scale"):
        lg().paged_prefill_attention_kv8(c.q, c.kc, c.vc, c.table, c.ctx, c.q_start, out=c.out)
    with pytest.raises(TypeError, match="bf16"):
        lg().paged_prefill_attention(c.q, c.kc, c.vc, c.table, c.ctx, c.q_start, out=c.out)
    with pytest.raises(ValueError, match="paged_prefill_attention reads them"):
        lg().paged_prefill_attention_kv8(c.q, torch.zeros(c.kc.shape, dtype=torch.bfloat16, device="cuda"),
                                         torch.zeros(c.vc.shape, dtype=torch.bfloat16, device="cuda"), c.table, c.ctx, c.q_start)
    c.resentinel()
    assert c.untouched()


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
# 4. beside a co-running load
# ------------------------------------------------------------------------------------------------
class Launch:
    """One launch on a Case's inputs into an output of its own (reset / enqueue / check, as CO's CaseLaunch has)."""

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
def test_prefill_kv8_corun(hip, aggressor, mode):
    c = case("match", 4, 2)
    victim = CO.Load("prefill-kv8", {}, [Launch(c, ("match", 4, 2, r)) for r in range(CO.R)])
    try:
        CO.corun(hip, victim, CO.aggressor_for(aggressor, mode), mode)
    finally:
        CO.restore_knobs(hip)


# ------------------------------------------------------------------------------------------------
# 5. addresses past 4 GiB
# ------------------------------------------------------------------------------------------------
def test_large_addresses():
    """KV8's large-address layout on the match regime: FP8 caches of 4 GiB + 512 KiB from torch.empty, only the named
    blocks and the decoys written.  Compact ids >= 32 become physical ids >= HIGH + 32: byte offset > 2^32.  A 32-bit
    byte offset would send such a block to physical block c in [32, 64), which no entry names and which holds finite
    decoys: a wrong value, not a fault."""
    HIGH, LOW_IDS, BIG_NB = KV8.HIGH, KV8.LOW_IDS, KV8.BIG_NB
    c = Case("match", KV8.BIG_GROUP, KV8.BIG_HKV, PRE.SEQS_B, [2.0 ** -2, 2.0 ** -3], [4.0, 2.0 ** -3], seed=9990)
    assert HIGH * KV8.BLOCK_BYTES == 1 << 32 and c.NB <= 2 * LOW_IDS
    table = c.host_table.clone()
    g = torch.Generator().manual_seed(9991)
    low, high = torch.randperm(LOW_IDS, generator=g).tolist(), (LOW_IDS + torch.randperm(LOW_IDS, generator=g)).tolist()
    remap = {}
    for s in range(table.shape[0]):
        for j in range(table.shape[1]):
            if int(table[s, j]) != SENT32:
                remap[int(table[s, j])] = (low if (j // 4 + j + s) % 2 == 0 else high).pop()
                table[s, j] = remap[int(table[s, j])]
    named = table[table != SENT32]
    assert int(named.max()) < 64 and named.numel() == named.unique().numel() == len(remap)
    assert bool((named >= LOW_IDS).any()) and bool((named < LOW_IDS).any())
    phys = KV8.physical(table)
    assert int(phys[phys != SENT32].max()) * KV8.BLOCK_BYTES > 1 << 32
    src = torch.tensor(sorted(remap), dtype=torch.int64)
    dst = KV8.physical(torch.tensor([remap[int(b)] for b in src], dtype=torch.int64)).cuda()
    kc = torch.empty((BIG_NB, KV8.BIG_HKV, T, D), dtype=U8, device="cuda")
    vc = torch.empty((BIG_NB, KV8.BIG_HKV, D, T), dtype=U8, device="cuda")
    assert kc.numel() > 1 << 32
    for x in (kc, vc):
        x[LOW_IDS:64] = 0x30                                                      # decoys: 0.5 everywhere
        x[:LOW_IDS] = NAN8
        x[HIGH + LOW_IDS:] = NAN8
    kc[dst] = c.k_bytes[src].cuda()
    vc[dst] = c.v_bytes[src].cuda()
    _, tview = ATT.guarded_ints_2d(phys.to(torch.int32), c.max_blocks + 2)
    c.resentinel()
    c.run(kc=kc.view(FP8), vc=vc.view(FP8), table=tview)
    c.check("large addresses")
    del c, kc, vc
    torch.cuda.empty_cache()
