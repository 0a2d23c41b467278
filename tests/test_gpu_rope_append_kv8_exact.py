"""Exact-arithmetic, guarded-buffer tests of the RoPE + append into an FP8 paged-KV cache (loadgen.rope_append with
float8_e4m3fn caches; run with `-m gpu` on an MI355X).  The Case machinery, the sequence lists SEQS_A / B / C, the
regimes and the guards are those of test_gpu_rope_append_exact.py (ROPE), which is not changed: Case8 below replaces
the caches by byte caches that are wholly SENT8 before a launch and compared whole afterwards, and adds the scales.

The reference is loadgen.rope_append_kv8_reference: the float64 rotation cast to fp32 once, an fp32 division by the
KV head's scale and THE QUANTISATION RULE in integer arithmetic (quantize_kv8_reference, pinned on literal vectors in
test_kv8_cpu.py).

  quarter, dyadic   y is exact in fp32 (ROPE's Case asserts it), so the kernel's fp32 y is the reference's, the division
                    is the same IEEE operation, and the cache bytes must EQUAL the reference bytes; q_out is bit-equal as
                    in ROPE.  Scales: powers of two {1, 2^-3, 4}, and at two KV heads a different one per head.
  true              k_scale = 1/16 (asserted on the reference: nothing saturates).  With z = y64 / k_scale the exact
                    quotient, the stored value deq satisfies
                        |k_scale * deq - y64| <= k_scale * max(2^-4 |z|, 2^-10) + 2^-20 (|x1| + |x2|):
                    the kernel divides z' with |z' - z| <= delta / k_scale, where delta collects the fp32 product, FMA
                    and division roundings, each below 2^-24 (|x1| + |x2|) because |y| <= |x1| + |x2|: delta <
                    2^-22 (|x1| + |x2|).  Rounding z' to e4m3fn moves it by at most half a step, and a step is 2^-3 of
                    the lower end of its binade (2^-9 for the subnormals), so half a step is at most
                    max(2^-4 |z'|, 2^-10) <= max(2^-4 |z|, 2^-10) + 2^-4 delta / k_scale.  Together
                    |k_scale * deq - y64| <= k_scale * max(2^-4 |z|, 2^-10) + (1 + 2^-4) delta, and (1 + 2^-4) delta is
                    below 2^-21 (|x1| + |x2|); the bound keeps a factor of two over that.  A near-tie that the
                    perturbation carries to the other neighbour is inside this: the stored value is then still the
                    nearest to z', which is what the derivation uses.
                    The measured maximum of the ratio is printed.
V is quantised from bf16 by the same rule and is exact in every regime: its bytes always equal the reference, for
random bit patterns (NaN -> 0x7F | sign, +-Inf and everything past 464 -> 0x7E | sign, -0.0 -> 0x80), and
test_v_exhaustive runs all 65,536 bf16 patterns under v_scale in {1, 2^-3, 4, 0.75}.
"""
import functools

import pytest
import torch

import test_gpu_corun_exact as CO
import test_gpu_prefill_attn_exact as PRE
import test_gpu_rope_append_exact as ROPE
from test_gpu_kernels_exact import SENT16, guarded_output, guards_intact

pytestmark = pytest.mark.gpu

MEASURED = """
  true regime, K: max |k_scale deq - y64| / bound per (group, sequences) 0.9412 .. 0.9910, the largest at (1, C); 0 of
  22,912 .. 124,672 K bytes differ from the reference bytes (the fp32 FMA never crossed a tie here); q_out ratio
  0.9111 .. 0.9714 of ROPE's bound.  V exhaustive: every byte equal under all four scales.  Co-run (4 launches per
  victim): the victim's slowdown 0.42 .. 0.78; every output bit-exact.  The module: 46 tests in 4.1 s.
"""

D, T, C0, HALF = ROPE.D, ROPE.T, ROPE.C0, ROPE.HALF
R0, LEAD = ROPE.R0, ROPE.LEAD
FP8, U8 = torch.float8_e4m3fn, torch.uint8
SENT8 = 0x5A
SCALES = (1.0, 2.0 ** -3, 4.0)
TRUE_K_SCALE = 1.0 / 16
SHAPES = [(group, name) for group in (1, 4, 16) for name in ("A", "B")] + [(1, "C"), (4, "C")]
EXACT = ("quarter", "dyadic")


@pytest.fixture(scope="module")
def hip():
    from k8s_gpu_scheduler_amd import _native
    return _native.hip(required=True)


def lg():
    from k8s_gpu_scheduler_amd.ops import loadgen
    return loadgen


def scales_for(regime, hkv, i):
    """(k_scale, v_scale) lists for the i-th shape: powers of two, different per KV head where there are two."""
    if regime == "true":
        return [TRUE_K_SCALE] * hkv, [SCALES[i % 3]] * hkv
    if hkv == 1:
        return [SCALES[i % 3]], [SCALES[(i + 1) % 3]]
    return [SCALES[i % 3], SCALES[(i + 2) % 3]], [SCALES[(i + 1) % 3], SCALES[i % 3]]


def expected_caches8(nb, hkv, k_codes, v_codes, pos, seq, table):
    """uint8 k_cache [NB, Hkv, 32, 128] and v_cache [NB, Hkv, 128, 32]: SENT8 everywhere but the slots of the rows
    with pos >= 0, which hold k_codes / v_codes [Tq, Hkv, 128] of the row."""
    kc = torch.full((nb, hkv, T, D), SENT8, dtype=U8)
    vc = torch.full((nb, hkv, D, T), SENT8, dtype=U8)
    rows = (pos >= 0).nonzero().flatten()
    blk, slot = table[seq[rows], pos[rows] // T].long(), pos[rows] % T
    kc[blk, :, slot] = k_codes[rows]
    vc[blk, :, :, slot] = v_codes[rows]
    return kc, vc


class Case8(ROPE.Case):
    def __init__(self, regime, group, name, seed, k_scale, v_scale, plant=None):
        self.k_scale = torch.tensor(k_scale, dtype=torch.float32).cuda()
        self.v_scale = torch.tensor(v_scale, dtype=torch.float32).cuda()
        super().__init__(regime, group, name, seed, plant=plant)
        ks, vs = self.k_scale.cpu(), self.v_scale.cpu()
        self.ref_kb, self.ref_vb = lg().rope_append_kv8_reference(self.qkv_host, self.cs_host, self.ctx_host,
                                                                  self.q_start_host, ks, vs)
        self.exp_kc, self.exp_vc = expected_caches8(self.NB, self.hkv, self.ref_kb, self.ref_vb, self.pos, self.seq,
                                                    self.table_host)
        if regime == "true":
            z = self.ref_k / ks.double().view(1, self.hkv, 1)
            assert float(z.abs().max()) < 448 and not bool(((self.ref_kb & 0x7F) >= 0x7E).any()), "a K value saturates"
            xa = self.qkv_host[:, self.Hq:self.Hq + self.hkv].double().abs()
            x12 = xa[..., :HALF] + xa[..., HALF:]
            self.k_bound = (ks.double().view(1, self.hkv, 1) * torch.maximum(2.0 ** -4 * z.abs(), torch.tensor(2.0 ** -10, dtype=torch.float64))
                            + 2.0 ** -20 * torch.cat([x12, x12], dim=-1))                       # [Tq, Hkv, 128]
            self.bound = self.bound[:, :self.Hq]                                               # q_out keeps ROPE's bound

    def new_outputs(self):
        W = self.Hq * D
        raw, out2d = guarded_output(self.Tq, W, W + C0, C0, "cuda")
        kc = torch.full((self.NB, self.hkv, T, D), SENT8, dtype=U8, device="cuda").view(FP8)
        vc = torch.full((self.NB, self.hkv, D, T), SENT8, dtype=U8, device="cuda").view(FP8)
        return raw, out2d.unflatten(1, (self.Hq, D)), kc, vc

    @staticmethod
    def resentinel(outs):
        raw, _, kc, vc = outs
        raw.fill_(SENT16)
        kc.view(U8).fill_(SENT8)
        vc.view(U8).fill_(SENT8)

    def launch(self, outs, table=None, ctx=None, q_start=None, **kw):
        _, q_out, kc, vc = outs
        kw.setdefault("k_scale", self.k_scale)
        kw.setdefault("v_scale", self.v_scale)
        return lg().rope_append(self.qkv, self.cos_sin, kc, vc, self.table if table is None else table,
                                self.ctx if ctx is None else ctx, self.q_start if q_start is None else q_start,
                                q_out=q_out, **kw)

    def results(self, outs=None):
        raw, q_out, kc, vc = self.outs if outs is None else outs
        torch.cuda.synchronize()
        written = (slice(R0 + LEAD, R0 + LEAD + self.n), slice(C0, C0 + self.Hq * D))
        assert guards_intact(raw, written, SENT16), "write outside the chunks' rows of q_out"
        return q_out[LEAD:LEAD + self.n].cpu(), kc.view(U8).cpu(), vc.view(U8).cpu()

    def check(self, what, outs=None):
        got_q, got_kc, got_vc = self.results(outs)
        assert torch.equal(got_vc, self.exp_vc), (what, "v_cache", int((got_vc != self.exp_vc).sum()),
                                                  (got_vc != self.exp_vc).nonzero()[:1].tolist())
        if self.regime != "true":
            assert torch.equal(got_q, self.exp_q), (what, "q_out", int((got_q.float() != self.exp_q.float()).sum()))
            bad = got_kc != self.exp_kc
            assert not bool(bad.any()), (what, "k_cache", int(bad.sum()), bad.nonzero()[0].tolist(),
                                         int(got_kc[bad][0]), int(self.exp_kc[bad][0]))
            return
        rows = (self.pos >= 0).nonzero().flatten()
        blk, slot = self.table_host[self.seq[rows], self.pos[rows] // T].long(), self.pos[rows] % T
        rest = got_kc.clone()
        rest[blk, :, slot] = SENT8
        assert bool((rest == SENT8).all()), (what, "k_cache written outside the chunks' slots")
        deq = lg().dequantize_kv8_reference(got_kc[blk, :, slot], self.k_scale.cpu().view(1, self.hkv, 1))
        err_k = (deq - self.ref_k[rows]).abs()
        ratio_k = (err_k / self.k_bound[rows]).max().item() if self.n else 0.0
        err_q = (got_q.double() - self.ref_q).abs()
        ratio_q = (err_q / self.bound.clamp_min(1e-300)).max().item() if self.n else 0.0
        differ = int((got_kc[blk, :, slot] != self.ref_kb[rows]).sum())
        print(f"rope_append kv8, true regime {what}: K max |k_scale deq - y64| / bound = {ratio_k:.4f}, "
              f"{differ} of {err_k.numel()} K bytes differ from the reference bytes; q_out ratio {ratio_q:.4f}")
        assert bool((err_k <= self.k_bound[rows]).all()), (what, ratio_k)
        assert bool((err_q <= self.bound).all()), (what, ratio_q)

    def untouched(self, outs=None):
        raw, _, kc, vc = self.outs if outs is None else outs
        torch.cuda.synchronize()
        return (guards_intact(raw, (slice(0, 0), slice(0, 0)), SENT16) and bool((kc.view(U8) == SENT8).all())
                and bool((vc.view(U8) == SENT8).all()))


@functools.lru_cache(maxsize=None)
def case(regime, group, name):
    i = SHAPES.index((group, name))
    ks, vs = scales_for(regime, ROPE.SEQS[name][1], i)
    return Case8(regime, group, name, seed=9000 + 1000 * ROPE.REGIMES.index(regime) + 10 * group + "ABC".index(name),
                 k_scale=ks, v_scale=vs)


# ------------------------------------------------------------------------------------------------
# 1. the regimes
# ------------------------------------------------------------------------------------------------
def test_the_scale_sweep_covers_what_it_claims():
    for regime in EXACT:
        ks = [scales_for(regime, ROPE.SEQS[name][1], i) for i, (_, name) in enumerate(SHAPES)]
        assert {s for k, v in ks for s in k} == set(SCALES) == {s for k, v in ks for s in v}
        assert any(len(k) == 2 and k[0] != k[1] and v[0] != v[1] for k, v in ks)            # one launch, a scale per KV head
    assert {g for g, n in SHAPES if n in "AB"} == {1, 4, 16} and (1, "C") in SHAPES and (4, "C") in SHAPES


@pytest.mark.parametrize("group,name", SHAPES)
@pytest.mark.parametrize("regime", ROPE.REGIMES)
def test_regimes(hip, regime, group, name):
    c = case(regime, group, name)
    c.run()
    c.check((regime, group, name))


@pytest.mark.parametrize("v_scale", [1.0, 2.0 ** -3, 4.0, 0.75])
def test_v_exhaustive(v_scale):
    """One sequence of 512 tokens, one KV head: its V holds all 65,536 bf16 patterns."""
    g = torch.Generator().manual_seed(9100)
    qkv = torch.zeros(512, 3, D, dtype=torch.bfloat16)
    pats = torch.arange(65536, dtype=torch.int32)[torch.randperm(65536, generator=g)].to(torch.int16).view(512, D)
    qkv.view(torch.int16)[:, 2] = pats
    table = torch.randperm(16, generator=g).to(torch.int32).view(1, 16)
    ctx, q_start = torch.tensor([512], dtype=torch.int32), torch.tensor([0, 512], dtype=torch.int32)
    cs = lg().rope_table(512)
    ks, vs = torch.tensor([1.0]), torch.tensor([v_scale])
    _, ref_v = lg().rope_append_kv8_reference(qkv, cs, ctx, q_start, ks, vs)
    assert sorted(qkv.view(torch.int16)[:, 2].flatten().tolist()) == list(range(-32768, 32768))
    kc = torch.full((16, 1, T, D), SENT8, dtype=U8, device="cuda").view(FP8)
    vc = torch.full((16, 1, D, T), SENT8, dtype=U8, device="cuda").view(FP8)
    lg().rope_append(qkv.cuda(), cs.cuda(), kc, vc, table.cuda(), ctx.cuda(), q_start.cuda(), k_scale=ks.cuda(), v_scale=vs.cuda())
    torch.cuda.synchronize()
    got = vc.view(U8).cpu()[table[0].long(), 0].permute(0, 2, 1).reshape(512, D)       # [block, d, slot] -> [token, d]
    bad = got != ref_v[:, 0]
    assert not bool(bad.any()), (int(bad.sum()), [(hex(int(qkv.view(torch.int16)[r, 2, d]) & 0xFFFF), int(got[r, d]), int(ref_v[r, 0, d]))
                                                  for r, d in bad.nonzero()[:8].tolist()])
    assert bool(((kc.view(U8) & 0x7F) == 0).all())                                     # K of zeros: +-0 in every slot


# ------------------------------------------------------------------------------------------------
# 2. Inf and NaN in K
# ------------------------------------------------------------------------------------------------
def test_inf_and_nan_rule_in_k():
    """ROPE's plants (NaN and +-Inf in x1, x2, c and s cells) on the dyadic case: a NaN result is the byte 0x7F with either
    sign, +-Inf saturates to 0x7E / 0xFE, and no other byte differs from the unplanted twin's."""
    seed = 9000 + 1000 * ROPE.REGIMES.index("dyadic") + 41
    ks, vs = [1.0, 2.0 ** -3], [4.0, 1.0]
    dirty = Case8("dyadic", 4, "B", seed, ks, vs, plant=ROPE.plant_nonfinite)
    twin = Case8("dyadic", 4, "B", seed, ks, vs, plant=functools.partial(ROPE.plant_nonfinite, dirty=False))
    twin.run()
    twin.check("twin")
    dirty.run()
    _, dkc, dvc = dirty.results()
    assert torch.equal(dvc, dirty.exp_vc)
    ref = dirty.exp_kc
    nan = (ref & 0x7F) == 0x7F
    assert torch.equal((dkc & 0x7F) == 0x7F, nan) and torch.equal(dkc[~nan], ref[~nan])
    rows = (dirty.pos >= 0).nonzero().flatten()
    ref_k = dirty.ref_k[rows]
    blk, slot = dirty.table_host[dirty.seq[rows], dirty.pos[rows] // T].long(), dirty.pos[rows] % T
    got = dkc[blk, :, slot]
    assert bool(ref_k.isnan().any()) and bool(ref_k.isinf().any())
    assert bool(((got & 0x7F) == 0x7F)[ref_k.isnan()].all())
    assert torch.equal(got[ref_k == float("inf")], torch.full_like(got[ref_k == float("inf")], 0x7E))
    assert torch.equal(got[ref_k == -float("inf")], torch.full_like(got[ref_k == -float("inf")], 0xFE))
    changed = dkc != twin.exp_kc
    hit = torch.zeros(got.shape, dtype=torch.bool)
    for r, heads, i in dirty.planted:
        for h in heads:
            if h >= dirty.Hq:
                hit[r, h - dirty.Hq, i] = hit[r, h - dirty.Hq, i + HALF] = True
    assert not bool(changed[blk, :, slot][~hit].any()), "a non-finite value reached another K element"


# ------------------------------------------------------------------------------------------------
# 3. chunked == whole; other launch paths
# ------------------------------------------------------------------------------------------------
def test_chunked_append_equals_whole():
    group, hkv = 2, 2
    Ht = group * hkv + 2 * hkv
    seqs = ROPE.SEQS_B
    g = torch.Generator().manual_seed(9902)
    ctxs = [c for c, _ in seqs]
    table, nb = PRE.block_tables(tuple(ctxs), g)
    full = torch.randn(sum(ctxs), Ht, D, generator=g).to(torch.bfloat16).cuda()
    cs = lg().rope_table(257).cuda()
    table, ctx = table.cuda(), torch.tensor(ctxs, dtype=torch.int32).cuda()
    sc = dict(k_scale=torch.tensor([0.0625, 0.1]).cuda(), v_scale=torch.tensor([0.05, 0.03]).cuda())
    starts = [0] + torch.tensor(ctxs).cumsum(0).tolist()
    csr = lambda lens: torch.tensor([0] + lens).cumsum(0).to(torch.int32).cuda()          # noqa: E731

    def caches():
        return (torch.full((nb, hkv, T, D), SENT8, dtype=U8, device="cuda").view(FP8),
                torch.full((nb, hkv, D, T), SENT8, dtype=U8, device="cuda").view(FP8))
    kc1, vc1 = caches()
    q1 = lg().rope_append(full, cs, kc1, vc1, table, ctx, csr(ctxs), **sc)
    kc2, vc2 = caches()
    pre = [c - n for c, n in seqs]
    pre_rows = torch.cat([torch.arange(starts[s], starts[s] + pre[s]) for s in range(len(seqs))]).cuda()
    new_rows = torch.cat([torch.arange(starts[s] + pre[s], starts[s + 1]) for s in range(len(seqs))]).cuda()
    qa = lg().rope_append(full[pre_rows], cs, kc2, vc2, table, torch.tensor(pre, dtype=torch.int32).cuda(), csr(pre), **sc)
    qb = lg().rope_append(full[new_rows], cs, kc2, vc2, table, ctx, csr([n for _, n in seqs]), **sc)
    torch.cuda.synchronize()
    assert torch.equal(kc1.view(U8), kc2.view(U8)) and torch.equal(vc1.view(U8), vc2.view(U8))
    assert torch.equal(ROPE.bits(q1[pre_rows]), ROPE.bits(qa)) and torch.equal(ROPE.bits(q1[new_rows]), ROPE.bits(qb))
    assert len(kc1.view(U8).unique()) > 100 and len(vc1.view(U8).unique()) > 100 and bool((kc1.view(U8) == SENT8).any())


def test_no_check_and_a_larger_max_q_len_give_the_same():
    c = case("quarter", 4, "B")
    for kw in (dict(check=False, max_q_len=c.max_q_len), dict(check=False, max_q_len=c.max_q_len + 100),
               dict(max_q_len=c.max_q_len + 1000)):
        c.run(**kw)
        c.check(kw)


@pytest.mark.parametrize("breakage", ["block-NB", "duplicate-block", "q_len-above-ctx", "k_scale-zero", "v_scale-negative",
                                      "k_scale-nan", "v_scale-nan", "k_scale-inf"])
def test_check_raises_and_launches_nothing(breakage):
    c = case("quarter", 4, "A")
    s = [x[0] for x in c.seqs].index(256)                   # (256, 1): touches entry 7 only
    table, ctx, kw = c.table.clone(), c.ctx.clone(), {}
    if breakage == "block-NB":
        table[s, 7] = c.NB
    elif breakage == "duplicate-block":
        table[s, 7] = c.table[c.seqs.index((33, 33)), 1]
    elif breakage == "q_len-above-ctx":
        ctx[c.seqs.index((33, 33))] = 32
    else:
        name, value = breakage.split("-")
        kw[name] = torch.tensor([{"zero": 0.0, "negative": -2.0, "nan": float("nan"), "inf": float("inf")}[value]]).cuda()
    c.resentinel(c.outs)
    with pytest.raises(ValueError):
        c.launch(c.outs, table=table, ctx=ctx, **kw)
    assert c.untouched()


def test_wrapper_raises_on_the_device_too():
    c = case("quarter", 4, "A")
    _, q_out, kc, vc = c.outs
    c.resentinel(c.outs)
    with pytest.raises(ValueError, match="need k_scale and v_scale"):
        lg().rope_append(c.qkv, c.cos_sin, kc, vc, c.table, c.ctx, c.q_start, q_out=q_out)
    with pytest.raises(TypeError, match="one cache dtype"):
        c.launch((None, q_out, kc, torch.zeros(vc.shape, dtype=torch.bfloat16, device="cuda")))
    b = ROPE.case("quarter", 4, "A")
    with pytest.raises(ValueError, match="scale"):
        b.launch(b.outs, k_scale=c.k_scale, v_scale=c.v_scale)
    assert c.untouched()


def test_side_stream_and_graph_replay():
    c = case("dyadic", 16, "A")
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


# ------------------------------------------------------------------------------------------------
# 4. beside a co-running load
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aggressor,mode", [pytest.param(a, m, id=f"{a}-{m}") for a, m in CO.BASE_PAIRS])
def test_rope_append_kv8_corun(hip, aggressor, mode):
    c = case("dyadic", 4, "B")
    victim = CO.Load("rope-append-kv8-dyadic", {}, [ROPE.AppendLaunch(c, ("dyadic", 4, "B", r)) for r in range(CO.R)])
    try:
        CO.corun(hip, victim, CO.aggressor_for(aggressor, mode), mode)
    finally:
        CO.restore_knobs(hip)
