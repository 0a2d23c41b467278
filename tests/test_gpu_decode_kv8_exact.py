"""Exact-arithmetic, guarded-buffer tests of the paged-KV decode attention over an FP8 cache
(loadgen.paged_decode_attention_kv8, unsplit and split; run with `-m gpu` on an MI355X).
The guards, context lists, block tables, shapes, regimes and the float64 reference are those of
test_gpu_decode_attn_exact.py (ATT) and, for kv_splits >= 2, of test_gpu_decode_split_exact.py (SPL), whose
placement of the targets by the partition rule is used; neither module is changed.

THE FORMAT (native/hip/api.h): a stored byte c of KV head g stands for e4m3fn(c) * scale[g].  The reference is
ATT.reference on loadgen.dequantize_kv8_reference of the byte caches with the scales applied per head -- float64
logical K and V -- so scale * k_scale and * v_scale are in it by construction.  e4m3fn -> bf16 is exact, the
kernels keep the bf16 MFMAs and the fp32 softmax, and with power-of-two scales the exact regimes of the bf16
modules stay exact; the comparison is `torch.equal` after float64 -> fp32 -> bf16:

  onehot   q = 8 H[r]; the stored K rows are +-16 (K_SCALE = 2^-2, so the logical K is the bf16 module's 4 H; with
           per-head scales (2^-2, 2^-3) the second head stores +-32): target score 362, all others 0, p = 1 and 0.
           V is drawn from the finite e4m3fn codes of six binades (magnitude codes 0x18 .. 0x47: 2^-4 .. 3.75).
  pair     two targets per head, p = 0.5 each: out = bf16(v_scale (v1 + v2) / 2).  Two 4-bit significands up to five
           binades apart need up to 9 bits: that some output is NOT a bf16 value before the rounding is asserted on
           the reference alone.
  uniform  q = 0, K random finite codes, V an integer in [-4, 4], ctx a power of two.

Unnamed blocks and the slots past ctx hold the NaN byte 0x7F in both caches.  Every exact regime runs over ATT.SHAPES
with the scales of scales_for (v_scale cycling through 1, 2^-3, 4; per-head differing k_scale and v_scale at
Hkv = 2), and at (4, 1) with each v_scale.

The random regime: K bytes are random finite codes of magnitude <= 2, V codes of magnitude <= 1, k_scale = 0.37,
v_scale = 1.9, q randn; |out - ref| <= 2^-7 * v_scale * max|e4m3(V)| -- ATT's derivation unchanged, because
dequantisation is exact and the two scales are single fp32 multiplies (2^-24 relative each).
"""
import functools

import pytest
import torch

import test_gpu_corun_exact as CO
import test_gpu_decode_attn_exact as ATT
import test_gpu_decode_split_exact as SPL
from test_gpu_kernels_exact import NAN, SENT16, SENT32, guarded_input, guarded_output, guarded_vector, guards_intact, out_window

pytestmark = pytest.mark.gpu

# MEASURED on an MI355X (printed by the tests):
MEASURED = """
  random regime, max|out - ref| over the shapes: 0.00313 .. 0.00503 unsplit and at every split count (bound 0.01484 =
  2^-7 * 1.9 * 1).  Co-run (4 + 4 launches per victim): the victim's slowdown 0.31 .. 0.48; every output bit-exact.
  The large-address case (two 4 GiB caches from torch.empty): 0.4 s.  The module: 142 tests in 4.6 s.
"""

D, T, C0 = ATT.D, ATT.T, ATT.C0
FP8, U8 = torch.float8_e4m3fn, torch.uint8
NAN8 = 0x7F
K_SCALE = 2.0 ** -2
V_SCALES = (1.0, 2.0 ** -3, 4.0)
RANDOM_K_SCALE, RANDOM_V_SCALE = 0.37, 1.9
EXACT = ("onehot", "pair", "uniform")
KV_SPLITS = (2, 3, 8, 32)
SPLIT_SHAPES = ((1, 2), (4, 1), (8, 2), (16, 1))


@pytest.fixture(scope="module")
def hip():
    from k8s_gpu_scheduler_amd import _native
    return _native.hip(required=True)


def lg():
    from k8s_gpu_scheduler_amd.ops import loadgen
    return loadgen


def scales_for(regime, hkv, i):
    """(k_scale, v_scale) lists of length hkv for the i-th shape of a sweep."""
    if regime == "random":
        return [RANDOM_K_SCALE] * hkv, [RANDOM_V_SCALE] * hkv
    if hkv == 1:
        return [K_SCALE], [V_SCALES[i % 3]]
    return [K_SCALE, K_SCALE / 2], [V_SCALES[i % 3], V_SCALES[(i + 1) % 3]]


def codes(shape, lo, hi, g):
    """Random e4m3fn values (fp32) whose magnitude codes lie in [lo, hi), any sign."""
    c = torch.randint(lo, hi, shape, generator=g) | (torch.randint(0, 2, shape, generator=g) << 7)
    return c.to(U8).view(FP8).float()


def to_bytes(x_bf16):
    """bf16 cache of e4m3fn values (NaN elsewhere) -> uint8 codes, NaN -> 0x7F, checked to be lossless."""
    b = lg().quantize_kv8_reference(x_bf16.float())
    back = lg().dequantize_kv8_reference(b, 1.0)
    assert torch.equal(back.nan_to_num(7.0), x_bf16.double().nan_to_num(7.0)), "a cache value is no e4m3fn value"
    b[x_bf16.float().isnan()] = NAN8                                             # the sign of the NaN filler is not kept
    return b


class Case:
    """One launch's operands, guarded, with the float64 reference.  kv_splits > 0 places the targets of the onehot
    and pair regimes by SPL's rule."""

    def __init__(self, regime, group, hkv, ctxs, k_scale, v_scale, seed, kv_splits=0):
        g = torch.Generator().manual_seed(seed)
        self.regime, self.S, self.Hq, self.hkv, self.ctxs, self.group = regime, len(ctxs), group * hkv, hkv, ctxs, group
        table, nb = ATT.block_tables(ctxs, g)
        self.targets = None
        if regime in ("onehot", "pair") and kv_splits:
            q, ks, _, self.targets = SPL.placed_operands(regime, group, hkv, ctxs, kv_splits, g)
        elif regime in ("onehot", "pair"):
            q, ks, _ = ATT.logical_operands(regime, group, hkv, ctxs, g)
        elif regime == "uniform":
            q, ks = torch.zeros(self.S, self.Hq, D), None
        else:
            q, ks = torch.randn(self.S, self.Hq, D, generator=g).to(torch.bfloat16).float(), None
        ksc, vsc = torch.tensor(k_scale, dtype=torch.float32), torch.tensor(v_scale, dtype=torch.float32)
        if ks is not None:                      # logical +-4 -> stored +-4 / k_scale[g]
            ks = [k / ksc.view(hkv, 1, 1) for k in ks]
            assert all(bool((k.abs() * ksc.view(hkv, 1, 1) == 4).all()) for k in ks)
            if k_scale[0] == K_SCALE:
                assert all(bool((k[0].abs() == 16).all()) for k in ks)
        else:
            ks = [codes((hkv, c, D), 0, 0x41, g) for c in ctxs]                  # |value| <= 2
        if regime == "uniform":
            vs = [torch.randint(-4, 5, (hkv, c, D), generator=g).float() for c in ctxs]
        elif regime == "random":
            vs = [codes((hkv, c, D), 0, 0x39, g) for c in ctxs]                  # |value| <= 1
        else:
            vs = [codes((hkv, c, D), 0x18, 0x48, g) for c in ctxs]               # six binades
        kb, vb = ATT.paged_caches(ks, vs, table, nb, hkv)                        # bf16, NaN wherever no token lives
        self.k_bytes, self.v_bytes = to_bytes(kb), to_bytes(vb)
        ctx = torch.tensor(ctxs, dtype=torch.int32)
        qb = q.to(torch.bfloat16)
        assert torch.equal(qb.float(), q)
        kd = lg().dequantize_kv8_reference(self.k_bytes, ksc.view(1, hkv, 1, 1))
        vd = lg().dequantize_kv8_reference(self.v_bytes, vsc.view(1, hkv, 1, 1))
        self.ref = ATT.reference(qb, kd, vd, table, ctx)
        self.vmax = max([float((v.abs() * vsc.view(hkv, 1, 1)).max()) for v in vs if v.numel()] + [0.0])
        self.NB, self.max_blocks, self.host_table = nb, table.shape[1], table
        W = self.Hq * D
        self.q = guarded_input(qb.view(self.S, W).cuda(), W + C0, c0=C0).unflatten(1, (self.Hq, D))
        self.kc, self.vc = self.k_bytes.cuda().view(FP8), self.v_bytes.cuda().view(FP8)
        self.k_scale, self.v_scale = ksc.cuda(), vsc.cuda()
        self.table_raw, self.table = ATT.guarded_ints_2d(table, self.max_blocks + 2)
        self.ctx_raw = torch.full((1 + self.S + 3,), SENT32, dtype=torch.int32, device="cuda")
        self.ctx = self.ctx_raw[1:1 + self.S]
        self.ctx.copy_(ctx)
        self.raw, self.out = self.new_output()
        self.ws_raw = {}
        if regime != "random":
            f = self.ref.float()
            big = self.ref.abs() > 2.0 ** -20          # (an exact 0 carries the other tokens' exp(-362) weights)
            assert torch.equal(f.double()[big], self.ref[big])                   # exact in fp32
            if regime == "pair":
                assert bool((f.to(torch.bfloat16).double() != f.double())[big].any()), "every output is a bf16 value"
            self.exp = f.to(torch.bfloat16).cuda()

    def new_output(self):
        W = self.Hq * D
        raw, out2d = guarded_output(self.S, W, W + C0, C0, "cuda")
        return raw, out2d.unflatten(1, (self.Hq, D))

    def workspace(self, kv_splits):
        n = lg().decode_split_workspace_floats(self.S, self.Hq, max(kv_splits, 2))
        if kv_splits not in self.ws_raw:
            self.ws_raw[kv_splits] = guarded_vector(n, SPL.WS_BEFORE, SPL.WS_AFTER, "cuda")
        ws = self.ws_raw[kv_splits][1]
        ws.fill_(NAN)
        return ws

    def resentinel(self):
        self.raw.fill_(SENT16)

    def run(self, kv_splits=1, out=None, **kw):
        args = dict(q=self.q, kc=self.kc, vc=self.vc, table=self.table, ctx=self.ctx, k_scale=self.k_scale,
                    v_scale=self.v_scale)
        args.update({k: kw.pop(k) for k in list(kw) if k in args})
        if kv_splits > 1 and "workspace" not in kw:
            kw["workspace"] = self.workspace(kv_splits)
        elif kw.get("workspace", 0) is None:                                      # workspace=None: let the wrapper allocate
            del kw["workspace"]
        return lg().paged_decode_attention_kv8(args["q"], args["kc"], args["vc"], args["table"], args["ctx"],
                                           out=self.out if out is None else out, kv_splits=kv_splits,
                                           k_scale=args["k_scale"], v_scale=args["v_scale"], **kw)

    def guards(self, what, raw=None, ws=None):
        torch.cuda.synchronize()
        assert guards_intact(self.raw if raw is None else raw, out_window(self.S, self.Hq * D, C0), SENT16), ("write outside out", what)
        for wraw, w in ([ws] if ws is not None else self.ws_raw.values()):
            assert guards_intact(wraw, slice(SPL.WS_BEFORE, SPL.WS_BEFORE + w.numel()), SENT32), ("write outside the workspace", what)

    def check(self, what, raw=None, out=None, ws=None):
        self.guards(what, raw, ws)
        out = self.out if out is None else out
        if self.regime == "random":
            err = (out.double().cpu() - self.ref).abs().max().item()
            print(f"kv8 decode attention, random regime {what}: max|out - ref| = {err:.5f} "
                  f"(bound {ATT.RANDOM_BOUND * self.vmax:.5f}, v_scale * max|V| = {self.vmax:.4f})")
            assert err <= ATT.RANDOM_BOUND * self.vmax, (what, err)
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
def _case(regime, group, hkv, ctxs, k_scale, v_scale, kv_splits):
    return Case(regime, group, hkv, ctxs, list(k_scale), list(v_scale),
                seed=8000 + 1000 * ATT.REGIMES.index(regime) + 10 * group + hkv + 100 * kv_splits, kv_splits=kv_splits)


def case(regime, group, hkv, i=0, kv_splits=0, ctxs=None, v_scale=None):
    """Unsplit (kv_splits == 0: ATT's context lists and targets) or placed for kv_splits (SPL's)."""
    if ctxs is None:
        mod = SPL if kv_splits else ATT
        ctxs = mod.CTX_UNIFORM if regime == "uniform" else (mod.CTX_A if hkv == 1 else mod.CTX_B)
    ks, vs = scales_for(regime, hkv, i)
    if v_scale is not None:
        vs = [v_scale] * hkv
    return _case(regime, group, hkv, ctxs, tuple(ks), tuple(vs), kv_splits if regime in ("onehot", "pair") else 0)


# ------------------------------------------------------------------------------------------------
# 1. the regimes, unsplit
# ------------------------------------------------------------------------------------------------
def test_the_scale_sweep_covers_what_it_claims():
    seen = {(regime, tuple(scales_for(regime, hkv, i)[1])) for regime in EXACT for i, (_, hkv) in enumerate(ATT.SHAPES)}
    for regime in EXACT:
        assert {v for r, vs in seen if r == regime for v in vs} == set(V_SCALES)
        assert any(len(vs) == 2 and vs[0] != vs[1] for r, vs in seen if r == regime)
    ks, _ = scales_for("onehot", 2, 0)
    assert ks[0] != ks[1] and ks[0] == K_SCALE == 0.25


@pytest.mark.parametrize("i,group,hkv", [(i, g, h) for i, (g, h) in enumerate(ATT.SHAPES)])
@pytest.mark.parametrize("regime", ATT.REGIMES)
def test_regimes(hip, regime, i, group, hkv):
    c = case(regime, group, hkv, i)
    c.resentinel()
    c.run()
    c.check((regime, group, hkv))


@pytest.mark.parametrize("v_scale", V_SCALES)
@pytest.mark.parametrize("regime", EXACT)
def test_each_exact_regime_with_each_v_scale(regime, v_scale):
    c = case(regime, 4, 1, v_scale=v_scale)
    c.resentinel()
    c.run()
    c.check((regime, "v_scale", v_scale))


@pytest.mark.parametrize("v_scale", [1.0, 2.0 ** -3])
def test_all_256_codes_decode(v_scale):
    """ctx = 1, q = 0: p = 1 and out[s, 0, d] = bf16(v_scale * e4m3(V[s, d])); two sequences hold the 256 codes."""
    from test_kv8_cpu import e4m3
    table = torch.tensor([[1], [0]], dtype=torch.int32).cuda()
    ctx = torch.ones(2, dtype=torch.int32).cuda()
    kc = torch.full((2, 1, T, D), NAN8, dtype=U8)
    vc = torch.full((2, 1, D, T), NAN8, dtype=U8)
    kc[:, :, 0] = 0x38
    vc[1, 0, :, 0] = torch.arange(128, dtype=U8)                                  # sequence 0 reads block 1
    vc[0, 0, :, 0] = torch.arange(128, 256, dtype=torch.int32).to(U8)
    q = torch.zeros(2, 1, D, dtype=torch.bfloat16).cuda()
    sc = torch.tensor([v_scale]).cuda()
    for splits in (1, 2):
        out = lg().paged_decode_attention_kv8(q, kc.cuda().view(FP8), vc.cuda().view(FP8), table, ctx, k_scale=sc, v_scale=sc,
                                          kv_splits=splits).float().cpu().flatten()
        want = torch.tensor([e4m3(c) * v_scale for c in range(256)], dtype=torch.float64)
        assert bool(out[0x7F].isnan()) and bool(out[0xFF].isnan()) and int(out.isnan().sum()) == 2
        fin = ~want.isnan()
        assert torch.equal(out.double()[fin], want[fin]), (splits, (out.double()[fin] != want[fin]).nonzero().flatten().tolist())


def test_no_check_gives_the_same():
    c = case("pair", 4, 2, 1)
    c.resentinel()
    c.run(check=False)
    c.check("check=False")


# ------------------------------------------------------------------------------------------------
# 2. split-KV
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kv_splits", KV_SPLITS)
@pytest.mark.parametrize("i,group,hkv", [(i, g, h) for i, (g, h) in enumerate(SPLIT_SHAPES)])
@pytest.mark.parametrize("regime", ATT.REGIMES)
def test_split_regimes(hip, regime, i, group, hkv, kv_splits):
    c = case(regime, group, hkv, i, kv_splits)
    c.resentinel()
    c.run(kv_splits)
    c.check((regime, group, hkv, kv_splits))


@pytest.mark.parametrize("regime", ["onehot", "pair"])
def test_more_splits_than_blocks(regime):
    """Empty splits: no sequence of CTX_SHORT has more than 4 blocks."""
    for kv_splits in (8, 32):
        c = case(regime, 4, 1, 1, kv_splits, SPL.CTX_SHORT)
        c.resentinel()
        c.run(kv_splits)
        c.check(("short", regime, kv_splits))


def test_workspace_is_allocated_when_none_is_given():
    c = case("onehot", 8, 2, 2, 3)
    c.resentinel()
    c.run(3, workspace=None)
    c.check("workspace=None")


# ------------------------------------------------------------------------------------------------
# 3. NaN bytes inside and past ctx
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kv_splits", [1, 4])
def test_nan_inside_ctx_propagates_and_past_ctx_does_not(kv_splits):
    c = case("onehot", 4, 2, 0, 4)
    c.resentinel()
    c.run(kv_splits)
    c.check(("base", kv_splits))                       # the slots past ctx and the unnamed blocks are 0x7F already
    base = c.out.clone()
    s = c.ctxs.index(max(c.ctxs))
    ctx, kv, d = c.ctxs[s], 1, 41
    tgs = [t for head in c.targets[s][kv] for t in head]
    t = next(u for u in range(ctx - 2, -1, -1) if u not in tgs)
    vc = c.vc.clone()
    vc.view(U8)[int(c.host_table[s, t // T]), kv, d, t % T] = NAN8             # probability 0, but 0 * NaN is NaN
    c.resentinel()
    c.run(kv_splits, vc=vc)
    c.guards("NaN in V")
    mask = torch.zeros_like(base, dtype=torch.bool)
    mask[s, kv * 4:(kv + 1) * 4, d] = True
    assert bool(c.out[mask].isnan().all()) and torch.equal(c.out.view(torch.int16)[~mask], base.view(torch.int16)[~mask])
    kc = c.kc.clone()
    kc.view(U8)[int(c.host_table[s, t // T]), kv, t % T, 5] = NAN8 | 0x80       # a NaN score: the group's rows are NaN
    c.resentinel()
    c.run(kv_splits, kc=kc)
    c.guards("NaN in K")
    mask = torch.zeros_like(base, dtype=torch.bool)
    mask[s, kv * 4:(kv + 1) * 4] = True
    assert bool(c.out[mask].isnan().all()) and torch.equal(c.out.view(torch.int16)[~mask], base.view(torch.int16)[~mask])


# ------------------------------------------------------------------------------------------------
# 4. check=True; side stream and graph replay
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kv_splits", [1, 4])
@pytest.mark.parametrize("breakage", ["block-NB", "ctx-negative", "k_scale-zero", "v_scale-negative", "k_scale-nan", "v_scale-inf"])
def test_check_raises_and_launches_nothing(breakage, kv_splits):
    c = case("onehot", 4, 1, 0)
    s = c.ctxs.index(257)
    kw = {}
    if breakage == "block-NB":
        kw["table"] = c.table.clone()
        kw["table"][s, 8] = c.NB
    elif breakage == "ctx-negative":
        kw["ctx"] = c.ctx.clone()
        kw["ctx"][c.ctxs.index(1)] = -1
    else:
        name, value = breakage.split("-")
        kw[name] = torch.tensor([{"zero": 0.0, "negative": -1.0, "nan": NAN, "inf": float("inf")}[value]]).cuda()
    c.resentinel()
    with pytest.raises(ValueError):
        c.run(kv_splits, **kw)
    assert c.untouched()
    if kv_splits > 1:
        torch.cuda.synchronize()
        assert bool(c.ws_raw[kv_splits][1].isnan().all())


def test_wrapper_raises_on_the_device_too():
    c = case("onehot", 4, 1, 0)
    with pytest.raises(ValueError, match="need k_scale and v_scale"):
        lg().paged_decode_attention_kv8(c.q, c.kc, c.vc, c.table, c.ctx, out=c.out)
    with pytest.raises(TypeError, match="bf16"):
        lg().paged_decode_attention(c.q, c.kc, c.vc, c.table, c.ctx, out=c.out)
    with pytest.raises(TypeError, match="one cache dtype"):
        lg().paged_decode_attention_kv8(c.q, c.kc, torch.zeros(c.vc.shape, dtype=torch.bfloat16, device="cuda"), c.table, c.ctx,
                                    out=c.out, k_scale=c.k_scale, v_scale=c.v_scale)
    with pytest.raises(ValueError, match="device"):
        lg().paged_decode_attention_kv8(c.q, c.kc, c.vc, c.table, c.ctx, out=c.out, k_scale=c.k_scale.cpu(), v_scale=c.v_scale)
    with pytest.raises(TypeError, match="bf16"):
        lg().paged_prefill_attention(c.q, c.kc, c.vc, c.table, c.ctx, torch.arange(c.S + 1, dtype=torch.int32).cuda())
    c.resentinel()
    assert c.untouched()


@pytest.mark.parametrize("kv_splits", [1, 4])
def test_side_stream_and_graph_replay(kv_splits):
    c = case("pair", 8, 2, 1, 4)
    s = torch.cuda.Stream()
    c.resentinel()
    ws = c.workspace(4)
    torch.cuda.synchronize()
    c.run(kv_splits, stream=s, workspace=ws)
    s.synchronize()
    c.check("side stream")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        c.run(kv_splits, stream=s, check=False, workspace=ws)
    for k in range(2):
        c.resentinel()
        ws.fill_(NAN)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        s.synchronize()
        c.check(("replay", k))


# ------------------------------------------------------------------------------------------------
# 5. beside a co-running load
# ------------------------------------------------------------------------------------------------
class Launch:
    """One launch (pair) on a Case's inputs into an output and a workspace of its own."""

    def __init__(self, c, kv_splits, what):
        self.case, self.kv_splits, self.what = c, kv_splits, what
        self.raw, self.out = c.new_output()
        self.ws = guarded_vector(lg().decode_split_workspace_floats(c.S, c.Hq, max(kv_splits, 2)), SPL.WS_BEFORE,
                                 SPL.WS_AFTER, "cuda")

    def reset(self):
        self.raw.fill_(SENT16)
        self.ws[1].fill_(NAN)

    def enqueue(self, st):
        self.case.run(self.kv_splits, out=self.out, workspace=self.ws[1], stream=st, check=False)

    def check(self, tag):
        self.case.check((tag, self.what), self.raw, self.out, self.ws)


@pytest.mark.parametrize("aggressor,mode", [pytest.param(a, m, id=f"{a}-{m}") for a, m in CO.BASE_PAIRS])
def test_decode_kv8_corun(hip, aggressor, mode):
    launches = [Launch(case("pair", 4, 2, 1), 1, ("pair", 4, 2, r)) for r in range(CO.R)]
    launches += [Launch(case("pair", 4, 1, 0, 4), 4, ("pair", 4, 1, "4 splits", r)) for r in range(CO.R)]
    victim = CO.Load("decode-kv8", {}, launches)
    try:
        CO.corun(hip, victim, CO.aggressor_for(aggressor, mode), mode)
    finally:
        CO.restore_knobs(hip)


# ------------------------------------------------------------------------------------------------
# 6. addresses past 4 GiB: decode, split decode and the append on one allocation
# ------------------------------------------------------------------------------------------------
BIG_HKV, BIG_GROUP = 2, 4
BLOCK_BYTES = BIG_HKV * T * D                # a block of one FP8 cache: 8 KiB
HIGH = (1 << 32) // BLOCK_BYTES              # 524288: the first block id at byte offset 2^32
LOW_IDS = 32                                 # compact ids below it stay; c >= 32 becomes HIGH + c
BIG_NB = HIGH + 64
SENT8 = 0x5A


def physical(ids):
    return torch.where((ids == SENT32) | (ids < LOW_IDS), ids, ids + HIGH)


def test_large_addresses_decode_and_append():
    """FP8 caches of 4 GiB + 512 KiB from torch.empty; only the named blocks (and the decoys) are written.  Compact
    ids >= 32 become physical ids >= HIGH + 32: byte offset > 2^32.  A 32-bit byte offset would send such a block to
    physical block c in [32, 64), which no table entry names: the readers find finite decoys there (a wrong value,
    not a fault), the writer leaves them SENT8."""
    assert HIGH * BLOCK_BYTES == 1 << 32 and (HIGH + LOW_IDS) * BLOCK_BYTES > 1 << 32
    ctxs = (257, 33, 64, 290, 129, 65, 97, 200)
    c = Case("pair", BIG_GROUP, BIG_HKV, ctxs, [K_SCALE, K_SCALE / 2], [4.0, 2.0 ** -3], seed=8990)
    # re-deal the table over compact ids so that consecutive entries alternate between the two ends
    table = c.host_table.clone()
    g = torch.Generator().manual_seed(8991)
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
    phys = physical(table)
    assert int(phys[phys != SENT32].max()) * BLOCK_BYTES > 1 << 32
    src = torch.tensor(sorted(remap), dtype=torch.int64)
    dst = physical(torch.tensor([remap[int(b)] for b in src], dtype=torch.int64)).cuda()
    kc = torch.empty((BIG_NB, BIG_HKV, T, D), dtype=U8, device="cuda")
    vc = torch.empty((BIG_NB, BIG_HKV, D, T), dtype=U8, device="cuda")
    assert kc.numel() > 1 << 32
    kc[LOW_IDS:64] = 0x30                                                         # decoys: 0.5 everywhere
    vc[LOW_IDS:64] = 0x30
    kc[:LOW_IDS] = NAN8
    vc[:LOW_IDS] = NAN8
    kc[HIGH + LOW_IDS:] = NAN8
    vc[HIGH + LOW_IDS:] = NAN8
    kc[dst] = c.k_bytes[src].cuda()
    vc[dst] = c.v_bytes[src].cuda()
    _, tview = ATT.guarded_ints_2d(phys.to(torch.int32), c.max_blocks + 2)
    for splits in (1, 4):
        c.resentinel()
        c.run(splits, kc=kc.view(FP8), vc=vc.view(FP8), table=tview)
        c.check(("large addresses", splits))
    del c
    # the append: whole sequences (q_len == ctx) into SENT8-filled caches
    import test_gpu_rope_append_kv8_exact as RA
    seqs = tuple((x, x) for x in ctxs)
    a = RA.Case8("quarter", BIG_GROUP, (seqs, BIG_HKV), seed=8992, k_scale=[1.0, 4.0], v_scale=[2.0 ** -3, 1.0])
    # the append case dealt its own compact ids: deal them anew by the same rule
    low, high = torch.randperm(LOW_IDS, generator=g).tolist(), (LOW_IDS + torch.randperm(LOW_IDS, generator=g)).tolist()
    amap = {}
    table = a.table_host.clone()
    for s in range(table.shape[0]):
        for j in range(-(-ctxs[s] // T)):
            amap[int(a.table_host[s, j])] = (low if (j // 4 + j + s) % 2 == 0 else high).pop()
            table[s, j] = amap[int(a.table_host[s, j])]
    phys = physical(table)
    kc.fill_(SENT8)
    vc.fill_(SENT8)
    _, tview = ATT.guarded_ints_2d(phys.to(torch.int32), a.max_blocks + 2)
    raw, q_out, _, _ = a.outs
    lg().rope_append(a.qkv, a.cos_sin, kc.view(FP8), vc.view(FP8), tview, a.ctx, a.q_start, q_out=q_out,
                     k_scale=a.k_scale, v_scale=a.v_scale)
    torch.cuda.synchronize()
    src = torch.tensor(sorted(amap), dtype=torch.int64)
    dst = physical(torch.tensor([amap[int(b)] for b in src], dtype=torch.int64)).cuda()
    assert torch.equal(kc[dst].cpu(), a.exp_kc[src]) and torch.equal(vc[dst].cpu(), a.exp_vc[src])
    assert torch.equal(q_out[RA.LEAD:RA.LEAD + a.n].cpu(), a.exp_q)
    want = int((a.exp_kc != SENT8).sum()), int((a.exp_vc != SENT8).sum())
    piece = 1 << 30
    got = [sum(int((x.flatten()[o:o + piece] != SENT8).sum()) for o in range(0, x.numel(), piece)) for x in (kc, vc)]
    assert tuple(got) == want, (got, want)                                        # nothing else was written, decoys included
    del kc, vc
    torch.cuda.empty_cache()
