"""Non-finite values, bf16 edges and the softmax scale through the two paged-KV attentions (run with
`-m gpu` on an MI355X): what the module docstring of k8s_gpu_scheduler_amd/ops/loadgen.py says of
them -- the NaN rule, "no zero is skipped", subnormals kept, one IEEE division, one bf16 rounding --
checked on the values that test_gpu_decode_attn_exact.py and test_gpu_prefill_attn_exact.py leave
out.  Their block-table, cache and guard builders are used, and the bit-pattern helpers of
test_gpu_numeric_edges.py.

The expectation never comes from a float64 softmax (which gives a token 362 below the maximum the
weight 6e-158 where the kernels' fp32 exp gives exactly 0, and so Inf where 0 * Inf = NaN is due).
One explicit reference serves every part:

    ref[q, h, d] = (sum_t P[q, h, t] * V[t, d]) / (sum_t P[q, h, t])

with P the contract's probabilities (`contract_probabilities`: 1 on the tokens whose score is the
row's maximum, 0 on those far enough below it for the fp32 exp to underflow and above the causal
limit, NaN where the score is NaN or +Inf -- Inf - Inf; any other score is refused), the products
and sums elementwise in float64 (no BLAS: 0 * Inf and 0 * NaN are NaN by IEEE), in fp32 where the
accumulator must overflow, then the integer nearest-even encoding `bf16_bits_rne` of the fp32
pattern.  NaNs are compared by class, everything else bitwise.

  A. every finite bf16 code as a V element with probability exactly 1: 510 (sequence, KV head) pairs
     of a launch of 64 sequences x 8 KV heads hold 128 consecutive codes each as their target's V
     row (two pairs repeat the subnormal rows); all heads of a group aim at that one token.  Decode
     at groups 1, 4, 16; prefill on the same caches with chunks of 1, 3 and 9 tokens whose queries
     all aim at the target, which lies at or below the chunk's first position.  out == the code,
     subnormals and +-0x7F7F included; for the two zero codes either sign is accepted (an
     accumulator zeroed by alpha = 0 keeps the sign of what it held).
  B. two matched tokens in blocks of different decode waves, V pairs crafted per d: (v, next code
     up) -- the mean is a rounding tie, with mantissa 0x7F it carries into the exponent, with
     exponent 0 it is subnormal --, (v, v), (v, -v), and (0x7F7F, 0x7F7F) whose fp32 sum overflows.
     A sum that is exactly zero may come out with either sign.
  C. one NaN / +-Inf planted into q, K or V of a pair-regime (decode) or match-regime (prefill)
     baseline reaches exactly its dependants: the whole case is compared with its own reference,
     and that the reference differs from the baseline in exactly the predicted cells is asserted on
     the CPU (test_attn_numeric_edges_helpers.py).  Prefill leaves the queries before a planted
     token of its own (sequence, KV head) uncompared where the token lies inside the chunk (two
     cases; at most 5 % of a launch).
  D. scale: 0.0 (every score 0: the exact uniform mean -- a baked-in default scale fails), the
     negated default on one-hot operands (the target's probability is exactly 0, the 2^k others
     share the rest), and the random regime of the exact modules at 2^-4 and 2^-3 against the
     float64 softmax at that scale.

Parts A, B and D also run through the split-KV launch pair (decode with kv_splits >= 2: a second place
where partials are weighed, summed, divided and rounded, behind a global-memory workspace): A at 2 and 4
splits (at 4 the one-block contexts have empty splits), B at 2 and 4 on the same layout, which by the
partition rule (SPL.split_of) holds pairs whose two tokens lie in different splits and pairs that share
one -- the expectation stays the one fp32 sum, one division, one rounding --, D at 3 splits (uneven: bps
does not divide nblk) and 4.  What the split counts cover is asserted by `split_coverage` on the operands
alone.  The workspace is the split module's guarded window, NaN-filled before every launch: a word the
merge reads without this launch having written it poisons the output.

Every launch runs guarded as in the two exact modules: q a window of a NaN-filled allocation (with
NaN rows before and after the chunks for prefill), out a window of a SENT16-filled allocation
compared bitwise, NaN in the blocks no table entry names and in the slots past ctx, SENT32 around
the integer operands.  No planted value is an index: block ids, context lengths and q_start stay
valid, and every launch runs with check=True.

The builders, the expectations and the comparison are CPU-tested in
test_attn_numeric_edges_helpers.py, which runs without a GPU.
"""
import functools

import pytest
import torch

import test_gpu_decode_attn_exact as ATT
import test_gpu_decode_split_exact as SPL
import test_gpu_prefill_attn_exact as PRE
from test_gpu_kernels_exact import NAN, SENT16, SENT32, guarded_input, guarded_output, guarded_vector, guards_intact
from test_gpu_numeric_edges import bf16_bits_rne, bf16_to_bits, bits_to_f32, edges_match, f32_is_nan, f32_to_bits

pytestmark = pytest.mark.gpu

# MEASURED on an MI355X (printed by the tests):
MEASURED = """
  random regime, max|out - ref| against the bound 0.00781 (max|V| = 1.0): at scale 2^-4 decode 0.00112 and prefill
  0.00283 (max|score| 2.83 and 3.49), at scale 2^-3 decode 0.00216 and prefill 0.00265 (max|score| 5.66 and 6.98).
  Every finite code, the subnormals of both signs and +-0x7F7F included, came out unchanged at every group
  size from both kernels: the P . V MFMA flushes no bf16 subnormal operand.  Every zero came out as +0.0: the
  -0.0 code with probability 1, and each of the 1404 (decode) and 6300 (prefill) exactly-zero sums of a pair.
  The seven decode q and K cases of part C are the ones that see a merge which guards its division with
  `lsum > 0`: it writes +0.0 in exactly their dependants ("[4, 5, 0] got=0x0000 exp=NaN").
  The module: 45 tests in 5 s.
  Split mode (16 tests in 0.9 s; the module is now 61 tests in 3 s): every finite code came out unchanged at 2 and
  4 splits and every group size, every zero as +0.0; pairs: 4 within one split and 4 across two at 2 splits, 2 and 6
  at 4, each of the 1404 exactly-zero sums +0.0; random regime at 3 and 4 splits 0.00112 (scale 2^-4) and 0.00216
  (2^-3), the unsplit launch's figures.  A merge that weighs every non-empty split by 1 fails A, B, the negated
  scale ("[4, 1, 0] got=0xbe59 exp=0xbe20": ctx 33, the head whose target is alone in split 1) and the random
  regime (0.123 and 0.359), not scale 0; a split launch that ignores `scale` fails all of part D.
"""

D, T, SCALE, C0, R0 = ATT.D, ATT.T, ATT.SCALE, ATT.C0, PRE.R0
INF = float("inf")
UNDERFLOW = 150.0           # exp(-x) = 2^(-x log2 e) is below fp32's smallest subnormal from x = 104 on; 150 for margin
ROW_BATCH = 32              # query rows per elementwise [rows, group, ctx, D] product
UNCOMPARED_CAP = 0.05       # part C, prefill: at most this share of a launch's cells is left uncompared


# ------------------------------------------------------------------------------------------------
# operands of one launch, and the explicit reference (CPU-tested in test_attn_numeric_edges_helpers.py)
# ------------------------------------------------------------------------------------------------
class Ops:
    """The logical operands of one launch as fp32 tensors of bf16 values: per sequence K and V
    [Hkv, ctx, D]; q [rows, Hq, D].  q_lens None is a decode launch: one row per sequence, at
    position ctx - 1 (a sequence with ctx == 0 has a row too, whose output is +0.0).  Otherwise the
    rows are the sequences' chunks, packed."""

    def __init__(self, group, hkv, ctxs, q_lens, q, ks, vs, seed):
        self.group, self.hkv, self.Hq = group, hkv, group * hkv
        self.ctxs, self.q_lens = tuple(ctxs), None if q_lens is None else tuple(q_lens)
        self.q, self.ks, self.vs, self.seed = q, ks, vs, seed
        self.R = len(ctxs) if q_lens is None else sum(q_lens)
        assert q.shape == (self.R, self.Hq, D) and len(ks) == len(vs) == len(ctxs)
        assert all(k.shape == v.shape == (hkv, c, D) for k, v, c in zip(ks, vs, ctxs))

    @property
    def decode(self):
        return self.q_lens is None

    def rows(self, s):
        """(first row, row count, positions [count]) of sequence s."""
        if self.decode:
            return s, 1, torch.tensor([self.ctxs[s] - 1])
        n = self.q_lens[s]
        return sum(self.q_lens[:s]), n, self.ctxs[s] - n + torch.arange(n)

    def copy(self):
        return Ops(self.group, self.hkv, self.ctxs, self.q_lens, self.q.clone(), [k.clone() for k in self.ks],
                   [v.clone() for v in self.vs], self.seed)


def contract_probabilities(q, k, scale, pos):
    """float64 [n, G, ctx]: the probabilities the numeric contract gives the queries q [n, G, D] at
    positions pos [n] over the tokens k [ctx, D], for operands whose scores are all-or-nothing.
    The scores are summed elementwise in float64 (a single Inf or NaN operand gives +-Inf or NaN by
    IEEE).  A token above the position has probability 0 (its score is never looked at).  Of the
    others, a NaN or +Inf score (Inf - Inf) is a NaN probability; a score equal to the row's maximum
    is 1; a score at least UNDERFLOW below it, -Inf included, is exactly 0; anything between is
    refused.  A row whose maximum is -Inf is NaN."""
    n, G, _ = q.shape
    ctx = k.shape[0]
    sc = torch.empty(n, G, ctx, dtype=torch.float64)
    for i in range(0, n, ROW_BATCH):
        sc[i:i + ROW_BATCH] = (q[i:i + ROW_BATCH].double()[:, :, None, :] * k.double()[None, None]).sum(-1) * scale
    seen = (torch.arange(ctx)[None, :] <= pos[:, None])[:, None, :].expand(n, G, ctx)
    nan = seen & (sc.isnan() | (sc == INF))
    live = seen & ~nan
    m = sc.masked_fill(~live, -INF).amax(-1, keepdim=True)           # fmax: a NaN is no maximum
    top = live & (sc == m) & (m > -INF)
    gap = (m - sc)[live & ~top]
    assert not bool((gap < UNDERFLOW).any()), "a score is neither the maximum nor far enough below it"
    p = torch.where(nan, torch.full_like(sc, NAN), top.double())
    return torch.where((m == -INF).expand_as(p) & seen, torch.full_like(p, NAN), p)


def explicit_reference(p, v, fp32=False, pos=None):
    """[n, G, D] = (sum_t p[.., t] * v[t, :]) / (sum_t p[.., t]), elementwise products and sums in
    float64, or all in fp32 (where the fp32 accumulator has to overflow).  With pos [n], the tokens
    above a row's position are no terms of its sum (0 * Inf there is not the reference's to judge)."""
    dt = torch.float32 if fp32 else torch.float64
    p, v = p.to(dt), v.to(dt)
    out = torch.empty(p.shape[0], p.shape[1], D, dtype=dt)
    for i in range(0, p.shape[0], ROW_BATCH):
        terms = p[i:i + ROW_BATCH, :, :, None] * v[None, None]
        if pos is not None:
            above = torch.arange(v.shape[0])[None, :] > pos[i:i + ROW_BATCH, None]
            terms = terms.masked_fill(above[:, None, :, None], 0)
        out[i:i + ROW_BATCH] = terms.sum(2)
    return out / p.sum(-1, keepdim=True)


def probabilities(ops, s, kv, scale=SCALE):
    """contract_probabilities of (sequence s, KV head kv): [n, group, ctx]."""
    r0, n, pos = ops.rows(s)
    q = ops.q[r0:r0 + n, kv * ops.group:(kv + 1) * ops.group]
    return contract_probabilities(q, ops.ks[s][kv], scale, pos)


def reference(ops, scale=SCALE, fp32=False, only=None, base=None):
    """[R, Hq, D] float64 (fp32 with fp32=True).  only=(s, kv) recomputes that pair alone into a copy
    of `base`.  A decode row with ctx == 0 is +0.0."""
    out = torch.zeros(ops.R, ops.Hq, D, dtype=torch.float32 if fp32 else torch.float64) if base is None else base.clone()
    for s, ctx in enumerate(ops.ctxs):
        r0, n, _ = ops.rows(s)
        if n == 0 or ctx == 0:
            continue
        for kv in range(ops.hkv):
            if only is None or only == (s, kv):
                p = probabilities(ops, s, kv, scale)
                out[r0:r0 + n, heads_of(ops, kv)] = explicit_reference(p, ops.vs[s][kv], fp32, ops.rows(s)[2])
    return out


def expected_bits(ref):
    """(bf16 patterns, NaN mask) of a reference: its fp32 pattern through bf16_bits_rne."""
    u = f32_to_bits(ref.float())
    return bf16_bits_rne(u), f32_is_nan(u)


def exact_in_fp32(ref):
    """Elementwise: the float64 value is an fp32 value (NaN and Inf count as exact)."""
    return (ref.float().double() == ref) | ref.isnan()


def cell_mismatches(got, exp, nan, either_zero=None, skip=None):
    """Bool mask of the cells of got (bf16 patterns) that are wrong: not a NaN where `nan`, not exp
    bitwise elsewhere.  Where either_zero, +0.0 and -0.0 both pass; where skip, anything does."""
    ok = edges_match(got, exp, nan)
    if either_zero is not None:
        ok = ok | (either_zero & ((got & 0x7FFF) == 0))
    if skip is not None:
        ok = ok | skip
    return ~ok


def assert_cells(got, exp, nan, what, either_zero=None, skip=None, limit=6):
    bad = cell_mismatches(got, exp, nan, either_zero, skip).nonzero()
    if len(bad):
        rows = [f"[{r}, {h}, {d}] got={int(got[r, h, d]):#06x} exp=" + ("NaN" if bool(nan[r, h, d]) else f"{int(exp[r, h, d]):#06x}")
                for r, h, d in bad[:limit].tolist()]
        raise AssertionError((what, f"{len(bad)} cells differ (row, head, d): " + "; ".join(rows)))


def heads_of(ops, kv):
    return slice(kv * ops.group, (kv + 1) * ops.group)


# ------------------------------------------------------------------------------------------------
# A. every finite bf16 code
# ------------------------------------------------------------------------------------------------
CODE_S, CODE_HKV = 64, 8
CODE_CTXS = (1, 33, 64, 97, 130)
CODE_CHUNKS = (1, 3, 9)
CODE_GROUPS = (1, 4, 16)
CODE_REPEATS = (0, 255)             # the rows of the code table the two spare pairs repeat: the subnormals of either sign


def finite_codes():
    c = torch.arange(1 << 16)
    return c[(c & 0x7F80) != 0x7F80]


def code_rows():
    """int64 [512, 128]: row i is the target V row of (sequence i // 8, KV head i % 8) as bf16 codes."""
    rows = finite_codes().view(-1, D)
    assert rows.shape[0] == CODE_S * CODE_HKV - len(CODE_REPEATS) == 510
    return torch.cat([rows, rows[list(CODE_REPEATS)]])


def shared_targets(ctx, n, count, g):
    """Up to `count` tokens at or below ctx - n, the chunk's first position, in the order of
    ATT.targets_for: the first block, the last slot inside ctx, the last block, the other waves'."""
    return [t for t in ATT.targets_for(ctx, max(count, 8), g) if t <= ctx - n][:count]


@functools.lru_cache(maxsize=None)
def code_layout():
    """(ctxs, q_lens, targets [S][Hkv], sign rows [S][Hkv], ks, vs): the caches of part A, the same
    for every group size and for decode and prefill."""
    g = torch.Generator().manual_seed(7100)
    H, codes = ATT.hadamard(), code_rows()
    ctxs = tuple(CODE_CTXS[s % len(CODE_CTXS)] for s in range(CODE_S))
    q_lens = tuple(min(CODE_CHUNKS[s % len(CODE_CHUNKS)], c) for s, c in enumerate(ctxs))
    targets, signs, ks, vs = [], [], [], []
    for s, (ctx, n) in enumerate(zip(ctxs, q_lens)):
        cand = shared_targets(ctx, n, CODE_HKV, g)
        k = 4 * H[64 + torch.randint(0, 64, (CODE_HKV, ctx), generator=g)]
        v = torch.randint(-127, 128, (CODE_HKV, ctx, D), generator=g).float() / 64
        tg = [cand[(kv + s) % len(cand)] for kv in range(CODE_HKV)]
        rs = [(CODE_HKV * s + kv) % 64 for kv in range(CODE_HKV)]
        for kv in range(CODE_HKV):
            k[kv, tg[kv]] = 4 * H[rs[kv]]
            v[kv, tg[kv]] = bits_to_f32(codes[CODE_HKV * s + kv] << 16)
            assert ctx == 1 or bool((v[kv, torch.arange(ctx) != tg[kv]] != 0).any())          # a leak shows
        targets.append(tg), signs.append(rs), ks.append(k), vs.append(v)
    return ctxs, q_lens, targets, signs, ks, vs


def code_ops(group, prefill):
    ctxs, q_lens, _, signs, ks, vs = code_layout()
    H = ATT.hadamard()
    per_seq = [(8 * H[torch.tensor(rs)]).repeat_interleave(group, 0) for rs in signs]          # [Hq, D]
    q = torch.cat([x[None].expand(n, -1, -1) for x, n in zip(per_seq, q_lens)]) if prefill else torch.stack(per_seq)
    return Ops(group, CODE_HKV, ctxs, q_lens if prefill else None, q.contiguous(), ks, vs, seed=7100)


def code_expected(ops):
    """int64 [R, Hq, D]: the code every cell must hold."""
    codes = code_rows().view(CODE_S, CODE_HKV, D)
    return torch.cat([codes[s].repeat_interleave(ops.group, 0)[None].expand(ops.rows(s)[1], -1, -1)
                      for s in range(CODE_S)])


# ------------------------------------------------------------------------------------------------
# B. two matches: the fp32 sum, the division, the rounding
# ------------------------------------------------------------------------------------------------
PAIR_EXPS = (0, 1, 126, 127, 128, 253)
PAIR_MANTS = (0x00, 0x01, 0x7E, 0x7F)
PAIR_CTXS = (65, 130, 257, 97)
PAIR_CHUNKS = (1, 3, 9, 5)
PAIR_GROUP, PAIR_HKV = 4, 2
PAIR_OVERFLOWS = ((0x7F7F, 0x7F7F), (0xFF7F, 0xFF7F))


def pair_table():
    """int64 [146, 2]: the bf16 code pairs; the last two are the overflows."""
    rows = []
    for sign in (0, 0x8000):
        for e in PAIR_EXPS:
            for m in PAIR_MANTS:
                v = sign | (e << 7) | m
                rows += [(v, v + 1), (v, v), (v, v ^ 0x8000)]
    return torch.tensor(rows + list(PAIR_OVERFLOWS))


def pair_entry(s, kv):
    """int64 [128]: the table entry that d of (sequence s, KV head kv) holds."""
    return (torch.arange(D) + D * (PAIR_HKV * s + kv)) % len(pair_table())


@functools.lru_cache(maxsize=None)
def pair_layout():
    """(targets [S][Hkv] of (t, u), ks, vs)."""
    g = torch.Generator().manual_seed(7200)
    H, table = ATT.hadamard(), pair_table()
    targets, ks, vs = [], [], []
    for s, (ctx, n) in enumerate(zip(PAIR_CTXS, PAIR_CHUNKS)):
        cand = shared_targets(ctx, n, 8, g)
        k = 4 * H[64 + torch.randint(0, 64, (PAIR_HKV, ctx), generator=g)]
        v = torch.randint(-127, 128, (PAIR_HKV, ctx, D), generator=g).float() / 64
        tg = []
        for kv in range(PAIR_HKV):
            t = cand[(2 * s + 3 * kv + 1) % len(cand)]
            u = ATT.partner_for(t, ctx, {t})
            assert u is not None and u <= ctx - n and (u // T) % 4 != (t // T) % 4           # different decode waves
            pair = table[pair_entry(s, kv)]
            for tok, col in ((t, 0), (u, 1)):
                k[kv, tok] = 4 * H[PAIR_HKV * s + kv]
                v[kv, tok] = bits_to_f32(pair[:, col] << 16)
            tg.append((t, u))
        targets.append(tg), ks.append(k), vs.append(v)
    return targets, ks, vs


def pair_ops(prefill):
    _, ks, vs = pair_layout()
    H = ATT.hadamard()
    per_seq = [(8 * H[PAIR_HKV * s:PAIR_HKV * (s + 1)]).repeat_interleave(PAIR_GROUP, 0) for s in range(len(PAIR_CTXS))]
    q = torch.cat([x[None].expand(n, -1, -1) for x, n in zip(per_seq, PAIR_CHUNKS)]) if prefill else torch.stack(per_seq)
    return Ops(PAIR_GROUP, PAIR_HKV, PAIR_CTXS, PAIR_CHUNKS if prefill else None, q.contiguous(), ks, vs, seed=7200)


def pair_entries(ops):
    """int64 [R, Hq, D]: the table entry behind every output cell."""
    per_seq = [torch.stack([pair_entry(s, kv) for kv in range(PAIR_HKV)]).repeat_interleave(PAIR_GROUP, 0)
               for s in range(len(PAIR_CTXS))]
    return torch.cat([x[None].expand(ops.rows(s)[1], -1, -1) for s, x in enumerate(per_seq)])


# ------------------------------------------------------------------------------------------------
# C. one non-finite value in q, K or V
# ------------------------------------------------------------------------------------------------
NONFINITE = {"nan": NAN, "+inf": INF, "-inf": -INF}
PLANT_D = 77                        # the d of the V plants


@functools.lru_cache(maxsize=None)
def plant_base(prefill):
    """The baseline: the decode module's pair regime on CTX_B, the prefill module's match regime on
    SEQS_B, both at group 4 with two KV heads."""
    g = torch.Generator().manual_seed(7300 + prefill)
    if prefill:
        q, ks, vs = PRE.logical_operands("match", 4, 2, PRE.SEQS_B, g)
        return Ops(4, 2, [c for c, _ in PRE.SEQS_B], [n for _, n in PRE.SEQS_B], q, ks, vs, seed=7300)
    q, ks, vs = ATT.logical_operands("pair", 4, 2, ATT.CTX_B, g)
    return Ops(4, 2, ATT.CTX_B, None, q, ks, vs, seed=7301)


@functools.lru_cache(maxsize=None)
def plant_base_reference(prefill):
    ref = reference(plant_base(prefill))
    assert bool(exact_in_fp32(ref).all()) and bool(ref.isfinite().all())
    return ref


# name -> (tensor, value, sequence, KV head, where), per mode.  `where` for q: (chunk row of the
# sequence, head of the group); for K and V: (first token, last token, "matched" | "unmatched" | "any"):
# the first token of the range that some query of the pair matches / that none does.
def _plants(prefill):
    if prefill:
        seqs = PRE.SEQS_B
        s_q, s_first, s_last, s_in = seqs.index((255, 100)), seqs.index((255, 100)), seqs.index((129, 1)), seqs.index((160, 33))
        first, last = (2, 31), (128, 128)                # the first block; the partial last block, inside ctx, in the prefix
        v_tok = (40, 120)
        q_row = 50
    else:
        ctxs = ATT.CTX_B
        s_q, s_first, s_last, s_in = ctxs.index(257), ctxs.index(127), ctxs.index(127), None
        first, last = (2, 31), (97, 125)                 # ctx 127: the last block holds tokens 96 .. 126
        v_tok = (40, 120)
        q_row = 0
    out = {}
    for name in NONFINITE:
        out[f"q-{name}"] = ("q", name, s_q, 1, (q_row, 1))
    for name in ("nan", "+inf"):
        out[f"k-first-block-{name}"] = ("k", name, s_first, 1, first + ("any",))
        out[f"k-last-block-{name}"] = ("k", name, s_last, 0, last + ("any",))
    for name in NONFINITE:
        out[f"v-unmatched-{name}"] = ("v", name, s_q, 0, v_tok + ("unmatched",))
        out[f"v-matched-{name}"] = ("v", name, s_q, 1, v_tok + ("matched",))
    if prefill:                                          # a few tokens into the chunk of (160, 33), which starts at token 127
        out["k-in-chunk-nan"] = ("k", "nan", s_in, 1, (130, 131, "any"))
        out["v-in-chunk-+inf"] = ("v", "+inf", s_in, 0, (131, 133, "any"))
    return out


PLANTS = {False: _plants(False), True: _plants(True)}


class Plant:
    """One planted case: the operands, where the value went, the predicted dependants (bool
    [R, Hq, D]) and, for prefill, the cells left uncompared."""

    def __init__(self, prefill, name):
        tensor, value, s, kv, where = PLANTS[prefill][name]
        base = plant_base(prefill)
        self.prefill, self.name, self.tensor, self.value, self.s, self.kv = prefill, name, tensor, NONFINITE[value], s, kv
        self.ops = ops = base.copy()
        r0, n, pos = ops.rows(s)
        heads = heads_of(ops, kv)
        self.dependants = torch.zeros(ops.R, ops.Hq, D, dtype=torch.bool)
        self.uncompared = torch.zeros_like(self.dependants)
        if tensor == "q":
            row, c = where
            h = kv * ops.group + c
            self.d0 = next(d for d in range(1, D) if bool((ops.ks[s][kv][:, d] != 0).any()))
            self.at = (r0 + row, h, self.d0)
            ops.q[self.at] = self.value
            self.dependants[r0 + row, h] = True
            return
        p = probabilities(base, s, kv)                                       # [n, group, ctx]
        lo, hi, kind = where
        hit = p.sum((0, 1)) > 0                                              # tokens some query of the pair matches
        self.t = t = next(t for t in range(lo, hi + 1) if kind == "any" or bool(hit[t]) == (kind == "matched"))
        after = pos >= t                                                     # the queries that attend token t
        self.uncompared[r0:r0 + n, heads] = ~after[:, None, None]
        if tensor == "v":
            self.d0 = PLANT_D
            ops.vs[s][kv, t, self.d0] = self.value
            self.dependants[r0:r0 + n, heads, self.d0] = after[:, None]
            return
        # K: a d at which every query that matches t has a positive element (its score is then +Inf
        # and not -Inf: no matched token is lost to probability 0) and the others have both signs
        qs = ops.q[r0:r0 + n, heads][after]                                  # [rows, group, D]
        matched = p[after][:, :, t] > 0
        self.d0 = next(d for d in range(1, D) if bool((qs[..., d][matched] > 0).all())
                       and bool((qs[..., d] > 0).any()) and bool((qs[..., d] < 0).any()))
        ops.ks[s][kv, t, self.d0] = self.value
        poisoned = torch.ones(n, ops.group, dtype=torch.bool) if value == "nan" else ops.q[r0:r0 + n, heads, self.d0] > 0
        self.dependants[r0:r0 + n, heads] = (poisoned & after[:, None])[:, :, None]

    def reference(self):
        """Only the planted (sequence, KV head) is computed anew; the rest is the baseline's."""
        return reference(self.ops, only=(self.s, self.kv), base=plant_base_reference(self.prefill))


@functools.lru_cache(maxsize=None)
def plant(prefill, name):
    return Plant(prefill, name)


# ------------------------------------------------------------------------------------------------
# D. scale
# ------------------------------------------------------------------------------------------------
NEG_CTXS = (3, 5, 9, 17, 33, 65, 129, 257)              # 2^k + 1
RANDOM_SCALES = (2.0 ** -4, 2.0 ** -3)
SCORE_CAP = 10.0                    # the random regime's bound is derived for |score| <~ 10


def zero_scale_ops(prefill):
    """q and K randn rounded to bf16, V integers in [-4, 4]; decode on CTX_UNIFORM (powers of two),
    prefill on SEQS_B."""
    g = torch.Generator().manual_seed(7400 + prefill)
    if prefill:
        q, ks, vs = PRE.logical_operands("uniform", 4, 2, PRE.SEQS_B, g)
        ctxs, q_lens = [c for c, _ in PRE.SEQS_B], [n for _, n in PRE.SEQS_B]
    else:
        q, ks, vs = ATT.logical_operands("uniform", 4, 2, ATT.CTX_UNIFORM, g)
        ctxs, q_lens = ATT.CTX_UNIFORM, None
    assert not q.any()
    q = torch.randn(q.shape, generator=g).to(torch.bfloat16).float()
    return Ops(4, 2, ctxs, q_lens, q, ks, vs, seed=7400)


def zero_scale_expected(ops):
    """(bits, nan) at scale 0.  Decode: the explicit reference -- every probability is 1, the sum is
    exact and ctx a power of two.  Prefill: the prefill module's exact fp32 quotient of the
    uniform regime, fp32(sum) / fp32(p + 1)."""
    if ops.decode:
        ref = reference(ops, scale=0.0)
        assert bool(exact_in_fp32(ref).all())
        return expected_bits(ref)
    exact, _ = PRE.exact_expectation("uniform", ops.group, ops.hkv, tuple(zip(ops.ctxs, ops.q_lens)), ops.vs)
    return expected_bits(exact)


def negated_scale_ops():
    """The decode module's one-hot operands (a target per head) with integer V, on contexts of
    2^k + 1 tokens."""
    g = torch.Generator().manual_seed(7500)
    q, ks, _ = ATT.logical_operands("onehot", 4, 2, NEG_CTXS, g)
    vs = [torch.randint(-4, 5, (2, c, D), generator=g).float() for c in NEG_CTXS]
    return Ops(4, 2, NEG_CTXS, None, q, ks, vs, seed=7500)


def softmax_case(prefill):
    """The random regime of the exact modules at group 4, two KV heads."""
    g = torch.Generator().manual_seed(7600 + prefill)
    if prefill:
        q, ks, vs = PRE.logical_operands("random", 4, 2, PRE.SEQS_B, g)
        return Ops(4, 2, [c for c, _ in PRE.SEQS_B], [n for _, n in PRE.SEQS_B], q, ks, vs, seed=7600)
    q, ks, vs = ATT.logical_operands("random", 4, 2, ATT.CTX_B, g)
    return Ops(4, 2, ATT.CTX_B, None, q, ks, vs, seed=7601)


def max_abs_score(ops, scale):
    """max |scale * q . k| over every (query, token at or below its position)."""
    worst = 0.0
    for s, ctx in enumerate(ops.ctxs):
        r0, n, pos = ops.rows(s)
        if n == 0 or ctx == 0:
            continue
        q = ops.q[r0:r0 + n].double().view(n, ops.hkv, ops.group, D)
        sc = torch.einsum("ngcd,gtd->ngct", q, ops.ks[s].double()) * scale
        seen = torch.arange(ctx)[None, :] <= pos[:, None]
        worst = max(worst, float(sc.abs().masked_fill(~seen[:, None, None, :], 0).max()))
    return worst


# ------------------------------------------------------------------------------------------------
# the split mode of parts A, B and D: what a split count covers, by the split module's partition rule
# ------------------------------------------------------------------------------------------------
CODE_SPLITS = (2, 4)
PAIR_SPLITS = (2, 4)
SCALE_SPLITS = (3, 4)               # 3 is uneven on every part D case; 4 the power of two


def split_sizes(ctx, kv_splits):
    """Blocks per split, by the partition rule."""
    return [hi - lo for lo, hi in (SPL.split_range(ctx, kv_splits, p) for p in range(kv_splits))]


def split_coverage(part, kv_splits):
    """Asserts on the operands alone what a split count covers for a part, and returns the figures."""
    if part == "codes":
        ctxs, _, targets, _, _, _ = code_layout()
        empty = {c for c in set(ctxs) if 0 in split_sizes(c, kv_splits)}
        used = {SPL.split_of(t, c, kv_splits) for c, ts in zip(ctxs, targets) for t in ts}
        assert len(used) >= 2 and 0 in used                                 # targets in the first and in later splits
        if kv_splits == 4:
            one_block = {c for c in set(ctxs) if c <= T}
            assert one_block and one_block <= empty                         # the one-block contexts have empty splits
            assert any(split_sizes(c, 4).count(0) == 0 for c in set(ctxs))  # ... beside sequences that fill all four
        return {"empty": sorted(empty), "splits with a target": sorted(used)}
    if part == "pairs":
        targets, _, _ = pair_layout()
        shared = [SPL.split_of(t, ctx, kv_splits) == SPL.split_of(u, ctx, kv_splits)
                  for ctx, tg in zip(PAIR_CTXS, targets) for t, u in tg]
        assert any(shared) and not all(shared)                              # pairs within one split, pairs across two
        # ... and of each kind one whose d run holds the two overflow entries: Inf from a walk and from the merge
        over = [bool((pair_entry(s, kv) >= len(pair_table()) - 2).any()) for s in range(len(PAIR_CTXS)) for kv in range(PAIR_HKV)]
        assert {sh for sh, o in zip(shared, over) if o} == {True, False}
        return {"within": sum(shared), "across": len(shared) - sum(shared)}
    ctxs = {"scale 0": ATT.CTX_UNIFORM, "negated": NEG_CTXS, "random": ATT.CTX_B}[part]
    sizes = [[n for n in split_sizes(c, kv_splits) if n] for c in ctxs if c]
    uneven = [sz for sz in sizes if len(set(sz)) > 1]
    if kv_splits == 3:
        assert uneven                                                       # bps does not divide nblk
    assert any(len(sz) >= 3 for sz in sizes) and any(len(sz) < kv_splits for sz in sizes)         # and empty splits
    return {"uneven": len(uneven), "sequences": len(sizes)}


def lonely_target(ops):
    """The negated-scale case holds a split whose only token is some head's target: ctx 33 has token 32
    alone in block 1, which is split 1 at every split count, and it has probability 0 for a head."""
    s = ops.ctxs.index(T + 1)
    p = probabilities(ops, s, 0, -SCALE)[0]                                 # [group, 33]
    return all(split_sizes(T + 1, k)[:2] == [1, 1] for k in SCALE_SPLITS) and bool((p[:, T] == 0).any())


def order_free_sums(ops):
    """The V of the scale-0 and negated-scale cases are integers in [-4, 4] over at most 257 tokens: every
    partial sum, in any order and over any split, is an integer below 2^24 -- exact in fp32."""
    return all(torch.equal(v, v.round()) and float(v.abs().max()) <= 4 for v in ops.vs if v.numel()) and 4 * max(ops.ctxs) < 1 << 24


# ------------------------------------------------------------------------------------------------
# GPU plumbing
# ------------------------------------------------------------------------------------------------
class Launch:
    """The guarded device buffers of an Ops, as the Case classes of the two exact modules build
    them; run() launches and returns the output rows as bf16 patterns on the CPU."""

    def __init__(self, ops):
        self.ops = ops
        self.table_cpu, self.nb = PRE.block_tables(ops.ctxs, torch.Generator().manual_seed(ops.seed))
        self.kc_cpu, self.vc_cpu = ATT.paged_caches(ops.ks, ops.vs, self.table_cpu, self.nb, ops.hkv)
        self.ctx_cpu = torch.tensor(ops.ctxs, dtype=torch.int32)
        self.lead = 0 if ops.decode else PRE.LEAD
        self.rows = ops.R if ops.decode else PRE.LEAD + ops.R + PRE.TRAIL
        qfull = torch.full((self.rows, ops.Hq, D), NAN)
        qfull[self.lead:self.lead + ops.R] = ops.q
        self.q_cpu = qfull.to(torch.bfloat16)
        mine = self.q_cpu[self.lead:self.lead + ops.R].float()
        assert torch.equal(mine.nan_to_num(7.0), ops.q.nan_to_num(7.0)) and torch.equal(mine.isnan(), ops.q.isnan())
        self.q_start_cpu = None if ops.decode else torch.tensor([PRE.LEAD] + list(ops.q_lens)).cumsum(0).to(torch.int32)

    def upload(self):
        ops, W = self.ops, self.ops.Hq * D
        self.W = W
        self.q = guarded_input(self.q_cpu.view(self.rows, W).cuda(), W + C0, c0=C0).unflatten(1, (ops.Hq, D))
        self.kc, self.vc = self.kc_cpu.cuda(), self.vc_cpu.cuda()
        self.table_raw, self.table = ATT.guarded_ints_2d(self.table_cpu, self.table_cpu.shape[1] + 2)
        self.ctx_raw, self.ctx = PRE.guarded_ints(self.ctx_cpu)
        if not ops.decode:
            self.q_start_raw, self.q_start = PRE.guarded_ints(self.q_start_cpu)
        self.raw, out2d = guarded_output(self.rows, W, W + C0, C0, "cuda")
        self.out = out2d.unflatten(1, (ops.Hq, D))
        assert self.q.data_ptr() % 16 == 0 and self.out.data_ptr() % 16 == 0 and self.q.stride(0) == W + C0
        return self

    def run(self, what, scale=None, kv_splits=1):
        """kv_splits >= 2 (decode only) is the split-KV launch pair with the caller's workspace: the split
        module's guarded window of exactly the floats the launch needs, all NaN before the launch."""
        from k8s_gpu_scheduler_amd.ops import loadgen
        self.raw.fill_(SENT16)
        if self.ops.decode:
            kw = {}
            if kv_splits > 1:
                n = loadgen.decode_split_workspace_floats(self.ops.R, self.ops.Hq, kv_splits)
                ws_raw, ws = guarded_vector(n, SPL.WS_BEFORE, SPL.WS_AFTER, "cuda")
                assert ws.data_ptr() % 16 == 0 and ws.numel() == n
                ws.fill_(NAN)
                kw = dict(kv_splits=kv_splits, workspace=ws)
            loadgen.paged_decode_attention(self.q, self.kc, self.vc, self.table, self.ctx, out=self.out, scale=scale, **kw)
            if kv_splits > 1:
                torch.cuda.synchronize()
                assert guards_intact(ws_raw, slice(SPL.WS_BEFORE, SPL.WS_BEFORE + n), SENT32), ("write outside the workspace", what)
        else:
            assert kv_splits == 1
            loadgen.paged_prefill_attention(self.q, self.kc, self.vc, self.table, self.ctx, self.q_start, out=self.out,
                                            scale=scale)
        torch.cuda.synchronize()
        written = (slice(R0 + self.lead, R0 + self.lead + self.ops.R), slice(C0, C0 + self.W))
        assert guards_intact(self.raw, written, SENT16), ("write outside the window", what)
        return bf16_to_bits(self.out[self.lead:self.lead + self.ops.R]).cpu()


def launch(ops):
    return Launch(ops).upload()


MODES = pytest.mark.parametrize("prefill", [False, True], ids=["decode", "prefill"])


# ------------------------------------------------------------------------------------------------
# A. every finite bf16 code with probability 1
# ------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("group", CODE_GROUPS)
def test_every_finite_code_passes_through(group, prefill):
    ops = code_ops(group, prefill)
    codes = code_expected(ops)
    either = (codes & 0x7FFF) == 0                                           # the two zero codes: either sign
    exp, nan = expected_bits(reference(ops))
    assert not cell_mismatches(exp, codes, nan, either).any() and not nan.any()           # the reference is the code itself
    got = launch(ops).run(("codes", group, prefill))
    print(f"codes, group {group}, {'prefill' if prefill else 'decode'}: {int((got >> 15)[either].sum())} of the "
          f"{int(either.sum())} zero-code cells ({int((codes == 0x8000).sum())} of them -0.0) came out as -0.0")
    assert_cells(got, codes, nan, ("codes", group, prefill), either_zero=either)


@pytest.mark.parametrize("kv_splits", CODE_SPLITS)
@pytest.mark.parametrize("group", CODE_GROUPS)
def test_every_finite_code_passes_through_the_split_launch(group, kv_splits):
    """The target's split has m = 362 and l = 1; every other non-empty split has m = 0 and merge weight
    exp2(-362 log2 e) = 0, an empty one m = -inf and weight 0: the merged row is the code."""
    split_coverage("codes", kv_splits)
    ops = code_ops(group, False)
    codes = code_expected(ops)
    either = (codes & 0x7FFF) == 0
    exp, nan = expected_bits(reference(ops))
    assert not cell_mismatches(exp, codes, nan, either).any() and not nan.any()
    got = launch(ops).run(("codes", group, "split", kv_splits), kv_splits=kv_splits)
    assert_cells(got, codes, nan, ("codes", group, "split", kv_splits), either_zero=either)


# ------------------------------------------------------------------------------------------------
# B. pairs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kv_splits", PAIR_SPLITS)
def test_pairs_sum_divide_and_round_through_the_split_launch(kv_splits):
    """A pair across two splits: each partial is the token's V with m = 362 and l = 1, the merge weighs both
    by exactly 1 and adds them in fp32; a pair within one split is added by that split's walk.  Either way
    one fp32 sum, one division by 2, one rounding -- and Inf for the two overflow pairs."""
    cover = split_coverage("pairs", kv_splits)
    ops = pair_ops(False)
    ref = reference(ops, fp32=True)
    exp, nan = expected_bits(ref)
    assert not nan.any() and bool((exp == 0x7F80).any()) and bool((exp == 0xFF80).any())
    got = launch(ops).run(("pairs", "split", kv_splits), kv_splits=kv_splits)
    print(f"pairs, {kv_splits} splits: {cover['within']} pairs within one split, {cover['across']} across two; "
          f"{int((got >> 15)[ref == 0].sum())} of {int((ref == 0).sum())} exactly-zero cells came out as -0.0")
    assert_cells(got, exp, nan, ("pairs", "split", kv_splits), either_zero=ref == 0)


@MODES
def test_pairs_sum_divide_and_round(prefill):
    ops = pair_ops(prefill)
    ref = reference(ops, fp32=True)
    exp, nan = expected_bits(ref)
    assert not nan.any()
    got = launch(ops).run(("pairs", prefill))
    # an exact zero -- (v, -v), and the pairs of zeros -- has either sign; a value that only rounds to zero keeps its own
    print(f"pairs, {'prefill' if prefill else 'decode'}: {int((got >> 15)[ref == 0].sum())} of {int((ref == 0).sum())} "
          f"exactly-zero cells came out as -0.0")
    assert_cells(got, exp, nan, ("pairs", prefill), either_zero=ref == 0)


# ------------------------------------------------------------------------------------------------
# C. planted non-finite values
# ------------------------------------------------------------------------------------------------
@MODES
def test_plant_baseline(prefill):
    base = plant_base(prefill)
    exp, nan = expected_bits(plant_base_reference(prefill))
    got = launch(base).run(("baseline", prefill))
    assert_cells(got, exp, nan, ("baseline", prefill))
    if base.decode:
        for s, c in enumerate(base.ctxs):
            assert c or not got[s].any(), "ctx == 0 must give +0.0"


@pytest.mark.parametrize("prefill,name", [pytest.param(m, n, id=("prefill-" if m else "decode-") + n)
                                          for m in (False, True) for n in PLANTS[m]])
def test_nonfinite_reaches_exactly_its_dependants(prefill, name):
    c = plant(prefill, name)
    exp, nan = expected_bits(c.reference())
    got = launch(c.ops).run((name, prefill))
    assert_cells(got, exp, nan, (name, "prefill" if prefill else "decode"), skip=c.uncompared if prefill else None)
    if c.ops.decode:
        for s, n in enumerate(c.ops.ctxs):
            assert n or not got[s].any(), "ctx == 0 must give +0.0"


# ------------------------------------------------------------------------------------------------
# D. scale
# ------------------------------------------------------------------------------------------------
@MODES
def test_scale_zero_is_the_uniform_mean(prefill):
    ops = zero_scale_ops(prefill)
    exp, nan = zero_scale_expected(ops)
    got = launch(ops).run(("scale 0", prefill), scale=0.0)
    assert_cells(got, exp, nan, ("scale 0", prefill))


def test_negated_scale_gives_the_target_probability_zero():
    ops = negated_scale_ops()
    ref = reference(ops, scale=-SCALE)
    assert bool(exact_in_fp32(ref).all())
    exp, nan = expected_bits(ref)
    got = launch(ops).run("scale -1/sqrt(128)", scale=-SCALE)
    assert_cells(got, exp, nan, "scale -1/sqrt(128)")


@MODES
@pytest.mark.parametrize("scale", RANDOM_SCALES, ids=["2^-4", "2^-3"])
def test_random_regime_at_other_scales(scale, prefill):
    ops = softmax_case(prefill)
    worst = max_abs_score(ops, scale)
    assert worst <= SCORE_CAP, worst
    ln = launch(ops)
    if prefill:
        ref = PRE.reference(ln.q_cpu, ln.kc_cpu, ln.vc_cpu, ln.table_cpu, ln.ctx_cpu, ln.q_start_cpu, scale=scale)[ln.lead:ln.lead + ops.R]
    else:
        ref = ATT.reference(ln.q_cpu, ln.kc_cpu, ln.vc_cpu, ln.table_cpu, ln.ctx_cpu, scale=scale)
    got = bits_to_f32(ln.run(("random", scale, prefill), scale=scale) << 16).double()
    vmax = max(float(v.abs().max()) for v in ops.vs if v.numel())
    err = (got - ref).abs().max().item()
    print(f"{'prefill' if prefill else 'decode'} attention, random regime at scale {scale}: max|out - ref| = {err:.5f} "
          f"(bound {ATT.RANDOM_BOUND * vmax:.5f}, max|V| = {vmax:.4f}, max|score| = {worst:.2f})")
    assert err <= ATT.RANDOM_BOUND * vmax, (scale, prefill, err)


@pytest.mark.parametrize("kv_splits", SCALE_SPLITS)
def test_scale_zero_is_the_uniform_mean_through_the_split_launch(kv_splits):
    """Every split has m = 0 and merge weight 1; its normaliser is its token count."""
    split_coverage("scale 0", kv_splits)
    ops = zero_scale_ops(False)
    assert order_free_sums(ops)
    exp, nan = zero_scale_expected(ops)
    got = launch(ops).run(("scale 0", "split", kv_splits), scale=0.0, kv_splits=kv_splits)
    assert_cells(got, exp, nan, ("scale 0", "split", kv_splits))


@pytest.mark.parametrize("kv_splits", SCALE_SPLITS)
def test_negated_scale_gives_the_target_probability_zero_through_the_split_launch(kv_splits):
    """A split that holds a target has m = 0 from its other tokens -- or, where the target is its only
    token (ctx 33: token 32 alone in block 1), m = -362 and l = 1, which the merge must weigh by
    exp2(-362 log2 e) = 0 beside the other splits' m = 0."""
    split_coverage("negated", kv_splits)
    ops = negated_scale_ops()
    assert order_free_sums(ops)
    assert lonely_target(ops)
    ref = reference(ops, scale=-SCALE)
    assert bool(exact_in_fp32(ref).all())
    exp, nan = expected_bits(ref)
    got = launch(ops).run(("scale -1/sqrt(128)", "split", kv_splits), scale=-SCALE, kv_splits=kv_splits)
    assert_cells(got, exp, nan, ("scale -1/sqrt(128)", "split", kv_splits))


@pytest.mark.parametrize("kv_splits", SCALE_SPLITS)
@pytest.mark.parametrize("scale", RANDOM_SCALES, ids=["2^-4", "2^-3"])
def test_random_regime_at_other_scales_through_the_split_launch(scale, kv_splits):
    split_coverage("random", kv_splits)
    ops = softmax_case(False)
    worst = max_abs_score(ops, scale)
    assert worst <= SCORE_CAP, worst
    ln = launch(ops)
    ref = ATT.reference(ln.q_cpu, ln.kc_cpu, ln.vc_cpu, ln.table_cpu, ln.ctx_cpu, scale=scale)
    got = bits_to_f32(ln.run(("random", scale, "split", kv_splits), scale=scale, kv_splits=kv_splits) << 16).double()
    vmax = max(float(v.abs().max()) for v in ops.vs if v.numel())
    err = (got - ref).abs().max().item()
    print(f"split decode attention ({kv_splits} splits), random regime at scale {scale}: max|out - ref| = {err:.5f} "
          f"(bound {ATT.RANDOM_BOUND * vmax:.5f}, max|V| = {vmax:.4f}, max|score| = {worst:.2f})")
    assert err <= ATT.RANDOM_BOUND * vmax, (scale, kv_splits, err)
