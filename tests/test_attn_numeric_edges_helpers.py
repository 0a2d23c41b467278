"""CPU-only tests of the builders, the expectations and the comparison of
test_gpu_attn_numeric_edges.py: the code table holds every finite bf16 code once and its targets sit
where the kernels change path, the pair table holds the rounding classes it is there for, every
planted non-finite value changes exactly the cells the contract names, the cells prefill leaves
uncompared stay under the cap, and the comparison rejects the wrong outputs it is there to catch."""
import pytest
import torch

import test_gpu_attn_numeric_edges as A
import test_gpu_decode_attn_exact as ATT
import test_gpu_prefill_attn_exact as PRE
from test_gpu_numeric_edges import bf16_is_nan, bf16_to_bits, bits_to_f32

D, T = A.D, A.T
NAN, INF = A.NAN, A.INF


def same(a, b):
    """Equal, NaN == NaN."""
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0))


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
def test_contract_probabilities_by_score_class():
    H = ATT.hadamard()
    q = (8 * H[:2])[None]                                                # one row, two heads
    k = torch.stack([4 * H[0], 4 * H[70], 4 * H[1], 4 * H[0], 4 * H[90]])
    p = A.contract_probabilities(q, k, A.SCALE, torch.tensor([4]))
    assert p.tolist() == [[[1, 0, 0, 1, 0], [0, 0, 1, 0, 0]]]
    assert A.contract_probabilities(q, k, A.SCALE, torch.tensor([2])).tolist() == [[[1, 0, 0, 0, 0], [0, 0, 1, 0, 0]]]
    assert A.contract_probabilities(q, k, 0.0, torch.tensor([3])).tolist() == [[[1, 1, 1, 1, 0]] * 2]
    assert A.contract_probabilities(q, k, -A.SCALE, torch.tensor([4])).tolist() == [[[0, 1, 1, 0, 1], [1, 1, 0, 1, 1]]]
    # d = 1: H[0] is +, H[1] is -.  +Inf in K there is a +Inf score for head 0 (NaN) and -Inf for head 1 (0)
    for value, want in ((INF, [[NAN, 0, 0, 1, 0], [0, 0, 1, 0, 0]]), (NAN, [[NAN, 0, 0, 1, 0], [NAN, 0, 1, 0, 0]])):
        kk = k.clone()
        kk[0, 1] = value
        assert same(A.contract_probabilities(q, kk, A.SCALE, torch.tensor([4])), torch.tensor([want], dtype=torch.float64))
    kk = k.clone()
    kk[3, 1] = INF                                                        # above the position: never looked at
    assert A.contract_probabilities(q, kk, A.SCALE, torch.tensor([2])).tolist() == [[[1, 0, 0, 0, 0], [0, 0, 1, 0, 0]]]
    kk = k[:1].clone()
    kk[0, 1] = INF                                                        # the only score of head 1 is -Inf: (-Inf) - (-Inf)
    assert same(A.contract_probabilities(q, kk, A.SCALE, torch.tensor([0])), torch.tensor([[[NAN], [NAN]]], dtype=torch.float64))
    with pytest.raises(AssertionError):                                   # scores 90 apart are not all-or-nothing
        A.contract_probabilities(q, torch.stack([4 * H[0], 3 * H[0]]), A.SCALE, torch.tensor([1]))


def test_explicit_reference_skips_no_zero():
    p = torch.tensor([[[1.0, 0.0, 1.0]]], dtype=torch.float64)
    v = torch.zeros(3, D)
    v[0, 0], v[2, 0] = 3.0, 4.0
    v[1, 1] = INF                                                         # probability 0 times Inf
    v[1, 2] = NAN
    v[0, 3] = -INF
    v[0, 4], v[2, 4] = INF, -INF
    v[0, 5] = v[2, 5] = bits_to_f32(torch.tensor(0x7F7F0000))
    ref = A.explicit_reference(p, v)
    assert ref[0, 0, :6].tolist()[0] == 3.5 and ref[0, 0, 1].isnan() and ref[0, 0, 2].isnan()
    assert ref[0, 0, 3] == -INF and ref[0, 0, 4].isnan() and ref[0, 0, 5].isfinite() and not ref[0, 0, 6:].any()
    assert A.explicit_reference(p, v, fp32=True)[0, 0, 5] == INF          # the fp32 accumulator overflows
    assert A.explicit_reference(torch.tensor([[[NAN, 1.0, 0.0]]], dtype=torch.float64), v).isnan().all()
    bits, nan = A.expected_bits(ref)
    assert bits[0, 0, 0] == 0x4060 and bits[0, 0, 3] == 0xFF80 and nan[0, 0, :6].tolist() == [False, True, True, False, True, False]


def test_the_float64_softmax_would_give_inf_where_the_contract_gives_nan():
    """Why the expectation never comes from a float64 softmax."""
    c = A.plant(False, "v-unmatched-+inf")
    ln = A.Launch(c.ops)
    soft = ATT.reference(ln.q_cpu, ln.kc_cpu, ln.vc_cpu, ln.table_cpu, ln.ctx_cpu)
    cell = (c.s, slice(c.kv * 4, c.kv * 4 + 4), c.d0)
    assert bool((soft[cell] == INF).all()) and bool(c.reference()[cell].isnan().all())


# ------------------------------------------------------------------------------------------------
# A. the code table
# ------------------------------------------------------------------------------------------------
def test_code_table_holds_every_finite_code_once_plus_the_repeats():
    rows = A.code_rows()
    assert rows.shape == (512, D)
    first = rows[:510].flatten()
    assert first.numel() == 65280 == first.unique().numel()
    finite = ~(((first >> 7) & 0xFF) == 0xFF)
    assert bool(finite.all()) and set(range(1 << 16)) - set(first.tolist()) == set(range(0x7F80, 0x8000)) | set(range(0xFF80, 0x10000))
    assert torch.equal(rows[510], torch.arange(0x0000, 0x0080)) and torch.equal(rows[511], torch.arange(0x8000, 0x8080))
    assert {0x0001, 0x007F, 0x0080, 0x7F7F, 0x8000, 0x8001, 0xFF7F} <= set(first.tolist())
    ctxs, q_lens, targets, _, _, vs = A.code_layout()
    for s in range(A.CODE_S):
        for kv in range(A.CODE_HKV):
            assert torch.equal(bf16_to_bits(vs[s][kv, targets[s][kv]].to(torch.bfloat16)), rows[A.CODE_HKV * s + kv])


def test_code_targets_sit_where_the_kernels_change_path():
    ctxs, q_lens, targets, _, _, _ = A.code_layout()
    assert len(ctxs) == 64 and set(ctxs) == set(A.CODE_CTXS) == {1, 33, 64, 97, 130}
    tg = [(c, n, t) for c, n, ts in zip(ctxs, q_lens, targets) for t in ts]
    assert all(0 <= t <= c - n for c, n, t in tg)                         # at or below the chunk's first position
    assert any(t < T < c for c, n, t in tg)                               # the first block of several
    assert any(t // T == (c - 1) // T > 0 for c, n, t in tg)              # the last block
    assert any(t == c - 1 and c > 1 for c, n, t in tg)                    # the last slot inside ctx
    assert any(t == c - 1 and c % T for c, n, t in tg)                    # ... of a partial block
    assert {(t // T) % 4 for c, n, t in tg} == {0, 1, 2, 3}               # blocks of all four decode waves
    assert any(t // T == 4 for c, n, t in tg)                             # a wave's second block
    assert {n for c, n in zip(ctxs, q_lens) if c > 1} == {1, 3, 9} and all(n == 1 for c, n in zip(ctxs, q_lens) if c == 1)
    assert {(c, n) for c, n in zip(ctxs, q_lens)} >= {(c, n) for c in (33, 64, 97, 130) for n in (1, 3, 9)}
    assert 9 * 16 > PRE.COLUMNS                                           # group 16: a chunk of 9 spans two column tiles
    assert 64 * 8 == 512                                                  # workgroups of a decode launch


@pytest.mark.parametrize("prefill", [False, True])
@pytest.mark.parametrize("group", [1, 4])
def test_code_reference_is_the_code(group, prefill):
    ops = A.code_ops(group, prefill)
    assert ops.R == (sum(A.code_layout()[1]) if prefill else 64) and ops.Hq == 8 * group
    ref = A.reference(ops)
    assert bool(A.exact_in_fp32(ref).all())
    exp, nan = A.expected_bits(ref)
    codes = A.code_expected(ops)
    assert torch.equal(exp | ((codes == 0x8000).long() << 15), codes) and not nan.any()       # -0.0 sums to +0.0


def test_comparison_rejects_a_flushed_subnormal_and_accepts_either_zero():
    ops = A.code_ops(1, False)
    codes = A.code_expected(ops)
    either = (codes & 0x7FFF) == 0
    nan = torch.zeros_like(either)
    assert int(either.sum()) == 4                                         # +0.0 and -0.0, each in a repeated row too
    assert not A.cell_mismatches(codes, codes, nan, either).any()
    assert not A.cell_mismatches(codes ^ (either.long() << 15), codes, nan, either).any()
    sub = (((codes >> 7) & 0xFF) == 0) & ~either
    assert int(sub.sum()) == 4 * 127
    flushed = torch.where(sub, codes & 0x8000, codes)
    assert torch.equal(A.cell_mismatches(flushed, codes, nan, either), sub)
    with pytest.raises(AssertionError, match="508 cells differ"):
        A.assert_cells(flushed, codes, nan, "flushed", either_zero=either)
    wrong_sign = codes.clone()
    wrong_sign[0, 0, 1] ^= 0x8000                                         # only a zero may change its sign
    assert int(A.cell_mismatches(wrong_sign, codes, nan, either).sum()) == 1


# ------------------------------------------------------------------------------------------------
# B. the pair table
# ------------------------------------------------------------------------------------------------
def test_pair_table_holds_ties_carries_subnormal_results_and_the_overflows():
    table = A.pair_table()
    assert table.shape == (2 * 6 * 4 * 3 + 2, 2) and int(table.max()) < 1 << 16
    assert not bf16_is_nan(table).any() and not (((table >> 7) & 0xFF) == 0xFF).any()
    v = bits_to_f32(table << 16).double()
    mean = (v[:, 0] + v[:, 1]) / 2
    over = torch.arange(len(table)) >= len(table) - 2
    assert bool(A.exact_in_fp32(v[:, 0] + v[:, 1])[~over].all()) and bool(A.exact_in_fp32(mean)[~over].all())
    assert bool(((v[:, 0] + v[:, 1])[over].abs() > 3.40283e38).all())     # no fp32 value: the accumulator overflows
    vf = bits_to_f32(table << 16)
    u = A.f32_to_bits((vf[:, 0] + vf[:, 1]) / 2)                          # the sum in fp32: the two overflows are Inf
    assert torch.equal(u[~over], A.f32_to_bits(mean.float())[~over])
    exp = A.bf16_bits_rne(u)
    up = (table[:, 1] == table[:, 0] + 1) & ~over
    assert int(up.sum()) == 48 and bool(((u & 0xFFFF) == 0x8000)[up].all())          # every (v, next) mean is a tie
    assert bool((exp[up] == table[up, 0] + (table[up, 0] & 1)).all())                 # ... that goes to the even code
    carry = up & ((table[:, 0] & 0x7F) == 0x7F)
    assert int(carry.sum()) == 12 and bool((((exp >> 7) & 0xFF) == ((table[:, 0] >> 7) & 0xFF) + 1)[carry].all())
    subnormal = (((exp >> 7) & 0xFF) == 0) & ((exp & 0x7F) != 0)
    assert int(subnormal.sum()) >= 8 and bool((subnormal & up).any())
    assert bool(((exp & 0x7FFF) == 0)[(table[:, 0] ^ table[:, 1]) == 0x8000].all())
    assert exp[over].tolist() == [0x7F80, 0xFF80]


@pytest.mark.parametrize("prefill", [False, True])
def test_pair_reference_is_the_mean_of_the_pair(prefill):
    ops = A.pair_ops(prefill)
    targets, _, _ = A.pair_layout()
    for (ctx, n), tg in zip(zip(A.PAIR_CTXS, A.PAIR_CHUNKS), targets):
        assert all((t // T) % 4 != (u // T) % 4 and max(t, u) <= ctx - n for t, u in tg)
    ref = A.reference(ops, fp32=True)
    exp, nan = A.expected_bits(ref)
    table = A.pair_table()
    v = bits_to_f32(table << 16)
    want = A.bf16_bits_rne(A.f32_to_bits((v[:, 0] + v[:, 1]) / 2))
    entries = A.pair_entries(ops)
    zero = ((v[:, 0] + v[:, 1]) == 0)[entries]                            # (v, -v), (+-0, +-0): the sign is the sum order's
    assert torch.equal(ref == 0, zero) and int(zero[0, 0].sum() + zero[0, 4].sum()) < 256 * 52 // 146 + 52
    assert torch.equal(exp[~zero], want[entries][~zero]) and bool(((exp & 0x7FFF) == 0)[zero].all()) and not nan.any()
    assert set(entries.flatten().tolist()) == set(range(len(table)))      # every entry is in the launch
    assert bool((exp == 0x7F80).any()) and bool((exp == 0xFF80).any())
    # the float64 sum is the same wherever it does not overflow
    exp64, _ = A.expected_bits(A.reference(ops))
    assert torch.equal((exp64 == exp) | zero, entries < len(table) - 2)


# ------------------------------------------------------------------------------------------------
# the split mode of parts A, B and D
# ------------------------------------------------------------------------------------------------
def test_split_counts_cover_empty_splits_and_pairs_within_and_across():
    assert A.CODE_SPLITS == (2, 4) and A.PAIR_SPLITS == (2, 4) and A.SCALE_SPLITS == (3, 4)
    assert A.split_sizes(130, 4) == [2, 2, 1, 0] and A.split_sizes(1, 4) == [1, 0, 0, 0] and A.split_sizes(257, 3) == [3, 3, 3]
    cover = A.split_coverage("codes", 4)
    assert {1} <= set(cover["empty"]) and cover["splits with a target"] == [0, 1, 2, 3]
    assert A.split_coverage("codes", 2)["splits with a target"] == [0, 1]
    for k in A.PAIR_SPLITS:
        cover = A.split_coverage("pairs", k)
        assert cover["within"] >= 2 and cover["across"] >= 2 and cover["within"] + cover["across"] == 8


def test_split_counts_of_the_scale_cases_are_uneven_at_three():
    for part in ("scale 0", "negated", "random"):
        assert A.split_coverage(part, 3)["uneven"] >= 1
        A.split_coverage(part, 4)
    assert A.split_sizes(256, 3) == [3, 3, 2] and A.split_sizes(129, 3) == [2, 2, 1]
    for ops in (A.zero_scale_ops(False), A.negated_scale_ops()):
        assert A.order_free_sums(ops)
    assert not A.order_free_sums(A.softmax_case(False))
    assert A.lonely_target(A.negated_scale_ops())


# ------------------------------------------------------------------------------------------------
# C. planted values
# ------------------------------------------------------------------------------------------------
CASES = [pytest.param(m, n, id=("prefill-" if m else "decode-") + n) for m in (False, True) for n in A.PLANTS[m]]


def test_the_plant_cases_are_the_ones_named():
    for prefill in (False, True):
        names = set(A.PLANTS[prefill])
        assert names >= {f"q-{v}" for v in A.NONFINITE} | {f"k-{b}-block-{v}" for b in ("first", "last") for v in ("nan", "+inf")}
        assert names >= {f"v-{m}-{v}" for m in ("matched", "unmatched") for v in A.NONFINITE}
    assert set(A.PLANTS[True]) - set(A.PLANTS[False]) == {"k-in-chunk-nan", "v-in-chunk-+inf"}
    base = A.plant_base(False)
    assert base.ctxs == ATT.CTX_B and base.group == 4 and base.hkv == 2
    base = A.plant_base(True)
    assert tuple(zip(base.ctxs, base.q_lens)) == PRE.SEQS_B and base.group == 4 and base.hkv == 2


@pytest.mark.parametrize("prefill,name", CASES)
def test_reference_dependants_are_the_predicted_ones(prefill, name):
    c = A.plant(prefill, name)
    base, ref = A.plant_base_reference(prefill), c.reference()
    changed = ~((ref == base) | (ref.isnan() & base.isnan()))
    assert bool(changed.any())
    assert torch.equal(changed, c.dependants), (int(changed.sum()), int(c.dependants.sum()))
    assert bool((ref.isnan() | ref.isinf())[c.dependants].all()) and bool(ref.isfinite()[~c.dependants].all())
    ops, r0, heads = c.ops, c.ops.rows(c.s)[0], A.heads_of(c.ops, c.kv)
    rows = slice(r0, r0 + ops.rows(c.s)[1])
    outside = torch.ones_like(changed)
    outside[rows, heads] = False
    assert not changed[outside].any()                                     # never another sequence or KV head
    if c.tensor == "q":
        r, h, d0 = c.at
        assert int(changed.sum()) == D and bool(ref[r, h].isnan().all()) and bool((ops.ks[c.s][c.kv][:, d0] != 0).any())
        assert heads.start < h < heads.stop - 1                           # both neighbours are heads of the same group
    elif c.tensor == "v":
        assert bool(changed[rows, heads, c.d0].any()) and int(changed.sum()) == int(changed[rows, heads, c.d0].sum())
        p = A.probabilities(A.plant_base(prefill), c.s, c.kv)[:, :, c.t]
        if "unmatched" in name:
            assert not p.any() and bool(ref[c.dependants].isnan().all())
        if "matched" in name and "unmatched" not in name:
            assert bool(p.any())
            want = NAN if c.value != c.value else c.value
            hit = torch.zeros_like(changed)
            hit[rows, heads, c.d0] = p > 0
            assert bool(hit.any()) and same(ref[hit], torch.full_like(ref[hit], want))           # the signed Inf of the mean
            assert bool(ref[c.dependants & ~hit].isnan().all())
    else:
        assert bool(ref[c.dependants].isnan().all())
        per_head = changed[rows, heads].all(-1)
        assert torch.equal(per_head, changed[rows, heads].any(-1))        # whole rows
        if "+inf" in name:                                                # some heads get -Inf: probability 0, unchanged
            attends = ops.rows(c.s)[2] >= c.t
            assert bool(per_head[attends].any()) and not per_head[attends].all()
        if "last-block" in name:
            ctx = ops.ctxs[c.s]
            assert ctx % T and c.t // T == (ctx - 1) // T and c.t < ctx
        if "first-block" in name:
            assert c.t < T
    if prefill:
        n, pos = ops.rows(c.s)[1:]
        before = int((pos < c.t).sum()) if c.tensor != "q" else 0
        assert int(c.uncompared.sum()) == before * ops.group * D and not (c.uncompared & c.dependants).any()
        assert ("in-chunk" in name) == (before > 0)
    else:
        assert not c.uncompared.any()


def test_uncompared_cells_stay_under_the_cap():
    shares = {n: float(A.plant(True, n).uncompared.float().mean()) for n in A.PLANTS[True]}
    assert all(v <= A.UNCOMPARED_CAP for v in shares.values()), shares
    assert sum(v > 0 for v in shares.values()) == 2
    assert not any(A.plant(False, n).uncompared.any() for n in A.PLANTS[False])


def test_comparison_rejects_a_zero_row_a_leaked_nan_and_a_nan_in_the_next_column():
    c = A.plant(False, "k-first-block-nan")
    exp, nan = A.expected_bits(c.reference())
    assert not A.cell_mismatches(torch.where(nan, torch.full_like(exp, 0xFFC1), exp), exp, nan).any()     # any NaN will do
    zero_row = torch.where(nan, torch.zeros_like(exp), exp)               # what `lsum > 0 ? acc / lsum : 0` makes of a NaN
    assert torch.equal(A.cell_mismatches(zero_row, exp, nan), c.dependants)
    with pytest.raises(AssertionError, match="exp=NaN"):
        A.assert_cells(zero_row, exp, nan, "zero row")
    c = A.plant(False, "q-nan")
    exp, nan = A.expected_bits(c.reference())
    r, h, d0 = c.at
    leaked = exp.clone()
    leaked[r, h + 1] = 0x7FC0
    assert int(A.cell_mismatches(leaked, exp, nan).sum()) == D and not A.cell_mismatches(exp, exp, nan)[r, h].any()
    c = A.plant(True, "v-unmatched-nan")
    exp, nan = A.expected_bits(c.reference())
    got = torch.where(nan, torch.full_like(exp, 0x7FC0), exp)
    assert not A.cell_mismatches(got, exp, nan).any()
    next_column = got.clone()
    next_column[:, :, c.d0 + 1] = torch.where(nan[:, :, c.d0], 0x7FC0, got[:, :, c.d0 + 1])
    assert int(A.cell_mismatches(next_column, exp, nan).sum()) == int(nan.sum()) > 0
    # the cells left uncompared take anything, and nothing else does
    c = A.plant(True, "v-in-chunk-+inf")
    exp, nan = A.expected_bits(c.reference())
    junk = torch.where(c.uncompared, torch.full_like(exp, 0x7FC0), exp)
    assert not A.cell_mismatches(torch.where(nan, 0x7FC0, junk), exp, nan, skip=c.uncompared).any()
    assert torch.equal(A.cell_mismatches(torch.where(nan, 0x7FC0, junk), exp, nan), c.uncompared)


# ------------------------------------------------------------------------------------------------
# D. scale
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefill", [False, True])
def test_scale_zero_expectation_rejects_the_default_scale(prefill):
    ops = A.zero_scale_ops(prefill)
    assert bool(ops.q.any()) and all(float(v.abs().max()) <= 4 and torch.equal(v, v.round()) for v in ops.vs if v.numel())
    if not prefill:
        assert ops.ctxs == ATT.CTX_UNIFORM
    exp, nan = A.zero_scale_expected(ops)
    assert not nan.any()
    ln = A.Launch(ops)
    if prefill:
        at = lambda scale: PRE.reference(ln.q_cpu, ln.kc_cpu, ln.vc_cpu, ln.table_cpu, ln.ctx_cpu, ln.q_start_cpu,
                                         scale=scale)[ln.lead:ln.lead + ops.R]
    else:
        at = lambda scale: ATT.reference(ln.q_cpu, ln.kc_cpu, ln.vc_cpu, ln.table_cpu, ln.ctx_cpu, scale=scale)
    # the float64 softmax at scale 0 is the same mean wherever the exact sum is not 0
    soft0, _ = A.expected_bits(at(0.0))
    assert torch.equal(soft0[(exp & 0x7FFF) != 0], exp[(exp & 0x7FFF) != 0])
    baked, _ = A.expected_bits(at(A.SCALE))                               # a kernel that ignores its scale argument
    wrong = A.cell_mismatches(baked, exp, nan)
    assert float(wrong.float().mean()) > 0.5
    with pytest.raises(AssertionError):
        A.assert_cells(baked, exp, nan, "default scale")


def test_negated_scale_expectation_is_the_mean_of_the_others():
    ops = A.negated_scale_ops()
    assert all(c - 1 == 1 << (c - 1).bit_length() - 1 for c in ops.ctxs)              # 2^k + 1
    ref = A.reference(ops, scale=-A.SCALE)
    assert bool(A.exact_in_fp32(ref).all())
    for s, ctx in enumerate(ops.ctxs):
        for kv in range(ops.hkv):
            p = A.probabilities(ops, s, kv, -A.SCALE)[0]                  # [group, ctx]
            assert bool((p.sum(-1) == ctx - 1).all()) and p.max() == 1 and p.min() == 0
            want = (p[:, :, None] * ops.vs[s][kv].double()[None]).sum(1) / (ctx - 1)
            assert torch.equal(ref[s, A.heads_of(ops, kv)], want)
    plus, _ = A.expected_bits(A.reference(ops, scale=A.SCALE))            # the sign of the scale matters everywhere
    minus, _ = A.expected_bits(ref)
    assert float((plus != minus).float().mean()) > 0.5


@pytest.mark.parametrize("prefill", [False, True])
def test_random_regime_scores_stay_inside_the_bound_derivation(prefill):
    ops = A.softmax_case(prefill)
    worst = [A.max_abs_score(ops, s) for s in A.RANDOM_SCALES]
    print(f"max|scale * q . k| at scales 2^-4, 2^-3 ({'prefill' if prefill else 'decode'}): {worst}")
    assert all(w <= A.SCORE_CAP for w in worst) and worst[1] == 2 * worst[0]
    assert worst[1] > A.max_abs_score(ops, A.SCALE)                       # a larger scale than the default's
