"""Exact, guarded-buffer tests of MoE routing -- loadgen.moe_route: the top-k + softmax launch and the align launch
(run with `-m gpu` on an MI355X), in the style of test_gpu_swiglu_exact.py and with the guard helpers of
test_gpu_kernels_exact.py.

Every launch runs guarded: the logits are a window (column offset 8, row stride E + 16) of a NaN-filled allocation,
each of the six outputs a window of a sentinel-filled int32 allocation (0x5A5A5A5A: garbage as ids, offsets and
weights alike) that is compared afterwards, guards included.

Shapes: T in {1, 3, 64, 65, 200} x E in {8, 64, 128, 256} x k in {1, 2, 8}.  T = 64 and 65 put one and two 64-slot
groups into the align kernel at k = 1, T = 200 with k = 8 gives every one of its 16 waves more than one group, T = 3
leaves most lanes of the only group idle.

What is compared, and how:

  ids, layout  BITWISE.  topk_ids against loadgen.moe_topk_reference (a stable descending sort: value descending,
               index ascending, +0 == -0), the four layout arrays against loadgen.moe_align_reference of the GPU's
               own ids, and the layout's defining properties again through test_moe_cpu.check_layout.  Regimes:
               "ties" (multiples of 1/4 in [-2, 2): 16 values, so almost every threshold is tied), "equal" (a row of
               one value), "inf" (+-Inf planted), "one" (everything routed to one expert: c_e = T crosses 64 and
               65), and the count vector (0, 1, 63, 64, 65, 7) over six experts at T = 200, k = 1.
  weights      against the float64 softmax over the selected logits, e_j / sum e with e_j = 2^((l_j - l_0) log2 e).
               The bound, from the contract (u = 2^-24, d = max_j |l_j - l_0| <= 32, asserted):
                 - the subtraction rounds once, the constant 1.44269504f is log2 e rounded once and the product
                   rounds once: the exponent is d_j log2 e (1 + 3 u) to first order, and 2^x turns an absolute
                   exponent error a into a relative error a ln 2: 3 u |d_j| (ln 2 * log2 e = 1);
                 - v_exp_f32 is documented at 1 ulp: 2 u relative;
                 so every e_j is within eps_e = 3 u d + 2 u of its value;
                 - the k-term sum of positive terms adds (k - 1) u to their common eps_e;
                 - the division adds u.
               |w - ref| <= (2 eps_e + k u) (1 + 2^-10) ref = ((6 d + 4 + k) u) (1 + 2^-10) ref, the last factor
               for the second-order terms.  For d = 32, k = 8: 204 u = 1.2e-5.  The measured maximum of error /
               bound is printed (MEASURED below).
  exact        the contract's consequences, bitwise: k = 1 gives 1.0f; a row of equal logits gives exactly 1 / k for
               k in {2, 4, 8} (e_j = exp2(0) = 1, the sum k, the quotient a power of two).
  NaN rows     ids in range and pairwise distinct, the layout consistent with them, every other row as the reference.
"""
import pytest
import torch

from test_gpu_kernels_exact import NAN, SENT32, guarded_input, guards_intact
from test_moe_cpu import check_layout

pytestmark = pytest.mark.gpu

# MEASURED on an MI355X (printed by test_weights_within_the_derived_bound):
MEASURED = """
  weights, max |w - ref| / bound over E in {8, 64, 128, 256}, T in {3, 65, 200}, k in {1, 2, 8}: 0.2173.
  The module: 22 tests in 4 s.
"""

BF, I32 = torch.bfloat16, torch.int32
TS, ES, KS = (1, 3, 64, 65, 200), (8, 64, 128, 256), (1, 2, 8)
REGIMES = ("ties", "equal", "inf", "one")
U = 2.0 ** -24
INF = float("inf")
PAD = 8                                                                # guard cells before and after every output


@pytest.fixture(scope="module")
def L():
    from k8s_gpu_scheduler_amd import _native
    from k8s_gpu_scheduler_amd.ops import loadgen
    _native.hip(required=True)
    return loadgen


def logits_for(regime, T, E, k, seed):
    g = torch.Generator().manual_seed(seed)
    if regime == "ties":
        x = torch.randint(-8, 8, (T, E), generator=g).float() / 4
    elif regime == "equal":
        x = (torch.randint(-8, 8, (T, 1), generator=g).float() / 4).expand(T, E).clone()
        x[::2] = torch.where(torch.rand(T, E, generator=g)[::2] < 0.5, 0.0, -0.0)      # both zeros: one value
    elif regime == "inf":
        x = torch.randn(T, E, generator=g)
        r = torch.rand(T, E, generator=g)
        x[r < 0.1] = -INF
        x[r > 0.95] = INF
        x[:, 0] = 0.5                                                                  # the maximum is never -Inf
    elif regime == "one":
        x = torch.zeros(T, E)
        x[:, E - 3] = 10.0                                                             # c_e = T for one expert
    else:
        x = 3 * torch.randn(T, E, generator=g)
    return x.to(BF)


def guarded_outputs(T, E, k, L):
    """{name: (raw, view)}: every output a window of a sentinel-filled int32 allocation."""
    tiles = L.moe_max_tiles(T, k, E)
    sizes = {"topk_ids": T * k, "topk_w": T * k, "sorted_ids": 64 * tiles, "tile_expert": tiles, "expert_offsets": E + 1,
             "slot_pos": T * k}
    out = {}
    for nm, n in sizes.items():
        raw = torch.full((PAD + n + PAD,), SENT32, dtype=I32, device="cuda")
        view = raw[PAD:PAD + n]
        if nm == "topk_w":
            view = view.view(torch.float32)
        if nm in ("topk_ids", "topk_w"):
            view = view.view(T, k)
        out[nm] = (raw, view)
    return out


def route(L, logits_host, k, **kw):
    """One guarded launch; returns the six outputs on the CPU and asserts the guards."""
    T, E = logits_host.shape
    lg = guarded_input(logits_host.cuda(), E + 16)
    outs = guarded_outputs(T, E, k, L)
    res = L.moe_route(lg, k, **{nm: v for nm, (_, v) in outs.items()}, **kw)
    torch.cuda.synchronize()
    assert all(r.data_ptr() == outs[nm][1].data_ptr() for r, nm in zip(res, outs))
    for nm, (raw, v) in outs.items():
        assert guards_intact(raw, slice(PAD, PAD + v.numel()), SENT32), nm
    return tuple(r.cpu() for r in res)


def compare_exact(L, logits_host, k, got):
    ids, w, s, t, off, p = got
    E = logits_host.shape[1]
    ref_ids, _ = L.moe_topk_reference(logits_host, k)
    assert torch.equal(ids, ref_ids), (ids != ref_ids).nonzero()[:4]
    for nm, a, b in zip(("sorted_ids", "tile_expert", "expert_offsets", "slot_pos"), (s, t, off, p), L.moe_align_reference(ids, E)):
        assert torch.equal(a, b), nm
    check_layout(ids, E, s, t, off, p)


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("regime", REGIMES)
def test_ids_and_layout_bitwise(L, regime, E):
    for T in TS:
        for k in KS:
            lg = logits_for(regime, T, E, k, 1000 * T + 10 * E + k)
            got = route(L, lg, k)
            compare_exact(L, lg, k, got)
            if regime == "one":
                assert int((got[0] == E - 3).sum()) == T and int(got[4][E - 2] - got[4][E - 3]) == 64 * -(-T // 64)


def test_the_count_vector_0_1_63_64_65(L):
    counts = [0, 1, 63, 64, 65, 7]                                     # 200 tokens, k = 1
    expert = torch.cat([torch.full((c,), e) for e, c in enumerate(counts)])
    expert = expert[torch.randperm(200, generator=torch.Generator().manual_seed(7))]
    for E in (8, 128):
        lg = torch.randint(-8, 8, (200, E), generator=torch.Generator().manual_seed(E)).float() / 4
        lg[torch.arange(200), expert] = 5.0
        lg = lg.to(BF)
        got = route(L, lg, 1)
        compare_exact(L, lg, 1, got)
        assert torch.equal(got[0].flatten().long(), expert)
        assert got[4][:7].tolist() == [0, 0, 64, 128, 192, 320, 384] and got[3][:7].tolist() == [1, 2, 3, 4, 4, 5, -1]


def test_two_launches_and_a_replay_into_the_same_buffers_are_identical(L):
    lg_host = logits_for("ties", 200, 128, 8, 5)
    lg = lg_host.cuda()
    first = L.moe_route(lg, 8)
    second = L.moe_route(lg, 8)
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(I32), b.view(I32)) for a, b in zip(first, second))
    keep = [x.clone() for x in first]
    names = ("topk_ids", "topk_w", "sorted_ids", "tile_expert", "expert_offsets", "slot_pos")
    L.moe_route(lg, 8, **dict(zip(names, first)), check=False)          # over its own earlier result
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(I32), b.view(I32)) for a, b in zip(first, keep))


def test_no_tokens(L):
    got = route(L, torch.zeros(0, 16, dtype=BF), 2)
    assert [x.numel() for x in got] == [0, 0, 0, 0, 17, 0] and got[4].tolist() == [0] * 17


def weight_bound(l_sel, k):
    """The docstring's bound per row, relative to the reference weight."""
    d = (l_sel - l_sel[:, :1]).abs().max(dim=1).values
    assert bool((d <= 32).all())
    return ((6 * d + 4 + k) * U * (1 + 2.0 ** -10))[:, None]


def test_weights_within_the_derived_bound(L):
    worst = 0.0
    for E in ES:
        for T in (3, 65, 200):
            for k in KS:
                g = torch.Generator().manual_seed(77 * E + T + k)
                lg = (3 * torch.randn(T, E, generator=g)).clamp(-15, 15).to(BF)
                lg[::7] = (torch.randint(-64, 65, (T, E), generator=g).float() / 4)[::7].to(BF)     # spreads up to 32
                ids, w, *_ = route(L, lg, k)
                compare_exact(L, lg, k, (ids, w) + tuple(_))
                l_sel = lg.double().gather(1, ids.long())
                e = torch.exp2((l_sel - l_sel[:, :1]) * 1.4426950408889634)
                ref = e / e.sum(dim=1, keepdim=True)
                ratio = ((w.double() - ref).abs() / (weight_bound(l_sel, k) * ref)).max().item()
                worst = max(worst, ratio)
                assert ratio <= 1.0, (E, T, k, ratio)
    print(f"moe_route weights: max |w - ref| / bound = {worst:.4f}")


def test_the_exact_consequences(L):
    for E in ES:
        lg = logits_for("ties", 65, E, 1, E)
        ids, w, *_ = route(L, lg, 1)
        assert torch.equal(w, torch.ones(65, 1))                                       # k = 1: exactly 1.0
        for k in (2, 4, 8):
            eq = logits_for("equal", 65, E, k, E + k)
            ids, w, *_ = route(L, eq, k)
            assert torch.equal(ids, torch.arange(k, dtype=I32).expand(65, k))
            assert torch.equal(w, torch.full((65, k), 1.0 / k))                         # bitwise: 1 / k is a power of two


def test_nan_rows_keep_everything_in_range(L):
    for E, k in ((8, 8), (64, 2), (256, 8), (128, 1)):
        T = 65
        lg = logits_for("normal", T, E, k, 31 * E + k)
        clean = lg.clone()
        nan_rows = [0, 7, 33, 64]
        lg[0, :] = NAN
        lg[7, E // 2] = NAN
        lg[33, ::3] = -NAN
        lg[64, 0] = NAN
        lg[12, :] = -INF                                                               # maximum -Inf: weights unspecified
        ids, w, s, t, off, p = route(L, lg, k)
        assert bool(((ids >= 0) & (ids < E)).all())
        assert all(len(set(r)) == k for r in ids.tolist())                             # k distinct ids on every row
        for nm, a, b in zip(("sorted_ids", "tile_expert", "expert_offsets", "slot_pos"), (s, t, off, p), L.moe_align_reference(ids, E)):
            assert torch.equal(a, b), nm
        check_layout(ids, E, s, t, off, p)
        others = [r for r in range(T) if r not in nan_rows and r != 12]
        ref_ids, ref_w = L.moe_topk_reference(clean, k)
        assert torch.equal(ids[others], ref_ids[others])
        l_sel = clean.double().gather(1, ref_ids.long())[others]
        assert bool(((w[others].double() - ref_w[others].double()).abs()
                     <= (weight_bound(l_sel, k) + U) * ref_w[others].double()).all())    # + u: ref_w is rounded to fp32
        assert ids[12].tolist() == list(range(k))                                      # all -Inf: ties to the lowest indices
