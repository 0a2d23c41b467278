"""Exact-arithmetic, guarded-buffer tests of the MoE combine -- loadgen.moe_combine (run with `-m gpu` on an MI355X),
with the guard helpers and sentinels of test_gpu_kernels_exact.py.

Shapes: T in {1, 5, 70} x D in {8, 2048, 2056} x k in {1, 2, 8}, routed over 16 experts by a seeded draw and laid out
by loadgen.moe_align_reference.  D = 8 is one 16-byte chunk per token, 2048 a whole workgroup per token (256 chunks),
2056 one chunk more, so workgroups straddle tokens; T = 70 with k = 8 names 560 rows of y.

Every launch runs guarded: y is a window (column offset 8, row stride D + 24) of a NaN-filled allocation, and every
row of it that slot_pos does not name -- the pad rows, the unused tiles -- holds NaN too: a read of any of them would
show; out is a window (column offset 8, row stride D + 16) of a SENT16-filled allocation compared bitwise, guards
included.

Value regimes:

  dyadic  weights drawn from {0, -0, +-1/4, +-1/2, +-1, +-2}, y integers of [-8, 8] with both zeros: every product
          and every partial sum is a multiple of 1/4 below 2^8, exact in fp32, so the chain of fmas equals the float64
          chain acc = acc + w y from acc = +0.0 bit for bit -- the signs of zero included: +0.0 + (-0.0) and x + (-x)
          are +0.0 under round-to-nearest, so every zero output is 0x0000.
  true    randn y, softmax weights: against an fp32 fma emulation -- acc = fp32(w y + acc) with the product and the sum
          formed in float64, where w y (24 x 8 significant bits) is exact -- rounded to bf16 once; bitwise.
"""
import functools

import pytest
import torch

from test_gpu_kernels_exact import NAN, SENT16, guarded_output, guards_intact

pytestmark = pytest.mark.gpu

BF, I32 = torch.bfloat16, torch.int32
TS, DS, KS = (1, 5, 70), (8, 2048, 2056), (1, 2, 8)
E = 16
R0, C0 = 2, 8
DYADIC = (0.0, -0.0, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0)


@pytest.fixture(scope="module")
def L():
    from k8s_gpu_scheduler_amd import _native
    from k8s_gpu_scheduler_amd.ops import loadgen
    _native.hip(required=True)
    return loadgen


@functools.lru_cache(maxsize=None)
def routing(T, k):
    """(sorted_ids, slot_pos) on the CPU for T tokens with k distinct experts each."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    g = torch.Generator().manual_seed(100 * T + k)
    ids = torch.rand(T, E, generator=g).argsort(dim=1)[:, :k].to(I32)
    s, _, _, p = loadgen.moe_align_reference(ids, E)
    return s, p


def operands(regime, T, D, k, seed):
    """(y [P_max, D] bf16 with NaN in every row no slot names, topk_w [T, k] fp32) on the CPU."""
    s, p = routing(T, k)
    g = torch.Generator().manual_seed(seed)
    if regime == "dyadic":
        y = torch.randint(-8, 9, (len(s), D), generator=g).float()
        y[torch.rand(len(s), D, generator=g) < 0.1] = -0.0
        w = torch.tensor(DYADIC)[torch.randint(len(DYADIC), (T, k), generator=g)]
    else:
        y = torch.randn(len(s), D, generator=g)
        w = torch.softmax(torch.randn(T, k, generator=g), dim=1)
    y[s >= T * k] = NAN
    return y.to(BF), w.float().contiguous()


def chain(y, p, w, fp32):
    """acc = +0.0; acc = w_j y_j + acc for j = 0 .. k - 1, in float64 -- rounded to fp32 after every step when fp32
    (the fused multiply-add: w y is exact in float64) --, then rounded to bf16 once."""
    T, k = w.shape
    acc = torch.zeros(T, y.shape[1], dtype=torch.float64)
    rows = p.view(T, k).long()
    for j in range(k):
        acc = w[:, j].double()[:, None] * y[rows[:, j]].double() + acc
        if fp32:
            acc = acc.float().double()
    if not fp32:
        assert torch.equal(acc.float().double(), acc)
    return acc.float().to(BF)


def run(L, y, p, w):
    T, k = w.shape
    P, D = y.shape
    big = torch.full((R0 + P + 3, D + 24), NAN, dtype=BF, device="cuda")
    gy = big[R0:R0 + P, C0:C0 + D]
    gy.copy_(y)
    raw, out = guarded_output(T, D, D + 16, C0, "cuda")
    res = L.moe_combine(gy, p.cuda(), w.cuda(), out=out)
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr()
    assert guards_intact(raw, (slice(R0, R0 + T), slice(C0, C0 + D)), SENT16)
    return raw[R0:R0 + T, C0:C0 + D].cpu()


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("regime", ("dyadic", "true"))
def test_bit_exact(L, regime, D):
    for T in TS:
        for k in KS:
            y, w = operands(regime, T, D, k, 1000 * T + D + k)
            _, p = routing(T, k)
            exp = chain(y, p, w, fp32=regime == "true")
            got = run(L, y, p, w)
            assert not bool(exp.isnan().any())
            bad = (got != exp.view(torch.int16)).nonzero()
            assert len(bad) == 0, (T, k, len(bad), bad[:4].tolist())
            if regime == "dyadic":
                assert int((exp == 0).sum()) > 0 or D == 8
                assert not bool((got == -32768).any())                                  # no -0.0: every zero is 0x0000


def test_a_planted_nan_stays_in_its_cell(L):
    T, D, k = 70, 2056, 8
    y, w = operands("true", T, D, k, 42)
    s, p = routing(T, k)
    cells = [(int(p[0]), 0), (int(p[T * k - 1]), D - 1), (int(p[300]), 1031)]            # rows of three named slots
    for r, c in cells:
        y[r, c] = NAN
    w[5, 3] = NAN                                                                      # a NaN weight: its whole token
    w[9, 2] = 0.0
    y[int(p[9 * k + 2]), 17] = float("inf")                                            # 0 * Inf is NaN: nothing is skipped
    got = run(L, y, p, w).view(BF)
    want = torch.zeros(T, D, dtype=torch.bool)
    for r, c in cells:
        want[int(s[r]) // k, c] = True
    want[5, :] = True
    want[9, 17] = True
    assert torch.equal(got.isnan(), want)
    clean = chain(y, p, w, fp32=True)
    assert torch.equal(got[~want].view(torch.int16), clean[~want].view(torch.int16))


def test_two_launches_are_identical_and_no_token_launches_nothing(L):
    y, w = operands("true", 70, 2048, 8, 1)
    _, p = routing(70, 8)
    assert torch.equal(run(L, y, p, w), run(L, y, p, w))
    out = L.moe_combine(torch.zeros(0, 16, dtype=BF, device="cuda"), torch.zeros(0, dtype=I32, device="cuda"),
                        torch.zeros(0, 2, device="cuda"))
    assert out.shape == (0, 16)
