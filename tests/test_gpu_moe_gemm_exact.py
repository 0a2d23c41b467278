"""Exact-arithmetic, guarded-buffer tests of the grouped expert GEMM -- loadgen.moe_gemm (run with `-m gpu` on an
MI355X), in the style of test_gpu_kernels_exact.py, whose guard helpers and sentinels are used.

The layout: 267 slots over 7 experts with the counts (0, 1, 64, 65, 130, 0, 7) -- an empty expert first and in the
middle, one row, exactly one tile, one row into a second tile, two tiles and two rows, a short tile -- as 89 tokens
with top-3 (gather_div = 3, A the [89, K] token rows) and as the sorted intermediate read in place (gather_div = 0, A
[P_max, K]).  moe_max_tiles(89, 3, 7) = 11 tiles, 8 of them used: the last three are unused tiles whose rows must
keep the sentinel.  N in {64, 128, 192, 256} takes both block widths (BN = 128 for 128 and 256), with one, two and
three column tiles; K in {64, 128, 192} is one, two and three K tiles (fewer than, as many as and more than the
tiles the pipeline has in flight before its loop).

Every launch runs guarded: A is a window (column offset 8, row stride K + 72) of a NaN-filled allocation -- and in the
in-place mode its pad rows and the rows of its unused tiles hold NaN themselves: nothing may read them --, W a window
[1:, 1:N + 1, 8:8 + K] of a NaN-filled [E + 1, N + 3, K + 16] allocation (row and expert strides that are no multiple
of N or K), out a window (column offset 8, row stride N + 24) of a SENT16-filled allocation that is compared WHOLE:
the valid rows of used tiles against the expectation, their pad rows against 0x0000, the rows of unused tiles and all
guards against the sentinel.

Value regimes:

  integer  A holds integers of [-64, 64], W integers of [-2, 2] times 2^-(e % 4) for expert e: every product and every
           partial sum is an integer multiple of 2^-3 below 2^15, exact in fp32 in any order, so the output is the
           bf16 rounding (nearest even; many values need it, asserted) of the float64 product, bit for bit.
  true     randn A and W / 8: |out - ref| <= 2^-8 |ref| + (1 + 2^-8) K 2^-23 sum_i |a_i w_i| against the float64
           product of the bf16 operands.  The products of two bf16 are exact in fp32; an fp32 accumulation of K
           terms in any order, rounding to nearest or truncating (the MFMA's internal adder is not documented),
           is within K 2^-23 sum |a_i w_i| of the exact sum; the one bf16 rounding (8 significant bits, to nearest:
           a unit roundoff of 2^-8) adds 2^-8 of what it rounds.
           The measured maximum of error / bound is printed (MEASURED below).
"""
import functools

import pytest
import torch

from test_gpu_kernels_exact import NAN, SENT16, guards_intact

pytestmark = pytest.mark.gpu

# MEASURED on an MI355X (printed by test_true_regime_within_the_derived_bound):
MEASURED = """
  true regime, max |out - ref| / bound over the five (N, K, mode) cases: 0.9905 -- the bf16 rounding's share alone.
  Every integer-regime, permutation, shared-matrix and all-sentinel output bit-exact.  The module: 14 tests in 3 s.
"""

BF, I32 = torch.bfloat16, torch.int32
COUNTS = (0, 1, 64, 65, 130, 0, 7)
E, T, TOP_K = len(COUNTS), 89, 3
N_SLOTS = T * TOP_K
NS, KS = (64, 128, 192, 256), (64, 128, 192)
R0, C0 = 2, 8


@pytest.fixture(scope="module")
def L():
    from k8s_gpu_scheduler_amd import _native
    from k8s_gpu_scheduler_amd.ops import loadgen
    _native.hip(required=True)
    return loadgen


@functools.lru_cache(maxsize=None)
def layout(seed=0):
    """(ids [T, k], sorted_ids, tile_expert, expert_offsets, slot_pos) on the CPU: the counts dealt to the slots by a
    seeded permutation."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    assert sum(COUNTS) == N_SLOTS
    expert = torch.cat([torch.full((c,), e) for e, c in enumerate(COUNTS)])
    ids = expert[torch.randperm(N_SLOTS, generator=torch.Generator().manual_seed(seed))].view(T, TOP_K).to(I32)
    s, t, off, p = loadgen.moe_align_reference(ids, E)
    assert t.tolist() == [1, 2, 3, 3, 4, 4, 4, 6, -1, -1, -1]
    return ids, s, t, off, p


def operands(regime, N, K, rows_a, seed):
    """(a [rows_a, K], w [E, N, K]) bf16 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    if regime == "integer":
        a = torch.randint(-64, 65, (rows_a, K), generator=g).float()
        w = torch.randint(-2, 3, (E, N, K), generator=g).float() * (2.0 ** -(torch.arange(E) % 4).float())[:, None, None]
    else:
        a = torch.randn(rows_a, K, generator=g)
        w = torch.randn(E, N, K, generator=g) / 8
    return a.to(BF), w.to(BF)


def guarded_a(a, hide_rows=None):
    """a as a window of a NaN-filled allocation; hide_rows (a bool mask) are set to NaN inside the window too."""
    rows, K = a.shape
    big = torch.full((R0 + rows + 3, K + 72), NAN, dtype=BF, device="cuda")
    view = big[R0:R0 + rows, C0:C0 + K]
    view.copy_(a)
    if hide_rows is not None:
        view[hide_rows.cuda()] = NAN
    return view


def guarded_w(w):
    n_e, N, K = w.shape
    big = torch.full((n_e + 1, N + 3, K + 16), NAN, dtype=BF, device="cuda")
    view = big[1:, 1:N + 1, 8:8 + K]
    view.copy_(w)
    assert view.stride(0) % N and view.stride(1) != K
    return view


def guarded_out(P, N):
    raw = torch.full((R0 + P + 3, N + 24), SENT16, dtype=torch.int16, device="cuda")
    return raw, raw.view(BF)[R0:R0 + P, C0:C0 + N]


def source_rows(s, gather_div):
    """(valid mask, source row of a) per row of the layout."""
    valid = s < N_SLOTS
    src = (s // gather_div if gather_div else torch.arange(len(s), dtype=I32)).long()
    return valid, torch.where(valid, src, torch.zeros_like(src))


def expected_raw(a, w, s, t, gather_div, N):
    """(the int16 image of the whole out window, the float64 reference, sum |a_i w_i|) -- valid rows of used tiles
    the bf16 rounding of the float64 product, their pad rows 0x0000, unused tiles the sentinel."""
    P = len(s)
    valid, src = source_rows(s, gather_div)
    e_row = t.long().repeat_interleave(64)
    used = e_row >= 0
    ref = torch.zeros(P, N, dtype=torch.float64)
    mag = torch.zeros(P, N, dtype=torch.float64)
    for e in range(E):
        rows = (valid & (e_row == e)).nonzero().flatten()
        if len(rows):
            ar, we = a[src[rows]].double(), w[e].double()
            ref[rows] = ar @ we.T
            mag[rows] = ar.abs() @ we.abs().T
    img = torch.full((P, N), SENT16, dtype=torch.int16)
    img[used] = 0
    img[valid] = ref[valid].float().to(BF).view(torch.int16)
    return img, ref, mag, valid


def run(L, regime, N, K, gather_div, seed, lay=None, check=True):
    ids, s, t, off, p = lay or layout()
    P = len(s)
    valid, _ = source_rows(s, gather_div)
    a, w = operands(regime, N, K, T if gather_div else P, seed)
    ga = guarded_a(a, None if gather_div else ~valid)               # in place: pad rows and unused tiles hold NaN
    raw, out = guarded_out(P, N)
    res = L.moe_gemm(ga, guarded_w(w), s.cuda(), t.cuda(), N_SLOTS, gather_div=gather_div, out=out, check=check)
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr()
    assert guards_intact(raw, (slice(R0, R0 + P), slice(C0, C0 + N)), SENT16)
    return raw[R0:R0 + P, C0:C0 + N].cpu(), a, w, s, t, p


@pytest.mark.parametrize("gather_div", (TOP_K, 0))
@pytest.mark.parametrize("N", NS)
def test_integer_regime_bit_exact(L, N, gather_div):
    for K in KS:
        got, a, w, s, t, _ = run(L, "integer", N, K, gather_div, 100 * N + K)
        img, ref, _, valid = expected_raw(a, w, s, t, gather_div, N)
        assert torch.equal(ref.float().double(), ref)                                   # exact in fp32
        assert int((ref[valid].float().to(BF).double() != ref[valid]).sum()) > 0        # some outputs need the rounding
        bad = (got != img).nonzero()
        assert len(bad) == 0, (K, len(bad), bad[:4].tolist())
        assert int((got[64 * 8:] == SENT16).all()) and bool((got[1:64] == 0).all())     # unused tiles; expert 1's 63 pad rows


def test_permuting_the_tokens_moves_rows_and_changes_no_value(L):
    N, K = 192, 192
    ids, s, t, off, p = layout()
    got, a, w, *_ = run(L, "true", N, K, TOP_K, 5)
    perm = torch.randperm(T, generator=torch.Generator().manual_seed(11))
    from k8s_gpu_scheduler_amd.ops import loadgen
    ids2 = ids[perm]
    s2, t2, off2, p2 = loadgen.moe_align_reference(ids2, E)
    raw, out = guarded_out(len(s2), N)
    L.moe_gemm(guarded_a(a[perm]), guarded_w(w), s2.cuda(), t2.cuda(), N_SLOTS, gather_div=TOP_K, out=out)
    torch.cuda.synchronize()
    got2 = raw[R0:R0 + len(s2), C0:C0 + N].cpu()
    assert torch.equal(t, t2) and not torch.equal(s, s2)
    # token perm[i] is token i of the second run: the row of its j-th slot holds the same bits in both
    rows1 = p.view(T, TOP_K)[perm].flatten().long()
    rows2 = p2.flatten().long()
    assert not torch.equal(rows1 % 64, rows2 % 64)                                      # at other places of their tiles
    assert torch.equal(got[rows1], got2[rows2])


def test_true_regime_within_the_derived_bound(L):
    worst = 0.0
    for N, K, gather_div in ((64, 64, TOP_K), (128, 192, 0), (192, 128, TOP_K), (256, 192, TOP_K), (256, 64, 0)):
        got, a, w, s, t, _ = run(L, "true", N, K, gather_div, 7 * N + K, check=False)
        img, ref, mag, valid = expected_raw(a, w, s, t, gather_div, N)
        assert torch.equal(got[~valid], img[~valid])                                    # pad rows, unused tiles
        out = got.view(BF).double()[valid]
        bound = 2.0 ** -8 * ref[valid].abs() + (1 + 2.0 ** -8) * K * 2.0 ** -23 * mag[valid]
        ratio = ((out - ref[valid]).abs() / bound).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, (N, K, gather_div, ratio)
    print(f"moe_gemm true regime: max |out - ref| / bound = {worst:.4f}")


def test_two_launches_are_identical(L):
    a = run(L, "true", 256, 192, TOP_K, 3)[0]
    b = run(L, "true", 256, 192, TOP_K, 3)[0]
    assert torch.equal(a, b)


def test_an_all_sentinel_layout_writes_nothing(L):
    tiles = 11
    s = torch.full((64 * tiles,), N_SLOTS, dtype=I32)
    t = torch.full((tiles,), -1, dtype=I32)
    lay = (None, s, t, None, None)
    for gather_div in (TOP_K, 0):
        got, *_ = run(L, "integer", 128, 64, gather_div, 1, lay=lay)
        assert bool((got == SENT16).all())


def test_a_shared_weight_matrix_and_one_expert(L):
    """Expert stride 0 (one matrix for every expert) is a legal 'arbitrary expert stride'."""
    ids, s, t, off, p = layout()
    a, w = operands("integer", 128, 128, T, 9)
    raw, out = guarded_out(len(s), 128)
    L.moe_gemm(guarded_a(a), guarded_w(w)[2:3].expand(E, 128, 128), s.cuda(), t.cuda(), N_SLOTS, gather_div=TOP_K, out=out)
    torch.cuda.synchronize()
    img, *_ = expected_raw(a, w[2:3].expand(E, 128, 128), s, t, TOP_K, 128)
    assert torch.equal(raw[R0:R0 + len(s), C0:C0 + 128].cpu(), img)


def test_the_device_check(L):
    ids, s, t, off, p = layout()
    a, w = operands("integer", 64, 64, T, 2)
    a, w, P = a.cuda(), w.cuda(), len(s)
    out = torch.zeros(P, 64, dtype=BF, device="cuda")

    def call(s_, t_, n=N_SLOTS, div=TOP_K, a_=a):
        return L.moe_gemm(a_, w, s_.cuda(), t_.cuda(), n, gather_div=div, out=out)

    bad_t = t.clone()
    bad_t[2] = E
    with pytest.raises(ValueError, match="tile_expert entry is outside"):
        call(s, bad_t)
    bad_t[2] = -2
    with pytest.raises(ValueError, match="tile_expert entry is outside"):
        call(s, bad_t)
    for v in (-1, N_SLOTS + 1):
        bad_s = s.clone()
        bad_s[70] = v
        with pytest.raises(ValueError, match="sorted_ids entry is outside"):
            call(bad_s, t)
    with pytest.raises(ValueError, match="source row is past the 88 rows"):
        call(s, t, a_=a[:88])
    with pytest.raises(ValueError, match="source row is past"):                        # in place, a shorter than the used tiles
        call(s, t, div=0, a_=torch.zeros(64 * 7, 64, dtype=BF, device="cuda"))
    call(s, t, div=0, a_=torch.zeros(64 * 8, 64, dtype=BF, device="cuda"))              # the used tiles alone suffice
    torch.cuda.synchronize()
    assert not bool(out.any())
