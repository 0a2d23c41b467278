"""CPU tests of what test_gpu_moe_edges.py and test_gpu_mx_edges.py rely on (no GPU): that the ring-wrap operands make
a stale or an early K tile visible in every tile of the output, that the generalised expectation is G.expected_raw on
G's layout and carries IEEE semantics for planted values, and that the routing cases at the limits are what their
names say."""
import pytest
import torch

import test_gpu_moe_edges as ED
import test_gpu_moe_gemm_exact as G
from test_gpu_kernels_exact import SENT16
from test_moe_cpu import check_layout

BF = torch.bfloat16


def tiles_that_differ(img, other):
    """bool [row tiles, 64-column tiles]: where the two int16 images differ in at least one cell."""
    P, N = img.shape
    return (img != other).view(P // 64, 64, N // 64, 64).any(dim=3).any(dim=1)


@pytest.mark.parametrize("gather_div", (G.TOP_K, 0))
@pytest.mark.parametrize("N", ED.RING_NS)
@pytest.mark.parametrize("K", ED.RING_KS)
def test_a_stale_or_early_k_tile_changes_every_used_tile(K, N, gather_div):
    """K tile t read from the ring slot before its refill landed is tile t - 3 (t >= 3); read one stage ahead it is tile
    t + 1 (t < nt - 1).  Either must change at least one cell of every used 64-row tile x every 64-column tile (so of
    every BN = 64 and BN = 128 workgroup): a workgroup that did it cannot pass test_ring_wrap_bit_exact."""
    ids, s, t, off, p = G.layout()
    a, w = ED.ring_operands(N, K, gather_div)
    img, ref, _, valid = G.expected_raw(a, w, s, t, gather_div, N)
    assert torch.equal(ref.float().double(), ref) and float(ref.abs().max()) * 8 < 2 ** 24
    nt, used = K // 64, int((t >= 0).sum())
    assert nt >= 4 and used == 8
    swaps = [(tt, tt - 3) for tt in range(3, nt)] + [(tt, tt + 1) for tt in range(nt - 1)]
    if nt > 7:                                                          # the long loop: both ends and the middle
        swaps = [sw for sw in swaps if sw[0] in (0, 1, 3, 4, nt // 2, nt - 2, nt - 1)]
    for tt, src in swaps:
        other, *_ = G.expected_raw(*ED.with_k_tile_from(a, w, tt, src), s, t, gather_div, N)
        d = tiles_that_differ(img, other)
        assert bool(d[:used].all()), (tt, src, (~d[:used]).nonzero().tolist())
        assert not bool(d[used:].any())


@pytest.mark.parametrize("gather_div", (G.TOP_K, 0))
def test_expected_image_is_expected_raw_on_the_shared_layout(gather_div):
    ids, s, t, off, p = G.layout()
    a, w = G.operands("integer", 128, 128, G.T if gather_div else len(s), 4100 + gather_div)
    img, ref, _, valid = G.expected_raw(a, w, s, t, gather_div, 128)
    img2, ref2, valid2 = ED.expected_image(a, w, s, t, G.N_SLOTS, gather_div)
    assert torch.equal(img, img2) and torch.equal(ref, ref2) and torch.equal(valid, valid2)
    a2, w2 = ED.int_operands(G.E, 128, 128, len(a), 4100 + gather_div)
    assert torch.equal(a, a2) and torch.equal(w, w2)                    # the same regime


def test_expected_image_forms_planted_products_by_ieee_rules():
    ids, s, t, off, p = G.layout()
    a, w = G.operands("integer", 128, 128, G.T, 1)
    clean, *_ = ED.expected_image(a, w, s, t, G.N_SLOTS, G.TOP_K)
    a = a.clone()
    a[40, 5] = float("inf")
    img, ref, valid = ED.expected_image(a, w, s, t, G.N_SLOTS, G.TOP_K)
    rows = p.view(G.T, G.TOP_K)[40].long()
    for r in rows.tolist():
        wk = w[int(t[r // 64]), :, 5].double()
        assert torch.equal(ref[r].isnan(), wk == 0)                     # Inf * 0
        assert torch.equal(ref[r][wk != 0], torch.sign(wk[wk != 0]) * float("inf"))
    other = torch.ones(len(s), dtype=torch.bool)
    other[rows] = False
    assert torch.equal(img[other], clean[other])
    same = ED.same_by_class(img, img.clone())
    assert bool(same.all())
    x = torch.tensor([[SENT16, 0x7FC0]], dtype=torch.int16)             # two NaNs of different payloads
    y = torch.tensor([[SENT16, 0x7FC1]], dtype=torch.int16)
    assert bool(x.view(BF)[0, 1].isnan()) and bool(y.view(BF)[0, 1].isnan())
    assert ED.same_by_class(x, y).tolist() == [[True, True]]
    y[0, 0] = 0
    assert ED.same_by_class(x, y).tolist() == [[False, True]]


@pytest.mark.parametrize("name", list(ED.LIMITS))
def test_the_routing_cases_at_the_limits(name):
    from k8s_gpu_scheduler_amd.ops import loadgen
    T, E, k = ED.LIMITS[name]
    x, k2, ids, w, s, t, off, p = ED.limit_case(name)
    assert k2 == k and tuple(x.shape) == (T, E) and x.dtype == BF and T * k <= loadgen.MOE_MAX_SLOTS
    check_layout(ids, E, s, t, off, p)
    counts = torch.bincount(ids.flatten().long(), minlength=E)
    d = x.double().gather(1, ids.long())
    assert float((d - d[:, :1]).abs().max()) <= 32                      # inside the weight bound's contract
    if name.startswith(("ties", "normal")):
        assert T * k == 32768 and len(t) == 764 and int(ids.max()) == 255      # ids through the unsigned char
        assert int((counts > 0).sum()) >= (256 if name.startswith("normal") else 250)
        groups_per_wave = -(-(T * k // 64) // 16)
        assert groups_per_wave == 32
    if name.startswith("normal"):
        assert all(len(set(r)) == E for r in x.tolist())                # no two equal in any row
    if name.startswith("ties"):
        kth = x.double().sort(dim=1, descending=True).values
        assert float((kth[:, k - 1] == kth[:, k]).float().mean()) > 0.9   # almost every threshold is tied
    if name.startswith("equal"):
        assert len(t) == 519 and counts.tolist() == [32768] + [0] * 7 and int((t == 0).sum()) == 512
        assert 32768 // 16 == 2048                                      # each (wave, expert 0) count
    if name.startswith("uneven"):
        assert counts[0] % 64 and counts[7] % 64 and counts[0] > 2 * counts[7] and int(counts[0] + counts[7]) == T
        assert T % 64 and int(s[int(off[1]) - 1]) == T and int(s[int(off[8]) - 1]) == T


def test_tie_free_keeps_the_order_and_removes_every_tie():
    x = (torch.randint(-8, 8, (50, 256), generator=torch.Generator().manual_seed(3)).float() / 4).to(BF)
    y = ED.tie_free(x)
    assert y.dtype == BF and all(len(set(r)) == 256 for r in y.tolist())
    assert torch.equal(x.double().sort(dim=1, stable=True).indices, y.double().sort(dim=1, stable=True).indices)
    assert float(y.max() - y.min()) <= 32


def test_the_small_layouts_of_the_large_offset_tests():
    for kind, tiles, n in (("experts", 3, 6), ("tokens", 2, 3), ("two-tile", 2, 66), ("two-tile-top2", 2, 66)):
        ids, E, s, t, off, p = ED.small_layout(kind)
        check_layout(ids, E, s, t, off, p)
        assert len(t) == tiles and ids.numel() == n and bool((t >= 0).all())
    assert 2 in ED.small_layout("experts")[3].tolist()
