"""The MoE kernels -- loadgen.moe_route, moe_gemm, moe_combine -- where their exact modules do not reach (run with
`-m gpu` on an MI355X).  Everything here reuses those modules: NAN, SENT16 and guards_intact of
test_gpu_kernels_exact.py, layout / operands / guarded_a / guarded_w / guarded_out / expected_raw of
test_gpu_moe_gemm_exact.py (G), chain of test_gpu_moe_combine_exact.py (CMB), the regimes, guarded outputs and weight
bound of test_gpu_moe_route_exact.py (RT), check_layout of test_moe_cpu.py and the co-run harness (CO), unchanged.

  A  ring wrap     moe_gemm stages K tile t + 2 into the buffer of tile t - 1; G's K in {64, 128, 192} never refills a
                   buffer.  G's integer regime and 7-expert layout at K in {256, 320, 448, 1088} -- 4, 5, 7 and 17 K
                   tiles: the first refill, two, the whole ring more than once, a long loop -- x N in {64, 256} (both
                   BN) x both modes; guarded operands, the whole out allocation compared.  Still exact: |a| <= 64,
                   |w| <= 2 in steps of 2^-3, so a sum over K = 1088 is at most 1088 * 128 * 8 = 1.1e6 units < 2^24
                   (asserted, as in G).  test_moe_mx_edges_helpers.py shows on the CPU that with these operands a stale
                   K tile (t - 3 in t's place) or an early one (t + 1) changes every used row tile x column tile.
  B  non-finite    one value planted per launch (N = K = 128); the output is compared with the float64 product of the
                   planted operands formed term by term (IEEE: Inf * 0 = NaN), NaN by class and everything else
                   bitwise, and the SET of cells that differ from the unplanted launch is asserted.
  C  limits        routing at 32,768 slots (T = 4096 x E = 256 x k = 8: 764 tiles, every align wave 32 groups, expert
                   ids up to 255; T = 32768 x E = 8 x k = 1 with equal logits: every (wave, expert 0) count 2,048, 512
                   full tiles of 519), a ragged T = 32767 shared unevenly by experts 0 and 7, and the prefill
                   workload's T = 2048 x E = 128 x k = 8: ids and layout bitwise against the references, twice into
                   the same guarded buffers.  On the first two layouts moe_gemm (integer regime, N = K = 64, both
                   modes: grids of 764 and 519 workgroups for the XCD remap) and moe_combine (D = 64, against
                   chain(fp32=True)).  The references alone take under 0.05 s at n = 32,768 on the CPU.
  D  past 4 GiB    one operand per test in an UNINITIALISED allocation of which only the windows are filled: the
                   weights' expert stride, a's rows (both modes), out's rows, combine's y and out.
  E  launch paths  side stream, then one capture and two replays (outputs re-filled before the first only).
  F  co-run        CO.R launches against CO.BASE_PAIRS, bit-exact: moe_gemm at K = 1088 (N = 256 and 64, both modes)
                   and K = 320, moe_route and moe_combine at 32,768 slots.
"""
import functools

import pytest
import torch

import test_gpu_corun_exact as CO
import test_gpu_moe_combine_exact as CMB
import test_gpu_moe_gemm_exact as G
import test_gpu_moe_route_exact as RT
from test_gpu_kernels_exact import NAN, SENT16, SENT32, guarded_input, guards_intact
from test_gpu_paged_large_addresses import need_free
from test_moe_cpu import check_layout

pytestmark = pytest.mark.gpu

# MEASURED on an MI355X (printed by CO.corun; victim slowdown = co-run event time / alone host time):
MEASURED = """
  The module: 71 tests in 4.9 s, none skipped (a test with an operand past 4 GiB takes 0.02 .. 0.1 s here and up to
  1.4 s in the whole suite, its allocation most of it).  Every
  comparison bit-exact; no kernel needed a change.  The seven co-run victims (five moe_gemm, moe_route, moe_combine):
  aggressor | mode        victim slowdown  aggressor slowdown  passes
  stream    | same-slice   0.41 .. 0.97     0.50 .. 1.06        5 .. 20
  stream    | unmasked     0.73 .. 1.78     0.78 .. 0.81       10 .. 72
  mfma      | same-slice   0.28 .. 1.26     0.36 .. 0.61       24 .. 225
  mfma      | unmasked     0.24 .. 0.96     0.30 .. 0.45       31 .. 272
  The largest pass counts are moe_route's: its four launches take 0.75 .. 0.81 ms alone (the one align workgroup over
  32,768 slots most of it) against 0.08 .. 0.18 ms for the other victims, and need up to 272 of the 512 MFMA passes
  the harness allows.  The largest victim slowdown under the stream aggressor is moe_gemm's at N = 256, K = 1088.
"""

BF, I32 = torch.bfloat16, torch.int32
INF = float("inf")
RING_NS, RING_KS = (64, 256), (256, 320, 448, 1088)
N_SLOTS, TOP_K = G.N_SLOTS, G.TOP_K
GIB = 1 << 30


@pytest.fixture(scope="module")
def L():
    from k8s_gpu_scheduler_amd import _native
    from k8s_gpu_scheduler_amd.ops import loadgen
    _native.hip(required=True)
    return loadgen


@pytest.fixture(scope="module")
def hip():
    from k8s_gpu_scheduler_amd import _native
    return _native.hip(required=True)


# ------------------------------------------------------------------------------------------------
# shared pieces (CPU-tested in test_moe_mx_edges_helpers.py)
# ------------------------------------------------------------------------------------------------
def ring_seed(N, K):
    return 100 * N + K


def ring_operands(N, K, gather_div):
    """The operands test_ring_wrap_bit_exact launches, on the CPU."""
    return G.operands("integer", N, K, G.T if gather_div else len(G.layout()[1]), ring_seed(N, K))


def with_k_tile_from(a, w, t, src):
    """(a, w) with K tile t of both replaced by K tile src: what the MFMAs of tile t would read had the ring slot
    still held (src = t - 3) or already held (src = t + 1) another tile."""
    a, w = a.clone(), w.clone()
    a[:, 64 * t:64 * t + 64] = a[:, 64 * src:64 * src + 64].clone()
    w[:, :, 64 * t:64 * t + 64] = w[:, :, 64 * src:64 * src + 64].clone()
    return a, w


def int_operands(E, N, K, rows, seed):
    """G's integer regime for any number of experts: (a [rows, K], w [E, N, K]) bf16 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-64, 65, (rows, K), generator=g).float()
    w = torch.randint(-2, 3, (E, N, K), generator=g).float() * (2.0 ** -(torch.arange(E) % 4).float())[:, None, None]
    return a.to(BF), w.to(BF)


def expected_image(a, w, s, t, n_slots, gather_div):
    """G.expected_raw for any layout and for non-finite operands: (the int16 image of the out window, the float64
    reference, the valid mask).  With a non-finite operand the products are formed and summed term by term (no BLAS:
    Inf * 0 and NaN * 0 are NaN and reach the sum)."""
    P, (_, N, K) = len(s), w.shape
    valid = s < n_slots
    src = torch.where(valid, (s // gather_div if gather_div else torch.arange(P, dtype=I32)), torch.zeros_like(s)).long()
    e_row = t.long().repeat_interleave(64)
    finite = bool(a[src[valid]].isfinite().all()) and bool(w.isfinite().all())
    ref = torch.zeros(P, N, dtype=torch.float64)
    for e in e_row[valid].unique().tolist():
        rows = (valid & (e_row == e)).nonzero().flatten()
        ar, we = a[src[rows]].double(), w[e].double()
        ref[rows] = ar @ we.T if finite else (ar[:, None, :] * we[None, :, :]).sum(-1)
    img = torch.full((P, N), SENT16, dtype=torch.int16)
    img[e_row >= 0] = 0
    img[valid] = ref[valid].float().to(BF).view(torch.int16)
    return img, ref, valid


def same_by_class(got, img):
    """int16 images: NaN by class (any payload), everything else bitwise."""
    return (got == img) | (got.view(BF).isnan() & img.view(BF).isnan())


def tie_free(x):
    """Every row of x keeps its order (value, then index) and takes the 256 distinct values i / 8, i in [-128, 128):
    exact in bf16, no two equal, spreads of at most 32."""
    T, E = x.shape
    assert E <= 256
    order = x.double().sort(dim=1, stable=True).indices
    grid = ((torch.arange(E) - 128).float() / 8).expand(T, E)
    out = torch.empty(T, E)
    out.scatter_(1, order, grid)
    out = out.to(BF)
    assert all(len(set(r)) == E for r in out[:4].tolist())
    return out


LIMITS = {"ties-4096x256x8": (4096, 256, 8), "normal-4096x256x8": (4096, 256, 8), "equal-32768x8x1": (32768, 8, 1),
          "uneven-32767x8x1": (32767, 8, 1), "prefill-2048x128x8": (2048, 128, 8)}
GRID_LAYOUTS = ("ties-4096x256x8", "equal-32768x8x1")


@functools.lru_cache(maxsize=None)
def limit_case(name):
    """(logits bf16 [T, E], k, reference ids, weights, sorted_ids, tile_expert, expert_offsets, slot_pos) on the CPU."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    T, E, k = LIMITS[name]
    kind = name.split("-")[0]
    if kind == "ties":
        x = RT.logits_for("ties", T, E, k, 4096)
    elif kind == "normal":
        x = tie_free(RT.logits_for("normal", T, E, k, 4097))
    elif kind == "equal":
        x = torch.full((T, E), 0.75).to(BF)
    elif kind == "uneven":
        x = torch.zeros(T, E)
        to7 = torch.rand(T, generator=torch.Generator().manual_seed(7)) < 0.3
        x[~to7, 0] = 2.0
        x[to7, 7] = 2.0
        x = x.to(BF)
    else:
        x = RT.logits_for("normal", T, E, k, 2048)
    ids, w = loadgen.moe_topk_reference(x, k)
    return (x, k, ids, w) + loadgen.moe_align_reference(ids, E)


def full_image(rows, cols, r0, c0, shape, window):
    """The int16 image of a whole SENT16-filled allocation of `shape` whose [r0:, c0:] window holds `window`."""
    img = torch.full(shape, SENT16, dtype=torch.int16)
    img[r0:r0 + rows, c0:c0 + cols] = window
    return img


# ------------------------------------------------------------------------------------------------
# launch objects: reset / enqueue / check, as the co-run module's have
# ------------------------------------------------------------------------------------------------
class GemmCase:
    """The inputs of one moe_gemm problem on the GPU (guarded) and the image of the whole out allocation."""

    def __init__(self, L, a, w, s, t, n_slots, gather_div, what):
        self.L, self.n_slots, self.gather_div, self.what = L, n_slots, gather_div, what
        self.P, self.N = len(s), w.shape[1]
        img, ref, valid = expected_image(a, w, s, t, n_slots, gather_div)
        assert torch.equal(ref.float().double(), ref)                                   # exact in fp32
        self.img = img
        self.ga = G.guarded_a(a, None if gather_div else ~valid)       # in place: pad rows and unused tiles hold NaN
        self.gw, self.s, self.t = G.guarded_w(w), s.cuda(), t.cuda()
        raw, _ = G.guarded_out(self.P, self.N)
        self.want = full_image(self.P, self.N, G.R0, G.C0, tuple(raw.shape), img)

    def launch(self, tag=None):
        return GemmLaunch(self, tag)


class GemmLaunch:
    def __init__(self, case, tag):
        self.case, self.tag = case, tag
        self.raw, self.out = G.guarded_out(case.P, case.N)

    def reset(self):
        self.raw.fill_(SENT16)

    def enqueue(self, st):
        c = self.case
        c.L.moe_gemm(c.ga, c.gw, c.s, c.t, c.n_slots, gather_div=c.gather_div, out=self.out, stream=st, check=False)

    def check(self, tag):
        got = self.raw.cpu()
        bad = (got != self.case.want).nonzero()
        assert len(bad) == 0, (tag, self.case.what, self.tag, len(bad), bad[:4].tolist())


@functools.lru_cache(maxsize=None)
def ring_case(L, N, K, gather_div):
    ids, s, t, off, p = G.layout()
    a, w = ring_operands(N, K, gather_div)
    return GemmCase(L, a, w, s, t, N_SLOTS, gather_div, ("moe_gemm", N, K, gather_div))


class RouteCase:
    def __init__(self, L, name):
        self.L, self.name = L, name
        self.x, self.k, *self.ref = limit_case(name)
        self.T, self.E = self.x.shape
        self.lg = guarded_input(self.x.cuda(), self.E + 16)
        l_sel = self.x.double().gather(1, self.ref[0].long())
        self.w_bound = (RT.weight_bound(l_sel, self.k) + RT.U) * self.ref[1].double()    # + u: ref_w is rounded to fp32

    def launch(self, tag=None):
        return RouteLaunch(self, tag)


class RouteLaunch:
    def __init__(self, case, tag):
        self.case, self.tag = case, tag
        self.outs = RT.guarded_outputs(case.T, case.E, case.k, case.L)

    def reset(self):
        for raw, _ in self.outs.values():
            raw.fill_(SENT32)

    def enqueue(self, st):
        c = self.case
        c.L.moe_route(c.lg, c.k, **{nm: v for nm, (_, v) in self.outs.items()}, stream=st, check=False)

    def results(self):
        torch.cuda.synchronize()
        for nm, (raw, v) in self.outs.items():
            assert guards_intact(raw, slice(RT.PAD, RT.PAD + v.numel()), SENT32), (self.case.name, self.tag, nm)
        return tuple(v.cpu() for _, v in self.outs.values())

    def check(self, tag):
        c = self.case
        ids, w, s, t, off, p = self.results()
        rid, rw, rs, rt_, roff, rp = c.ref
        for nm, a, b in zip(("topk_ids", "sorted_ids", "tile_expert", "expert_offsets", "slot_pos"), (ids, s, t, off, p),
                            (rid, rs, rt_, roff, rp)):
            assert torch.equal(a, b), (tag, c.name, self.tag, nm, int((a != b).sum()))
        assert bool(((w.double() - rw.double()).abs() <= c.w_bound).all()), (tag, c.name, self.tag, "weights")


@functools.lru_cache(maxsize=None)
def route_case(L, name):
    return RouteCase(L, name)


class CombineCase:
    def __init__(self, L, name, D, seed):
        self.L, self.name = L, name
        _, k, _, w, s, _, _, p = limit_case(name)
        T, n = w.shape[0], w.numel()
        y = torch.randn(len(s), D, generator=torch.Generator().manual_seed(seed))
        y[s >= n] = NAN                                                # pad rows and unused tiles: never read
        y = y.to(BF)
        self.T, self.D = T, D
        self.exp = CMB.chain(y, p, w, fp32=True)
        assert not bool(self.exp.isnan().any())
        big = torch.full((CMB.R0 + len(s) + 3, D + 24), NAN, dtype=BF, device="cuda")
        self.gy = big[CMB.R0:CMB.R0 + len(s), CMB.C0:CMB.C0 + D]
        self.gy.copy_(y)
        self.p, self.w = p.cuda(), w.cuda()

    def launch(self, tag=None):
        return CombineLaunch(self, tag)


class CombineLaunch:
    def __init__(self, case, tag):
        self.case, self.tag = case, tag
        self.raw, self.out = CMB.guarded_output(case.T, case.D, case.D + 16, CMB.C0, "cuda")
        self.want = full_image(case.T, case.D, CMB.R0, CMB.C0, tuple(self.raw.shape), case.exp.view(torch.int16))

    def reset(self):
        self.raw.fill_(SENT16)

    def enqueue(self, st):
        c = self.case
        c.L.moe_combine(c.gy, c.p, c.w, out=self.out, stream=st)

    def check(self, tag):
        bad = (self.raw.cpu() != self.want).nonzero()
        assert len(bad) == 0, (tag, self.case.name, self.tag, len(bad), bad[:4].tolist())


@functools.lru_cache(maxsize=None)
def combine_case(L, name):
    return CombineCase(L, name, 64, 640 + len(name))


def run_once(x):
    x.reset()
    torch.cuda.synchronize()
    x.enqueue(None)
    torch.cuda.synchronize()
    x.check("one launch")


def side_stream_and_graph_replay(x):
    """A launch on a side stream, then one capture and two replays; the outputs are re-filled with the sentinel before
    the first replay only (the second writes over the first: idempotent).  The shape of the swiglu module's test."""
    s = torch.cuda.Stream()
    x.reset()
    torch.cuda.synchronize()
    x.enqueue(s)
    s.synchronize()
    x.check("side stream")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        x.enqueue(s)
    for k in range(2):
        if k == 0:
            x.reset()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        s.synchronize()
        x.check(("replay", k))
    del g


def corun(hip, name, launches, aggressor, mode):
    try:
        CO.corun(hip, CO.Load(name, {}, launches), CO.aggressor_for(aggressor, mode), mode)
    finally:
        CO.restore_knobs(hip)


PAIRS = [pytest.param(a, m, id=f"{a}-{m}") for a, m in CO.BASE_PAIRS]


# ------------------------------------------------------------------------------------------------
# A. the ring wraps
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gather_div", (TOP_K, 0))
@pytest.mark.parametrize("N", RING_NS)
@pytest.mark.parametrize("K", RING_KS)
def test_ring_wrap_bit_exact(L, K, N, gather_div):
    got, a, w, s, t, _ = G.run(L, "integer", N, K, gather_div, ring_seed(N, K))
    a2, w2 = ring_operands(N, K, gather_div)
    assert torch.equal(a, a2) and torch.equal(w, w2)                                    # what the CPU helper test examined
    img, ref, _, valid = G.expected_raw(a, w, s, t, gather_div, N)
    assert float(ref.abs().max()) * 8 < 2 ** 24
    assert torch.equal(ref.float().double(), ref)                                       # exact in fp32
    assert int((ref[valid].float().to(BF).double() != ref[valid]).sum()) > 0            # some outputs need the rounding
    bad = (got != img).nonzero()
    assert len(bad) == 0, (K, len(bad), bad[:4].tolist())
    assert int((got[64 * 8:] == SENT16).all()) and bool((got[1:64] == 0).all())         # unused tiles; expert 1's 63 pad rows


# ------------------------------------------------------------------------------------------------
# B. non-finite values: sets of cells
# ------------------------------------------------------------------------------------------------
NF_N = NF_K = 128


def planted(L, gather_div, plant):
    """(got as bf16, the cells whose bits differ from the unplanted launch, a, w after planting, the layout)."""
    lay = G.layout()
    ids, s, t, off, p = lay
    a, w = G.operands("integer", NF_N, NF_K, G.T if gather_div else len(s), 4100 + gather_div)
    clean = GemmCase(L, a, w, s, t, N_SLOTS, gather_div, "clean")
    x = clean.launch()
    run_once(x)
    was = x.raw.cpu()
    a, w = a.clone(), w.clone()
    plant(a, w)
    img, _, valid = expected_image(a, w, s, t, N_SLOTS, gather_div)
    raw, out = G.guarded_out(len(s), NF_N)
    L.moe_gemm(G.guarded_a(a, None if gather_div else ~valid), G.guarded_w(w), s.cuda(), t.cuda(), N_SLOTS,
               gather_div=gather_div, out=out)
    got = raw.cpu()
    same = same_by_class(got, full_image(len(s), NF_N, G.R0, G.C0, tuple(raw.shape), img))
    assert bool(same.all()), (int((~same).sum()), (~same).nonzero()[:4].tolist())
    win = (slice(G.R0, G.R0 + len(s)), slice(G.C0, G.C0 + NF_N))
    changed = got != was
    assert int(changed.sum()) == int(changed[win].sum())               # nothing outside the window
    pads = (t.long().repeat_interleave(64) >= 0) & ~valid
    assert bool((got[win][pads] == 0).all()) and bool((got[win][64 * 8:] == SENT16).all())
    return got[win].view(BF), changed[win], a, w, lay


def rows_mask(rows, cols=None):
    m = torch.zeros(len(G.layout()[1]), NF_N, dtype=torch.bool)
    if cols is None:
        m[rows] = True
    else:
        m[rows, cols] = True
    return m


@pytest.mark.parametrize("which", ("a token of three experts", "the token behind expert 1's only slot"))
def test_a_nan_in_a_token_reaches_exactly_its_k_rows(L, which):
    ids, s, t, off, p = G.layout()
    lone = int(s[int(off[1])]) // TOP_K
    assert int(off[2]) - int(off[1]) == 64 and int(s[int(off[1]) + 1]) == N_SLOTS         # one slot, 63 pad rows
    tok = lone if which.startswith("the token") else next(i for i in range(G.T) if i != lone and len(set(ids[i].tolist())) == 3)
    assert int(s[int(off[1])]) // 3 == lone
    got, changed, *_ = planted(L, TOP_K, lambda a, w: a.__setitem__((tok, 77), NAN))
    rows = p.view(G.T, TOP_K)[tok].long()
    want = rows_mask(rows)
    assert int(want.sum()) == TOP_K * NF_N
    assert torch.equal(got.isnan(), want) and torch.equal(changed, want)
    if tok == lone:
        assert int(off[1]) in rows.tolist() and bool((got.view(torch.int16)[int(off[1]) + 1:int(off[2])] == 0).all())


def test_an_inf_in_a_token_gives_signed_inf_or_nan_by_the_weight(L):
    ids, s, t, off, p = G.layout()
    _, w0 = G.operands("integer", NF_N, NF_K, G.T, 4100 + TOP_K)
    tok, k0 = 40, 5
    got, changed, a, w, _ = planted(L, TOP_K, lambda a, w: a.__setitem__((tok, k0), INF))
    assert torch.equal(w, w0)
    rows = p.view(G.T, TOP_K)[tok].long()
    assert torch.equal(changed, rows_mask(rows))
    kinds = set()
    for r in rows.tolist():
        wk = w[int(t[r // 64]), :, k0].float()
        want = torch.where(wk == 0, torch.tensor(NAN), torch.where(wk > 0, torch.tensor(INF), torch.tensor(-INF)))
        assert torch.equal(got[r].float().isnan(), want.isnan())
        assert torch.equal(got[r].float()[~want.isnan()], want[~want.isnan()])
        kinds |= {"nan"} if bool(want.isnan().any()) else set()
        kinds |= {"+inf"} if bool((want == INF).any()) else set()
        kinds |= {"-inf"} if bool((want == -INF).any()) else set()
    assert kinds == {"nan", "+inf", "-inf"}


def test_a_nan_in_a_weight_reaches_one_column_of_its_experts_valid_rows(L):
    ids, s, t, off, p = G.layout()
    e, n0 = 4, 97                                                      # 130 slots: two full tiles and a short one
    assert G.COUNTS[e] == 130 and int(off[e + 1]) - int(off[e]) == 192
    got, changed, *_ = planted(L, TOP_K, lambda a, w: w.__setitem__((e, n0, 31), NAN))
    rows = torch.arange(int(off[e]), int(off[e]) + 130)
    want = rows_mask(rows, n0)
    assert torch.equal(got.isnan(), want) and torch.equal(changed, want)
    assert bool((got.view(torch.int16)[int(off[e]) + 130:int(off[e + 1])] == 0).all())


@pytest.mark.parametrize("which", ("first", "inner"))
def test_in_place_a_nan_row_stays_its_own(L, which):
    """gather_div = 0: the pad rows and the unused tiles of `a` hold NaN throughout (planted() hides them) and are never
    read; a NaN in a valid row -- the tile's first, which every pad row of the tile loads in its own stead, or an inner
    one -- makes that row NaN and no other."""
    ids, s, t, off, p = G.layout()
    i = int(off[6]) + (0 if which == "first" else 3)                    # expert 6: 7 rows and 57 pad rows
    assert G.COUNTS[6] == 7 and int(s[i]) < N_SLOTS
    got, changed, *_ = planted(L, 0, lambda a, w: a.__setitem__((i, 64), NAN))
    want = rows_mask([i])
    assert torch.equal(got.isnan(), want) and torch.equal(changed, want)


# ------------------------------------------------------------------------------------------------
# C. routing and layout at the limits
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LIMITS))
def test_route_at_the_limits_twice_into_the_same_buffers(L, name):
    c = route_case(L, name)
    T, E, k = LIMITS[name]
    x = c.launch()
    run_once(x)
    first = x.results()
    x.enqueue(None)                                                     # over its own result
    second = x.results()
    assert all(torch.equal(a.view(I32), b.view(I32)) for a, b in zip(first, second))
    x.check("second launch")
    ids, w, s, t, off, p = second
    check_layout(ids, E, s, t, off, p)
    counts = torch.bincount(ids.flatten().long(), minlength=E)
    if name.startswith(("ties", "normal")):
        assert T * k == 32768 and len(t) == 764 and int(ids.max()) == 255      # ids through the unsigned char
        assert int((counts > 0).sum()) >= (256 if name.startswith("normal") else 250)
    if name.startswith("normal"):
        assert all(len(set(r)) == E for r in c.x[::97].tolist())                        # tie-free rows
    if name.startswith("equal"):
        assert len(t) == 519 and counts.tolist() == [32768] + [0] * 7 and int((t == 0).sum()) == 512
    if name.startswith("uneven"):
        assert counts[0] % 64 and counts[7] % 64 and counts[0] > 2 * counts[7] and int(counts[0] + counts[7]) == T
        assert T % 64 and int(s[int(off[1]) - 1]) == T and int(s[int(off[8]) - 1]) == T   # pad rows at both ends


@pytest.mark.parametrize("gather_div", ("k", 0))
@pytest.mark.parametrize("name", GRID_LAYOUTS)
def test_moe_gemm_on_the_largest_layouts(L, name, gather_div):
    T, E, k = LIMITS[name]
    _, _, ids, _, s, t, off, p = limit_case(name)
    gather_div = k if gather_div == "k" else 0
    a, w = int_operands(E, 64, 64, T if gather_div else len(s), 64 + E)
    c = GemmCase(L, a, w, s, t, T * k, gather_div, (name, gather_div))
    assert len(t) in (764, 519) and int((c.img == SENT16).all(1).sum()) == 64 * int((t < 0).sum())
    run_once(c.launch())


@pytest.mark.parametrize("name", GRID_LAYOUTS)
def test_moe_combine_on_the_largest_layouts(L, name):
    run_once(combine_case(L, name).launch())


# ------------------------------------------------------------------------------------------------
# D. offsets past 4 GiB
# ------------------------------------------------------------------------------------------------
BIG_LD = 2 ** 30 + 8                                                   # rows 2 and later start past 4 GiB
ROW_LD = 2 ** 25 + 8                                                   # rows 64 and later do
C0 = 8


def strided(rows, cols, ld, c0=C0, tail=0):
    """(raw, view): an UNINITIALISED int16 allocation and its bf16 window [rows, cols] at column c0, row stride ld."""
    raw = torch.empty(((rows - 1) * ld + c0 + cols + tail,), dtype=torch.int16, device="cuda")
    view = raw.view(BF).as_strided((rows, cols), (ld, 1), c0)
    assert view.data_ptr() % 16 == 0
    return raw, view


@functools.lru_cache(maxsize=None)
def small_layout(kind):
    """(ids, E, sorted_ids, tile_expert, expert_offsets, slot_pos): "experts": six top-1 tokens over three experts, one
    tile each; "two-tile": 66 slots of one expert, as 66 x 1 or 33 x 2."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    if kind == "experts":
        ids, E = torch.tensor([[0], [2], [1], [2], [0], [2]], dtype=I32), 3
    elif kind == "tokens":
        ids, E = torch.tensor([[0], [1], [0]], dtype=I32), 2
    else:
        ids, E = torch.zeros((66, 1) if kind == "two-tile" else (33, 2), dtype=I32), 1
    return (ids, E) + loadgen.moe_align_reference(ids, E)


def big_gemm(L, kind, gather_div, big, need):
    """One moe_gemm with one operand (`big`: "w", "a" or "out") spread past 4 GiB; the rest guarded as everywhere."""
    need_free(need * GIB, f"moe_gemm with {big} spread past 4 GiB")
    ids, E, s, t, off, p = small_layout(kind)
    n, P, N, K = ids.numel(), len(s), 64, 64
    a, w = int_operands(E, N, K, ids.shape[0] if gather_div else P, 77)
    img, ref, valid = expected_image(a, w, s, t, n, gather_div)
    assert torch.equal(ref.float().double(), ref)
    raw = None
    try:
        ga, gw = G.guarded_a(a, None if gather_div else ~valid), G.guarded_w(w)
        graw, out = G.guarded_out(P, N)
        want = full_image(P, N, G.R0, G.C0, tuple(graw.shape), img)
        if big == "w":
            raw = torch.empty(((E - 1) * BIG_LD + N * (K + 8) + 16,), dtype=torch.int16, device="cuda")
            gw = raw.view(BF).as_strided((E, N, K), (BIG_LD, K + 8, 1), C0)
            gw.copy_(w.cuda())
            assert 2 * BIG_LD * 2 > 2 ** 32 and bool((t == 2).any()) and gw.stride(0) == BIG_LD
        elif big == "a" and gather_div:
            raw, ga = strided(len(a), K, BIG_LD)
            ga.copy_(a.cuda())
            assert 2 * BIG_LD * 2 > 2 ** 32 and 2 in (s[valid] // gather_div).tolist()
        elif big == "a":
            raw, ga = strided(P, K, ROW_LD)
            ga[:n].copy_(a[:n].cuda())                                 # the pad rows stay uninitialised: never read
            assert 64 * ROW_LD * 2 > 2 ** 32 and bool(valid[64:].any()) and bool(valid[:n].all())
        else:
            raw, out = strided(P, N, ROW_LD, tail=C0)
            graw = raw.as_strided((P, C0 + N + C0), (ROW_LD, 1), 0)     # 8 guard cells on each side of every row window
            graw.fill_(SENT16)
            want = full_image(P, N, 0, C0, (P, C0 + N + C0), img)
            assert 64 * ROW_LD * 2 > 2 ** 32 and bool(valid[64:].any()) and not bool(valid[64:].all())
        L.moe_gemm(ga, gw, s.cuda(), t.cuda(), n, gather_div=gather_div, out=out)
        torch.cuda.synchronize()
        bad = (graw.cpu() != want).nonzero()
        assert len(bad) == 0, (big, gather_div, len(bad), bad[:4].tolist())
    finally:
        del raw
        ga = gw = out = graw = None
        torch.cuda.empty_cache()


def test_weights_with_an_expert_stride_past_4_gib(L):
    big_gemm(L, "experts", 1, "w", 5)


def test_gathered_a_rows_past_4_gib(L):
    big_gemm(L, "tokens", 1, "a", 5)


def test_in_place_a_rows_past_4_gib(L):
    big_gemm(L, "two-tile", 0, "a", 9)


@pytest.mark.parametrize("gather_div", (1, 0))
def test_out_rows_past_4_gib(L, gather_div):
    big_gemm(L, "two-tile", gather_div, "out", 9)


@pytest.mark.parametrize("big", ("y", "out"))
def test_combine_rows_past_4_gib(L, big):
    """y: 33 tokens x top-2 whose 66 rows of y are ROW_LD apart (slot_pos names rows 64 and 65, past 4 GiB); out: 66
    tokens x top-1 into rows ROW_LD apart, 8 guard cells on each side of every row."""
    need_free(5 * GIB, f"moe_combine with {big} spread past 4 GiB")
    ids, E, s, t, off, p = small_layout("two-tile" if big == "out" else "two-tile-top2")
    T, k = ids.shape
    D = 72
    g = torch.Generator().manual_seed(72)
    y = torch.randn(len(s), D, generator=g).to(BF)
    w = torch.softmax(torch.randn(T, k, generator=g), dim=1).float().contiguous() * 1.5
    exp = CMB.chain(y, p, w, fp32=True).view(torch.int16)
    raw = None
    try:
        if big == "y":
            raw, gy = strided(66, D, ROW_LD)
            gy.copy_(y[:66].cuda())
            graw, out = CMB.guarded_output(T, D, D + 16, CMB.C0, "cuda")
            want = full_image(T, D, CMB.R0, CMB.C0, tuple(graw.shape), exp)
            assert int(p.max()) == 65 and int(p.max()) * ROW_LD * 2 > 2 ** 32
        else:
            gy = guarded_input(y.cuda(), D + 24)
            raw, out = strided(T, D, ROW_LD, tail=C0)
            graw = raw.as_strided((T, C0 + D + C0), (ROW_LD, 1), 0)
            graw.fill_(SENT16)
            want = full_image(T, D, 0, C0, (T, C0 + D + C0), exp)
            assert (T - 1) * ROW_LD * 2 > 2 ** 32
        L.moe_combine(gy, p.cuda(), w.cuda(), out=out)
        torch.cuda.synchronize()
        bad = (graw.cpu() != want).nonzero()
        assert len(bad) == 0, (big, len(bad), bad[:4].tolist())
    finally:
        del raw
        gy = out = graw = None
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------
# E. other launch paths
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gather_div", (TOP_K, 0))
def test_moe_gemm_side_stream_and_graph_replay(L, gather_div):
    side_stream_and_graph_replay(ring_case(L, 256, 448, gather_div).launch())


def test_moe_combine_side_stream_and_graph_replay(L):
    side_stream_and_graph_replay(combine_case(L, GRID_LAYOUTS[0]).launch())


# ------------------------------------------------------------------------------------------------
# F. beside a co-running load
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aggressor,mode", PAIRS)
@pytest.mark.parametrize("N,K,gather_div", [(256, 1088, TOP_K), (256, 1088, 0), (64, 1088, TOP_K), (64, 1088, 0), (256, 320, TOP_K)])
def test_moe_gemm_corun(hip, L, N, K, gather_div, aggressor, mode):
    c = ring_case(L, N, K, gather_div)
    corun(hip, f"moe_gemm-{N}x{K}-div{gather_div}", [c.launch(r) for r in range(CO.R)], aggressor, mode)


@pytest.mark.parametrize("aggressor,mode", PAIRS)
def test_moe_route_corun(hip, L, aggressor, mode):
    c = route_case(L, GRID_LAYOUTS[0])
    corun(hip, "moe_route-4096x256x8", [c.launch(r) for r in range(CO.R)], aggressor, mode)


@pytest.mark.parametrize("aggressor,mode", PAIRS)
def test_moe_combine_corun(hip, L, aggressor, mode):
    c = combine_case(L, GRID_LAYOUTS[0])
    corun(hip, "moe_combine-4096x64x8", [c.launch(r) for r in range(CO.R)], aggressor, mode)
