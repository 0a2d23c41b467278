"""Exact-arithmetic, guarded-buffer tests of every GEMM tile, the tile-order maps, the fp8 decode
and the stream triad (run with `-m gpu` on an MI355X).

The tolerance tests of test_gpu_native.py allow an absolute error of 1-3 per element at the K they
use, so a dropped k-chunk or a shifted bias passes them.  Here the operands are small integers:
every product and every partial sum of the fp32-accumulate GEMM is exactly representable, the
result does not depend on the summation order, and the comparison with a float64 reference is
`torch.equal` -- one wrong element of any size fails.

  representable regime  A, Bt in {-1, 0, +1}, integer bias: |ref| <= 256 (asserted on the
                        reference alone), so bf16 holds every expected value exactly.
  rounded regime        A, Bt uniform integers in [-2, 2] (fp8: [-4, 4]), bias a multiple of 0.25:
                        the fp32 result is still exact, most outputs need the bf16 rounding and
                        many are ties, which pins round-to-nearest-even in the epilogue.

Part B runs the same operands as views into larger allocations (padded leading dimensions,
offset columns, NaN guards around A and Bt, a sentinel bit pattern around C) and compares the
guards bitwise after the launch.  Part C checks that the block -> tile maps are bijections (a hole
keeps its NaN prefill, a doubly assigned tile leaves a hole elsewhere).  Part D sends every e4m3fn
byte code through gemm_fp8 against an identity.  Part E runs the stream triad over several
grid-stride trips with a ragged tail inside guarded buffers.

The helpers (operand builders, guard wrapper, sentinel check) live here; their CPU-only tests are
in test_kernels_exact_helpers.py, which runs without a GPU.
"""
import contextlib
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
NAN = float("nan")
SENT16 = 0x5A5A            # sentinel bit pattern of the bf16 guard cells (read through int16)
SENT32 = 0x5A5A5A5A        # ... of the fp32 guard cells (read through int32)
REP_CAP = 256              # bf16 holds every integer of magnitude <= 256
REGIMES = ("rep", "rnd")
ACTS = [(False, False), (False, True), (True, False), (True, True)]      # (relu, bias)

# block tile of every selectable GEMM tile, and the tiles whose kernels stage two K-tiles in their
# prologue: a K = 64 problem falls back to a 2-stage kernel of the same block (resolve_gemm_tile)
TILE_BM = {1: 128, 2: 64, 3: 64, 4: 256, 5: 256, 6: 128, 7: 64, 8: 256, 9: 256, 10: 256, 11: 128, 12: 128,
           13: 256, 14: 256, 15: 256, 16: 128}
TILE_BN = {1: 128, 2: 128, 3: 64, 4: 256, 5: 128, 6: 128, 7: 128, 8: 128, 9: 256, 10: 256, 11: 128, 12: 128,
           13: 128, 14: 256, 15: 128, 16: 128}
NEEDS_K128 = (9, 10, 13, 14, 15, 16)
# 2, 3, 4, 5 and 7 K-tiles (minimum, double-buffer parities, fewer / as many / more tiles than the
# 5-slot ring) and one long loop
TILE_KS = (128, 192, 256, 320, 448, 1088)


# ------------------------------------------------------------------------------------------------
# helpers (CPU-tested in test_kernels_exact_helpers.py)
# ------------------------------------------------------------------------------------------------
def restore_knobs(h):
    """Every launch knob back at its default (the defaults are pinned in test_gemm_plan_cpu.py)."""
    h.reset_knobs()


@contextlib.contextmanager
def knobs(h, **settings):
    """Set process-wide launch knobs (set_<name>) for the block; every knob is back at its
    default afterwards, whatever happened inside."""
    try:
        for name, value in settings.items():
            getattr(h, "set_" + name)(value)
        yield
    finally:
        restore_knobs(h)


def rep_density(K, fp8=False):
    """Non-zero probability of the representable regime's operand entries."""
    if fp8:
        return 0.2           # entries up to +-4: E[x^2] = 7.5 p, so p = 0.2 keeps K = 384 under the cap
    return 0.5 if K <= 2048 else 0.25


def _seed(M, N, K, regime, fp8):
    return (M * 1_000_003 + N * 10_007 + K * 101 + (17 if regime == "rnd" else 0) + (5 if fp8 else 0)) % (2**31)


def build_operands(M, N, K, regime, fp8=False):
    """(a, bt, bias) on the CPU with a fixed seed: a [M, K] and bt [N, K] float32 holding small
    integers, bias [N] float32."""
    assert regime in REGIMES
    g = torch.Generator().manual_seed(_seed(M, N, K, regime, fp8))
    mag = 4 if fp8 else (1 if regime == "rep" else 2)

    def operand(rows):
        if regime == "rnd":
            return torch.randint(-mag, mag + 1, (rows, K), generator=g).float()
        nz = torch.rand(rows, K, generator=g) < rep_density(K, fp8)
        val = torch.randint(1, mag + 1, (rows, K), generator=g) * (torch.randint(0, 2, (rows, K), generator=g) * 2 - 1)
        return (val * nz).float()

    a, bt = operand(M), operand(N)
    if regime == "rep":
        bias = torch.randint(-8, 9, (N,), generator=g).float()
    else:
        bias = torch.randint(-8, 9, (N,), generator=g).float() * 0.25
    return a, bt, bias


def reference(a, bt):
    """a @ bt.T in float64 (the bias and the activation are applied by `expected`)."""
    return a.double() @ bt.double().T


def expected(ref, bias, relu, use_bias, regime):
    """The exact expected output: float32 in the representable regime (every value an integer
    of magnitude <= 256, asserted here on the reference alone), bf16 (round-to-nearest-even of the
    exact value) in the rounded regime."""
    r = ref + bias.double() if use_bias else ref
    if regime == "rep":
        cap = r.abs().max().item()
        assert cap <= REP_CAP, f"representable regime: max|ref| = {cap} > {REP_CAP}; lower the density"
    if relu:
        r = r.clamp_min(0.0)       # valid only because no NaN reaches it: the kernels' ReLU makes NaN +0.0, this keeps it
    return r.float() if regime == "rep" else r.float().to(torch.bfloat16)


def exact_match(out, exp, regime):
    """Bit-level agreement of a bf16 kernel output with `expected(...)`; no tolerance."""
    assert out.dtype == torch.bfloat16 and out.shape == exp.shape
    return torch.equal(out.float(), exp) if regime == "rep" else torch.equal(out, exp)


def first_mismatch(out, exp):
    """Where and what, for the assertion message."""
    bad = (out.float() != exp.float()).nonzero()
    if not len(bad):
        return "none"
    i, j = bad[0].tolist()
    return f"{len(bad)} elements differ, first at [{i}, {j}]: got {out[i, j].item()}, expected {exp[i, j].item()}"


def guarded_input(t, ld, r0=2, c0=8, r1=3):
    """A copy of the 2-D tensor t as the view big[r0:r0+rows, c0:c0+cols] of one allocation of
    (r0 + rows + r1) x ld elements whose every other element is NaN."""
    rows, cols = t.shape
    assert ld >= c0 + cols
    if t.dtype == FP8:
        big = torch.full((r0 + rows + r1, ld), 0x7F, dtype=torch.uint8, device=t.device)   # e4m3fn NaN
        big[r0:r0 + rows, c0:c0 + cols] = t.view(torch.uint8)
        return big.view(FP8)[r0:r0 + rows, c0:c0 + cols]
    big = torch.full((r0 + rows + r1, ld), NAN, dtype=t.dtype, device=t.device)
    big[r0:r0 + rows, c0:c0 + cols] = t
    return big[r0:r0 + rows, c0:c0 + cols]


def guarded_output(rows, cols, ld, c0, device, r0=2, r1=3):
    """(raw, view): raw is one int16 allocation of (r0 + rows + r1) x ld cells all holding SENT16,
    view its bf16 window [r0:r0+rows, c0:c0+cols] for the kernel to write."""
    assert ld >= c0 + cols
    raw = torch.full((r0 + rows + r1, ld), SENT16, dtype=torch.int16, device=device)
    return raw, raw.view(torch.bfloat16)[r0:r0 + rows, c0:c0 + cols]


def guarded_vector(n, before, after, device, sentinel=SENT32):
    """(raw, view): raw is one int32 allocation of before + n + after cells all holding the
    sentinel, view its fp32 window [before:before+n]."""
    raw = torch.full((before + n + after,), sentinel, dtype=torch.int32, device=device)
    return raw, raw.view(torch.float32)[before:before + n]


def guards_intact(raw, window, sentinel):
    """True iff every cell of raw outside `window` (a slice, or a tuple of slices) still holds the
    sentinel bit pattern."""
    g = raw.clone()
    g[window] = sentinel
    return bool((g == sentinel).all().item())


def out_window(M, N, c0, r0=2):
    return (slice(r0, r0 + M), slice(c0, c0 + N))


# ------------------------------------------------------------------------------------------------
# GPU plumbing
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    from k8s_gpu_scheduler_amd import _native
    return _native.hip(required=True)


@pytest.fixture(autouse=True)
def default_knobs(hip):
    """Every test of this module, also one that sets no knob itself, leaves the defaults behind."""
    try:
        yield
    finally:
        restore_knobs(hip)


@functools.lru_cache(maxsize=None)
def gpu_case(M, N, K, regime, fp8=False):
    """Operands on the GPU in the kernel's dtype plus the float64 reference, built once per shape
    and shared by every test (nothing writes to them)."""
    a, bt, bias = (t.cuda() for t in build_operands(M, N, K, regime, fp8))
    ref = reference(a, bt)
    dt = FP8 if fp8 else torch.bfloat16
    a_k, bt_k = a.to(dt), bt.to(dt)
    assert torch.equal(a_k.float(), a) and torch.equal(bt_k.float(), bt)     # the operands are exact
    return a_k, bt_k, bias, ref


def run_exact(M, N, K, cu_budget=0, fp8=False, regimes=REGIMES, acts=ACTS, pad=None):
    """Launch the GEMM for every regime and (relu, bias) pair into a NaN-prefilled output (pad =
    None), or, with pad = (ldc_extra, c0), from NaN-guarded padded operands into a sentinel-guarded
    window; exact comparison, and bitwise guard comparison when padded."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    fn = loadgen.gemm_fp8 if fp8 else loadgen.gemm
    for regime in regimes:
        a, bt, bias, ref = gpu_case(M, N, K, regime, fp8)
        if pad is not None:
            # fp8 rows are bytes (16-byte units), bf16 rows 2-byte elements (8-element units)
            ea, eb, c0 = (80, 144, 16) if fp8 else (72, 136, 8)
            a, bt = guarded_input(a, K + ea, c0=c0), guarded_input(bt, K + eb, r0=1, c0=2 * c0)
            assert a.stride(0) != bt.stride(0) and K not in (a.stride(0), bt.stride(0))
        for relu, use_bias in acts:
            exp = expected(ref, bias, relu, use_bias, regime)
            if pad is None:
                out = torch.full((M, N), NAN, dtype=torch.bfloat16, device="cuda")
            else:
                raw, out = guarded_output(M, N, N + pad[0], pad[1], "cuda")
            fn(a, bt, out=out, bias=bias if use_bias else None, relu=relu, cu_budget=cu_budget)
            what = (M, N, K, regime, "relu" if relu else "-", "bias" if use_bias else "-", cu_budget, pad)
            assert exact_match(out, exp, regime), (what, first_mismatch(out, exp))
            if pad is not None:
                assert guards_intact(raw, out_window(M, N, pad[1]), SENT16), ("write outside the C window", what)


WIDE_C = (8, 8)        # ldc = N + 8, column offset 8: 16-byte aligned rows (wide epilogue, 4-wave kernels)
NARROW_C = (4, 4)      # ldc = N + 4, column offset 4: 8-byte aligned rows (narrow epilogue / fallbacks)


# ------------------------------------------------------------------------------------------------
# A. exact operands, zero tolerance
# ------------------------------------------------------------------------------------------------
def forced_tile_cases():
    """(tile, M, N, K, cu_budget): 2 x 3 blocks of the tile (not a multiple of 8 blocks: legacy
    order, m0 and n0 != 0) and 4 x 2 blocks at a 64-CU share (XCD-block order on the co-run
    path), every K of TILE_KS, and K = 64 for the kernels that cannot run it themselves."""
    cases = []
    for tile in range(1, 17):
        bm, bn = TILE_BM[tile], TILE_BN[tile]
        for (gm, gn, cu) in ((2, 3, 0), (4, 2, 64)):
            for K in TILE_KS + ((64,) if tile in NEEDS_K128 else ()):
                cases.append(pytest.param(tile, gm * bm, gn * bn, K, cu,
                                          id=f"tile{tile}-{gm * bm}x{gn * bn}x{K}-cu{cu}"))
    return cases


@pytest.mark.parametrize("tile,M,N,K,cu_budget", forced_tile_cases())
def test_forced_tile_exact(hip, tile, M, N, K, cu_budget):
    with knobs(hip, gemm_tile=tile):
        assert hip.pick_gemm_tile(M, N, cu_budget) == tile
        # 8 blocks at a share: an XCD-block map; 6 blocks: the legacy order
        assert bool(hip.pick_xcd_map(M // TILE_BM[tile], N // TILE_BN[tile]) & 0xFF) == (cu_budget > 0)
        run_exact(M, N, K, cu_budget)


# (policy, M, N, tile the picker must choose at a 4-CU share)
PICKER_CASES = [pytest.param(10, 512, 512, 14, id="policy10-512x512-tile14"),
                pytest.param(10, 256, 256, 1, id="policy10-256x256-tile1"),
                pytest.param(10, 128, 128, 3, id="policy10-128x128-tile3"),
                pytest.param(11, 512, 256, 15, id="policy11-512x256-tile15"),
                pytest.param(13, 256, 256, 16, id="policy13-256x256-tile16")]


@pytest.mark.parametrize("policy,M,N,tile", PICKER_CASES)
@pytest.mark.parametrize("K", [64, 128, 320])
def test_default_picker_exact(hip, policy, M, N, tile, K):
    """The bench's paths: the default picker (no forced tile) at a small CU share."""
    with knobs(hip, gemm_policy=policy):
        assert hip.pick_gemm_tile(M, N, 4) == tile
        run_exact(M, N, K, cu_budget=4)


@pytest.mark.parametrize("M,N,K", [pytest.param(256, 256, 2048, id="256x256x2048"),
                                   pytest.param(512, 768, 4096, id="512x768x4096")])
def test_split_k_exact(hip, M, N, K):
    with knobs(hip, split_k=-1):
        assert hip.pick_split_k(M, N, K) > 1
        run_exact(M, N, K)


def test_split_k_policy8_exact(hip):
    M, N, K = 1024, 1024, 2048
    with knobs(hip, gemm_policy=8):
        assert hip.pick_split_k(M, N, K, 64) > 1
        run_exact(M, N, K, cu_budget=64)


def test_policy9_row_slices_exact(hip):
    """More 256 x 256 tiles than the CU share: several row-slice launches of the 8-phase kernel."""
    M, N, K = 1024, 512, 256
    with knobs(hip, gemm_policy=9):
        assert hip.pick_gemm_tile(M, N, 4) == 10
        assert hip.gemm_workgroups(M, N, K, 4) > 4
        run_exact(M, N, K, cu_budget=4)


# the 64 x 64 fp8 tile (a lone 128 x 192 problem) and the 128 x 128 one (256 x 256 at a 4-CU share)
FP8_CASES = [pytest.param(128, 192, 0, 6, id="fp8-64x64-128x192"), pytest.param(256, 256, 4, 4, id="fp8-128x128-256x256")]


@pytest.mark.parametrize("M,N,cu_budget,blocks", FP8_CASES)
@pytest.mark.parametrize("K", [128, 256, 384])
def test_fp8_exact(hip, M, N, cu_budget, blocks, K):
    assert hip.gemm_workgroups(M, N, K, cu_budget, True) == blocks
    run_exact(M, N, K, cu_budget, fp8=True)


# ------------------------------------------------------------------------------------------------
# B. padded, offset, guarded buffers
# ------------------------------------------------------------------------------------------------
PAD_ACTS = [(False, False), (True, True)]
PAD_K = 320


def padded_tile_cases():
    cases = []
    for tile in (1, 3, 10, 13, 14, 15, 16):
        bm, bn = TILE_BM[tile], TILE_BN[tile]
        for (gm, gn, cu) in ((2, 2, 0), (4, 2, 64)):
            cases.append(pytest.param(tile, gm * bm, gn * bn, cu, id=f"tile{tile}-{gm * bm}x{gn * bn}x{PAD_K}-cu{cu}"))
    return cases


@pytest.mark.parametrize("tile,M,N,cu_budget", padded_tile_cases())
def test_forced_tile_padded_guarded(hip, tile, M, N, cu_budget):
    """lda = K + 72, ldb = K + 136, offset columns, NaN around A and Bt, sentinel around C: the
    interior is exact and no cell outside the M x N window changes.  8-byte aligned C rows take the
    narrow epilogue; the 4-wave kernels (14-16) refuse them when forced."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    with knobs(hip, gemm_tile=tile):
        run_exact(M, N, PAD_K, cu_budget, acts=PAD_ACTS, pad=WIDE_C)
        if tile in (14, 15, 16):
            a, bt, _, _ = gpu_case(M, N, PAD_K, "rep")
            raw, out = guarded_output(M, N, N + NARROW_C[0], NARROW_C[1], "cuda")
            with pytest.raises(RuntimeError):
                loadgen.gemm(a, bt, out=out, cu_budget=cu_budget)
            torch.cuda.synchronize()
            assert guards_intact(raw, (slice(0, 0), slice(0, 0)), SENT16)      # nothing was launched
        else:
            run_exact(M, N, PAD_K, cu_budget, acts=PAD_ACTS, pad=NARROW_C)


@pytest.mark.parametrize("policy,M,N,tile", [pytest.param(10, 512, 512, 14, id="policy10-512x512-tile14"),
                                             pytest.param(11, 512, 256, 15, id="policy11-512x256-tile15"),
                                             pytest.param(13, 256, 256, 16, id="policy13-256x256-tile16")])
def test_policy_four_wave_padded_guarded(hip, policy, M, N, tile):
    """The 4-wave kernels as the picker launches them, and their fallback kernels when C rows are
    only 8-byte aligned."""
    with knobs(hip, gemm_policy=policy):
        assert hip.pick_gemm_tile(M, N, 4) == tile
        run_exact(M, N, PAD_K, cu_budget=4, acts=PAD_ACTS, pad=WIDE_C)
        run_exact(M, N, PAD_K, cu_budget=4, acts=PAD_ACTS, pad=NARROW_C)


@pytest.mark.parametrize("tile", [1, 10])
def test_narrow_epilogue_knob_padded_guarded(hip, tile):
    """set_wide_epilogue(0): the 8-byte epilogue on 16-byte aligned rows."""
    M, N = 2 * TILE_BM[tile], 2 * TILE_BN[tile]
    with knobs(hip, gemm_tile=tile, wide_epilogue=0):
        run_exact(M, N, PAD_K, acts=PAD_ACTS, pad=WIDE_C)


def test_split_k_padded_guarded(hip):
    """splitk_reduce indexes the partials by e / N and C by m * ldc."""
    with knobs(hip, split_k=-1):
        assert hip.pick_split_k(256, 256, 2048) > 1
        run_exact(256, 256, 2048, acts=PAD_ACTS, pad=WIDE_C)
        run_exact(256, 256, 2048, acts=PAD_ACTS, pad=NARROW_C)
    with knobs(hip, gemm_policy=8):
        assert hip.pick_split_k(512, 512, 1024, 64) > 1
        run_exact(512, 512, 1024, cu_budget=64, acts=PAD_ACTS, pad=WIDE_C)
        run_exact(512, 512, 1024, cu_budget=64, acts=PAD_ACTS, pad=NARROW_C)


def test_policy9_row_slices_padded_guarded(hip):
    M, N = 1024, 512
    with knobs(hip, gemm_policy=9):
        assert hip.pick_gemm_tile(M, N, 4) == 10 and hip.gemm_workgroups(M, N, PAD_K, 4) > 4
        run_exact(M, N, PAD_K, cu_budget=4, acts=PAD_ACTS, pad=WIDE_C)
        run_exact(M, N, PAD_K, cu_budget=4, acts=PAD_ACTS, pad=NARROW_C)


@pytest.mark.parametrize("M,N,cu_budget,blocks", FP8_CASES)
def test_fp8_padded_guarded(hip, M, N, cu_budget, blocks):
    """The fp8 kernel stages through a bf16 view with lda / 2: lda = K + 80, ldb = K + 144 bytes."""
    K = 384
    assert hip.gemm_workgroups(M, N, K, cu_budget, True) == blocks
    run_exact(M, N, K, cu_budget, fp8=True, acts=PAD_ACTS, pad=WIDE_C)
    run_exact(M, N, K, cu_budget, fp8=True, acts=PAD_ACTS, pad=NARROW_C)


# ------------------------------------------------------------------------------------------------
# C. tile-order bijection (64 x 64 blocks, K = 64: large grids are tiny problems)
# ------------------------------------------------------------------------------------------------
ORDER_ACTS = [(False, False), (True, True)]


@pytest.mark.parametrize("tiles_m,tiles_n", [(7, 3), (19, 5), (9, 1)])
def test_tile_order_remainder_and_partial_group(hip, tiles_m, tiles_n):
    """Block counts that are no multiple of 8 (remainder split of the XCD remap) with a partial
    last GROUP_M group."""
    with knobs(hip, gemm_tile=3):
        assert (tiles_m * tiles_n) % 8 and tiles_m % 8
        assert hip.pick_xcd_map(tiles_m, tiles_n) == 0
        run_exact(64 * tiles_m, 64 * tiles_n, 64, regimes=("rep",), acts=ORDER_ACTS)


@pytest.mark.parametrize("tiles_m,tiles_n,px", [(8, 1, 8), (1, 8, 1), (3, 8, 1)])
def test_tile_order_xcd_split(hip, tiles_m, tiles_n, px):
    with knobs(hip, gemm_tile=3):
        assert hip.pick_xcd_map(tiles_m, tiles_n) & 0xFF == px
        run_exact(64 * tiles_m, 64 * tiles_n, 64, regimes=("rep",), acts=ORDER_ACTS)


@pytest.mark.parametrize("cu_budget", [64, 0])
@pytest.mark.parametrize("group", [1, 3, 4, 64])
@pytest.mark.parametrize("tiles_m,tiles_n,px", [(6, 4, 2), (24, 16, 4), (40, 24, 4)])
def test_tile_order_xcd_groups(hip, tiles_m, tiles_n, px, group, cu_budget):
    """Rows per group that divide the XCD rectangle's height, that do not (partial last group), and
    that exceed it."""
    with knobs(hip, gemm_tile=3, xcd_group=group):
        xmap = hip.pick_xcd_map(tiles_m, tiles_n)
        assert xmap & 0xFF == px and xmap >> 8 == group
        run_exact(64 * tiles_m, 64 * tiles_n, 64, cu_budget, regimes=("rep",), acts=ORDER_ACTS)


@pytest.mark.parametrize("tile", [14, 10])
def test_tile_order_xcd_group3_large_tiles(hip, tile):
    M, N = 4 * TILE_BM[tile], 2 * TILE_BN[tile]
    with knobs(hip, gemm_tile=tile, xcd_group=3):
        xmap = hip.pick_xcd_map(4, 2)
        assert xmap & 0xFF == 4 and xmap >> 8 == 3
        run_exact(M, N, 128, cu_budget=64, regimes=("rep",), acts=ORDER_ACTS)


# ------------------------------------------------------------------------------------------------
# D. fp8 decode table
# ------------------------------------------------------------------------------------------------
NAN_CODES = (0x7F, 0xFF)


def _decode_operands(codes):
    """A [256, 128]: row i holds byte code i at column i % 128 if i is in codes, zero elsewhere;
    Bt = the 128 x 128 identity."""
    a8 = torch.zeros(256, 128, dtype=torch.uint8)
    for i in codes:
        a8[i, i % 128] = i
    bt = torch.eye(128).to(FP8)
    assert torch.equal(bt.view(torch.uint8), torch.eye(128, dtype=torch.uint8) * 0x38)     # 1.0 = 0x38
    return a8.cuda().view(FP8), bt.cuda()


@pytest.mark.parametrize("cu_budget,blocks", [pytest.param(0, 8, id="tile64x64"), pytest.param(2, 2, id="tile128x128")])
def test_fp8_decode_table(hip, cu_budget, blocks):
    """Every e4m3fn (OCP) byte code through the MFMA against an identity: each finite code must come
    out as the value the encoding defines (all exact in bf16; subnormals and +-448 included), the
    rest of its row 0; the two NaN codes, in a call of their own, give NaN."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    assert hip.gemm_workgroups(256, 128, 128, cu_budget, True) == blocks
    finite = [i for i in range(256) if i not in NAN_CODES]
    a, bt = _decode_operands(finite)
    out = torch.full((256, 128), NAN, dtype=torch.bfloat16, device="cuda")
    loadgen.gemm_fp8(a, bt, out=out, cu_budget=cu_budget)
    want = torch.zeros(256, 128)
    table = torch.arange(256, dtype=torch.uint8).view(FP8).float()
    for i in finite:
        want[i, i % 128] = table[i]
    assert table[finite].isfinite().all() and table[0x7E] == 448.0 and table[0x01] == 2.0 ** -9
    got = out.float().cpu()
    bad = (got != want).nonzero().tolist()
    assert not bad, [(i, j, got[i, j].item(), want[i, j].item()) for i, j in bad[:8]]

    a, bt = _decode_operands(NAN_CODES)
    out = torch.full((256, 128), NAN, dtype=torch.bfloat16, device="cuda")
    loadgen.gemm_fp8(a, bt, out=out, cu_budget=cu_budget)
    got = out.float().cpu()
    for i in NAN_CODES:
        assert got[i, i % 128].isnan(), (hex(i), got[i, i % 128].item())
    rest = [i for i in range(256) if i not in NAN_CODES]
    assert torch.equal(got[rest], torch.zeros(len(rest), 128))


# ------------------------------------------------------------------------------------------------
# E. stream triad: several grid-stride trips, ragged tail, guards
# ------------------------------------------------------------------------------------------------
TRIAD_S = 2.5          # b, c integers in [-1024, 1024]: b + 2.5 c is exact, fused or not
TRIAD_GUARD = (64, 1024)                    # sentinel / NaN cells before and after each array (16-byte multiples)


def triad_n(blocks):
    """Floats such that the widest kernel (8 float4 per thread) takes three full trips of `blocks`
    blocks and a fourth, partial one whose last unrolled step is itself partial."""
    return 4 * (3 * blocks * 256 * 8 + 256 * 5 + 77)


def triad_buffers(n, seed):
    """(raw_a, a, b, c, ref): a is a sentinel-guarded window, b and c NaN-guarded ones, all
    16-byte aligned slices of larger allocations."""
    before, after = TRIAD_GUARD
    g = torch.Generator(device="cuda").manual_seed(seed)
    ins = []
    for _ in range(2):
        big = torch.full((before + n + after,), NAN, device="cuda")
        big[before:before + n] = torch.randint(-1024, 1025, (n,), device="cuda", generator=g).float()
        ins.append(big[before:before + n])
    raw, a = guarded_vector(n, before, after, "cuda")
    ref = ins[0] + TRIAD_S * ins[1]
    assert all(t.data_ptr() % 16 == 0 for t in (a, *ins))
    return raw, a, ins[0], ins[1], ref


def run_triad(raw, a, b, c, ref, blocks, what):
    from k8s_gpu_scheduler_amd.ops import loadgen
    raw.fill_(SENT32)
    loadgen.triad(a, b, c, TRIAD_S, blocks=blocks)
    assert torch.equal(a, ref), (what, int((a != ref).sum().item()), "elements differ")
    before = TRIAD_GUARD[0]
    assert guards_intact(raw, slice(before, before + a.numel()), SENT32), ("write outside a", what)


@functools.lru_cache(maxsize=None)
def small_triad(n):
    return triad_buffers(n, seed=n)


@pytest.mark.parametrize("n", [pytest.param(triad_n(1), id="blocks1-4trips"), pytest.param(triad_n(3), id="blocks3-4trips"),
                               pytest.param(4, id="one-float4"), pytest.param(4 * 255, id="under-one-block")])
@pytest.mark.parametrize("variant", range(11))
def test_triad_trips_tail_guards(hip, variant, n):
    blocks = 3 if n == triad_n(3) else 1
    with knobs(hip, triad_variant=variant):
        run_triad(*small_triad(n), blocks, (variant, n, blocks))


def test_triad_default_blocks_two_trips_and_size_switch(hip):
    """The bench's situation: the default 8192 blocks and an array the 4x kernels need a second,
    partial trip for (explicit variant 3 and the auto variant 6); at just over 128 MiB the same
    array takes variant 10's write-through arm."""
    n = 4 * (8192 * 256 * 4 + 1000)
    assert n * 4 >= 128 << 20 and n * 12 > 96 << 20
    bufs = triad_buffers(n, seed=7)
    for variant in (3, 6, 10, 8):
        with knobs(hip, triad_variant=variant):
            run_triad(*bufs, 0, (variant, n, 0))
