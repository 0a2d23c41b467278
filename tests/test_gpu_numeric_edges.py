"""bf16 rounding edges and non-finite values through every epilogue, the gather and the triad (run
with `-m gpu` on an MI355X).

The exact-arithmetic suites (test_gpu_kernels_exact.py, test_gpu_gather_exact.py) keep every value
finite, below 512 and inside a few binades.  Here the data are the values they leave out: fp32
patterns at every rounding edge of the fp32 -> bf16 conversion (ties both ways, the carry into the
exponent, the overflow to Inf, subnormals, NaNs whose payload lies in the dropped bits), Inf / NaN
operands, signed zeros.  What the kernels must do with them is written down in the module
docstring of k8s_gpu_scheduler_amd/ops/loadgen.py; the reference here is integer arithmetic on bit
patterns (`bf16_bits_rne`) and explicit float64 sums, never another GPU path.

  A. the 512-entry edge table as the bias of an all-zero GEMM through every epilogue: generic
     kernel wide / narrow, fp8 kernel, 8-phase kernel wide / narrow, 4-wave kernel, splitk_reduce
     (the eighth, the gather's, is part C)
  B. Inf / NaN operands reach exactly the outputs that depend on them; accumulator overflow
  C. gather: all 65536 bf16 codes at every D, two-row bags with non-finite / cancelling /
     overflowing / subnormal sums
  D. triad: signed zeros, Inf, NaN, subnormals, overflow at the first and last float4 and at the
     start of every kernel's ragged last trip

NaN results are compared by class (the payload is unspecified), everything else bitwise.  The
helpers are CPU-tested in test_numeric_edges_helpers.py, which runs without a GPU.
"""
import functools

import pytest
import torch

from test_gpu_kernels_exact import (FP8, NAN, SENT16, SENT32, TILE_BM, TILE_BN, TRIAD_GUARD, TRIAD_S, build_operands,
                                    guarded_input, guarded_output, guards_intact, knobs, out_window, triad_buffers, triad_n)
from test_gpu_kernels_exact import default_knobs, hip      # noqa: F401  (fixtures: the native module; autouse knob reset)

pytestmark = pytest.mark.gpu

TABLE_N = 512
NAN_CAP = TABLE_N * 5 // 100          # at most 5 % of the table may be compared by class only
BF16_MAX = 0x7F7F                     # largest finite bf16
EDGE_NANS = (0x7FC00000, 0x7F800001, 0x7F80FFFF, 0x7FFFFFFF, 0x7FBF0000)


# ------------------------------------------------------------------------------------------------
# reference (CPU-tested in test_numeric_edges_helpers.py)
# ------------------------------------------------------------------------------------------------
def f32_is_nan(u):
    """NaN class of fp32 bit patterns (int64 tensor of values in [0, 2^32))."""
    return ((u >> 23) & 0xFF == 0xFF) & ((u & 0x7FFFFF) != 0)


def bf16_is_nan(b):
    """NaN class of bf16 bit patterns (int64 tensor of values in [0, 2^16))."""
    return ((b >> 7) & 0xFF == 0xFF) & ((b & 0x7F) != 0)


def bf16_bits_rne(u):
    """fp32 -> bf16 round-to-nearest-even, defined on bit patterns in integer arithmetic: int64
    tensor of fp32 patterns in, int64 tensor of bf16 patterns out.  A NaN (exponent 0xFF, mantissa
    != 0) gives the quiet NaN of its sign (compare it by class: bf16_is_nan); everything else is
    (u + 0x7FFF + lsb) >> 16, which carries into the exponent and overflows to Inf by itself."""
    assert u.dtype == torch.int64 and int(u.min()) >= 0 and int(u.max()) < 1 << 32
    rounded = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return torch.where(f32_is_nan(u), ((u >> 16) & 0x8000) | 0x7FC0, rounded)


def edge_table():
    """512 fp32 bit patterns (int64), fixed: every rounding edge of every exponent class in both
    signs, +-Inf, NaNs with the payload in the kept / the dropped / both halves, a seeded fill over
    the whole 32-bit range, then a seeded shuffle (so NaNs share a packed conversion pair with
    finite values)."""
    pats = [(s << 31) | (e << 23) | (m << 16) | lo
            for s in (0, 1) for e in (0, 1, 126, 127, 128, 253, 254) for m in (0x00, 0x01, 0x7E, 0x7F)
            for lo in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)]
    assert len(pats) == 336
    pats += [0x7F800000, 0xFF800000]
    pats += [n | (s << 31) for n in EDGE_NANS for s in (0, 1)]
    g = torch.Generator().manual_seed(950)
    fill = torch.randint(0, 1 << 32, (TABLE_N - len(pats),), generator=g, dtype=torch.int64)
    table = torch.cat([torch.tensor(pats, dtype=torch.int64), fill])
    return table[torch.randperm(TABLE_N, generator=g)]


def bits_to_f32(u):
    """int64 fp32 patterns -> the float32 tensor with exactly these bits."""
    return torch.where(u >= 1 << 31, u - (1 << 32), u).to(torch.int32).view(torch.float32)


def f32_to_bits(f):
    return f.contiguous().view(torch.int32).long() & 0xFFFFFFFF


def bf16_to_bits(t):
    return t.contiguous().view(torch.int16).long() & 0xFFFF


def epilogue_expected(bits, relu):
    """What an epilogue makes of v = 0.0f + bias for bias = the fp32 patterns `bits`:
    (expected bf16 patterns, mask of the entries that are NaN and compared by class).  The add
    turns -0.0 into +0.0, keeps subnormals (the kernels run with fp32 denormals on, MFMA C / D never
    flush) and leaves NaN a NaN; ReLU is v > 0 ? v : 0, so NaN and every negative value become
    +0.0; then the nearest-even conversion."""
    v = torch.where(bits == 0x80000000, torch.zeros_like(bits), bits)
    nan = f32_is_nan(v)
    if relu:
        positive = (v >> 31 == 0) & (v != 0) & ~nan
        v = torch.where(positive, v, torch.zeros_like(v))
        nan = torch.zeros_like(nan)
    return bf16_bits_rne(v), nan


def edges_match(got, exp, nan):
    """Elementwise: got (bf16 patterns) is a NaN where `nan`, equals exp bitwise elsewhere."""
    return torch.where(nan, bf16_is_nan(got), got == exp)


def edge_mismatches(got, exp, nan, src=None, limit=8):
    """For the assertion message: how many cells differ and the first few as (index, source
    pattern, got, expected)."""
    exp, nan = exp.expand_as(got), nan.expand_as(got)
    bad = (~edges_match(got, exp, nan)).nonzero()
    rows = []
    for ix in bad[:limit].tolist():
        s = "" if src is None else f" src={int(src[ix[-1]]):#010x}"
        want = "NaN" if bool(nan[tuple(ix)]) else f"{int(exp[tuple(ix)]):#06x}"
        rows.append(f"{ix}{s} got={int(got[tuple(ix)]):#06x} exp={want}")
    return f"{len(bad)} cells differ: " + "; ".join(rows)


def f64_to_bf16_expected(ref, relu=False):
    """(bf16 patterns, NaN mask) of a float64 reference: ReLU as the kernels define it, one
    rounding to fp32 (exact or an overflow for every value used here), then bf16_bits_rne."""
    if relu:
        ref = torch.where(ref > 0, ref, torch.zeros_like(ref))
    u = f32_to_bits(ref.float())
    return bf16_bits_rne(u), f32_is_nan(u)


# ------------------------------------------------------------------------------------------------
# GPU plumbing
# ------------------------------------------------------------------------------------------------
def sentinel_out(M, N):
    return torch.full((M, N), SENT16, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def assert_cells(out, exp, nan, what, src=None):
    got = bf16_to_bits(out)
    ok = edges_match(got, exp.to(got.device), nan.to(got.device))
    assert bool(ok.all()), (what, edge_mismatches(got.cpu(), exp.cpu(), nan.cpu(), src))


# ------------------------------------------------------------------------------------------------
# A. the edge table through every epilogue
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table_case(relu):
    bits = edge_table()
    exp, nan = epilogue_expected(bits, relu)
    return bits, bits_to_f32(bits).cuda(), exp.cuda(), nan.cuda()


@functools.lru_cache(maxsize=None)
def zeros(rows, K, fp8=False):
    return torch.zeros(rows, K, device="cuda").to(FP8 if fp8 else torch.bfloat16)


def run_table(M, K, relu, cu_budget=0, fp8=False):
    """act(0 @ 0^T + table) into a sentinel-filled M x 512 output: every row is the table's
    expected encoding."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    bits, bias, exp, nan = table_case(relu)
    assert torch.equal(f32_to_bits(bias.cpu()), bits)               # the patterns survived the copies
    out = sentinel_out(M, TABLE_N)
    fn = loadgen.gemm_fp8 if fp8 else loadgen.gemm
    fn(zeros(M, K, fp8), zeros(TABLE_N, K, fp8), out=out, bias=bias, relu=relu, cu_budget=cu_budget)
    assert_cells(out, exp, nan, (M, K, relu, cu_budget, fp8), bits)


RELU = pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])


@RELU
@pytest.mark.parametrize("tile", range(1, 17))
def test_edge_table_forced_tile(hip, tile, relu):
    """The generic kernel's wide epilogue (tiles 1-8, 11, 12), the 8-phase kernel's narrow (9)
    and wide (10, 13) ones and the 4-wave kernel's (14-16, bias as the MFMA accumulator)."""
    M, K = TILE_BM[tile], 128
    with knobs(hip, gemm_tile=tile):
        assert hip.pick_gemm_tile(M, TABLE_N, 0) == tile
        assert hip.gemm_workgroups(M, TABLE_N, K, 0) == (M // TILE_BM[tile]) * (TABLE_N // TILE_BN[tile])
        run_table(M, K, relu)


@RELU
@pytest.mark.parametrize("tile", range(1, 14))
def test_edge_table_forced_tile_narrow_epilogue(hip, tile, relu):
    """set_wide_epilogue(0): the 8-byte epilogue of the generic and the 8-phase kernels."""
    M, K = TILE_BM[tile], 128
    with knobs(hip, gemm_tile=tile, wide_epilogue=0):
        assert hip.pick_gemm_tile(M, TABLE_N, 0) == tile
        assert hip.gemm_workgroups(M, TABLE_N, K, 0) == (M // TILE_BM[tile]) * (TABLE_N // TILE_BN[tile])
        run_table(M, K, relu)


@RELU
def test_edge_table_split_k_reduce(hip, relu):
    with knobs(hip, split_k=-1):
        assert hip.pick_split_k(256, TABLE_N, 2048) > 1
        run_table(256, 2048, relu)


@RELU
@pytest.mark.parametrize("M,cu_budget,blocks", [pytest.param(64, 0, 8, id="tile64x64"),
                                                pytest.param(128, 4, 4, id="tile128x128")])
def test_edge_table_fp8(hip, M, cu_budget, blocks, relu):
    assert hip.gemm_workgroups(M, TABLE_N, 128, cu_budget, True) == blocks
    run_table(M, 128, relu, cu_budget, fp8=True)


# ------------------------------------------------------------------------------------------------
# B. non-finite operands reach exactly their dependants
# ------------------------------------------------------------------------------------------------
INF = float("inf")
PLANT_A = ((3, 5, INF), (130, 64, -INF), (-1, 127, NAN))           # (row, k, value); -1 = the last row
PLANT_BT = (77, 31)                                                 # (column, k) of the NaN in Bt
PLANT_PATHS = [pytest.param(0, id="picker")] + [pytest.param(t, id=f"tile{t}") for t in (3, 10, 13, 14, 16)]


def explicit_reference(a, bt):
    """sum_k a[m, k] * bt[n, k] in float64 as an elementwise product and a sum, row by row: every
    Inf * 0 is formed (a BLAS may skip zero multiplicands)."""
    a, bt = a.double(), bt.double()
    return torch.stack([(a[m].unsqueeze(0) * bt).sum(1) for m in range(a.shape[0])])


@functools.lru_cache(maxsize=None)
def planted_case(M, N, fp8=False):
    """rep operands with the planted values, (a, bt, bias) on the GPU in the kernel's dtype and
    the float64 reference with the bias added (CPU)."""
    a, bt, bias = build_operands(M, N, 128, "rep", fp8)
    (r1, k1, _), (c1, k4) = PLANT_A[0], PLANT_BT
    planted = PLANT_A[2:] if fp8 else PLANT_A                       # e4m3fn has no Inf
    for r, k, v in planted:
        a[r, k] = v
    bt[c1, k4] = NAN
    if not fp8:
        col = bt[:, k1]
        assert (col == 0).any() and (col == 1).any() and (col == -1).any()
    ref = explicit_reference(a, bt) + bias.double()
    finite = ref[ref.isfinite()]
    assert finite.abs().max() <= 256 and torch.equal(finite, finite.round())
    rows = sorted({r for r, _, _ in planted})
    clean = torch.ones(M, N, dtype=torch.bool)
    clean[rows] = False
    clean[:, c1] = False
    assert ref[clean].isfinite().all() and not ref[~clean].isfinite().all()
    assert ref[:, c1].isnan().all() and ref[PLANT_A[2][0]].isnan().all()
    if not fp8:
        assert (ref[r1] == INF).any() and (ref[r1] == -INF).any() and ref[r1].isnan().any()
        r2 = PLANT_A[1][0]
        assert (ref[r2] == INF).any() and (ref[r2] == -INF).any()
    dt = FP8 if fp8 else torch.bfloat16
    a_k, bt_k = a.to(dt), bt.to(dt)
    same = lambda x, y: torch.equal(x.float().nan_to_num(7.0, 8.0, 9.0), y.nan_to_num(7.0, 8.0, 9.0))
    assert same(a_k, a) and same(bt_k, bt)
    if fp8:
        assert int(a_k.view(torch.uint8)[PLANT_A[2][0], PLANT_A[2][1]]) == 0x7F
        assert int(bt_k.view(torch.uint8)[c1, k4]) == 0x7F
    return a_k.cuda(), bt_k.cuda(), bias.cuda(), ref


def run_planted(M, N, cu_budget, fp8=False):
    from k8s_gpu_scheduler_amd.ops import loadgen
    a, bt, bias, ref = planted_case(M, N, fp8)
    fn = loadgen.gemm_fp8 if fp8 else loadgen.gemm
    for relu in (False, True):
        exp, nan = f64_to_bf16_expected(ref, relu)
        if relu:                                                    # NaN -> +0.0, -Inf -> +0.0, +Inf stays
            assert not nan.any() and bool((exp[ref.isnan() | (ref == -INF)] == 0).all())
            assert bool((exp[ref == INF] == 0x7F80).all())
        out = sentinel_out(M, N)
        fn(a, bt, out=out, bias=bias, relu=relu, cu_budget=cu_budget)
        assert_cells(out, exp, nan, (M, N, relu, cu_budget, fp8))


@pytest.mark.parametrize("tile", PLANT_PATHS)
def test_nonfinite_operands_reach_exactly_their_dependants(hip, tile):
    """+Inf, -Inf and NaN in A, NaN in Bt: the three rows and the column are what the float64
    elementwise reference says (Inf * 0 = NaN included), every other cell keeps its exact value."""
    with knobs(hip, gemm_tile=tile):
        if tile:
            assert hip.pick_gemm_tile(256, 256, 4) == tile
            assert hip.gemm_workgroups(256, 256, 128, 4) == (256 // TILE_BM[tile]) * (256 // TILE_BN[tile])
        run_planted(256, 256, cu_budget=4)


@pytest.mark.parametrize("M,N,cu_budget,blocks", [pytest.param(128, 192, 0, 6, id="tile64x64"),
                                                  pytest.param(256, 256, 4, 4, id="tile128x128")])
def test_nan_code_reaches_exactly_its_dependants_fp8(hip, M, N, cu_budget, blocks):
    assert hip.gemm_workgroups(M, N, 128, cu_budget, True) == blocks
    run_planted(M, N, cu_budget, fp8=True)


@functools.lru_cache(maxsize=None)
def overflow_case():
    """One non-zero per operand row (a[m, m % 128], bt[n, n % 128] in {-1, -0.5, 0.5, 1}), except
    row 100 of A and row 200 of Bt, whose 128 entries are all the largest finite bf16: out[100, 200]
    overflows the fp32 accumulator, out[100, n] and out[m, 200] are +-1 or +-0.5 times that value
    (one term each, exact), every other cell one product or zero."""
    g = torch.Generator().manual_seed(128)
    big = bits_to_f32(torch.tensor([BF16_MAX << 16])).item()
    ops = []
    for special in (100, 200):
        t = torch.zeros(256, 128)
        val = torch.randint(1, 3, (256,), generator=g) * (torch.randint(0, 2, (256,), generator=g) * 2 - 1)
        t[torch.arange(256), torch.arange(256) % 128] = val.float() / 2
        t[special] = big
        ops.append(t)
    a, bt = ops
    ref = explicit_reference(a, bt)
    assert ref[100, 200] > 3.5e38 and ref.isfinite().all()          # finite in float64, past fp32
    exp, nan = f64_to_bf16_expected(ref)
    assert int(exp[100, 200]) == 0x7F80 and not nan.any()
    others = torch.ones(256, 256, dtype=torch.bool)
    others[100, 200] = False
    assert bool((((exp[others] >> 7) & 0xFF) != 0xFF).all())         # every neighbour is finite
    assert bool(((exp[100] & 0x7FFF) >= BF16_MAX - 0x80).sum() >= 255)
    a_k, bt_k = a.to(torch.bfloat16), bt.to(torch.bfloat16)
    assert torch.equal(a_k.float(), a) and torch.equal(bt_k.float(), bt)
    return a_k.cuda(), bt_k.cuda(), exp, nan


@pytest.mark.parametrize("tile", PLANT_PATHS)
def test_accumulator_overflow_gives_inf_in_one_cell(hip, tile):
    from k8s_gpu_scheduler_amd.ops import loadgen
    a, bt, exp, nan = overflow_case()
    with knobs(hip, gemm_tile=tile):
        if tile:
            assert hip.pick_gemm_tile(256, 256, 4) == tile
        out = sentinel_out(256, 256)
        loadgen.gemm(a, bt, out=out, cu_budget=4)
        assert_cells(out, exp, nan, ("overflow", tile))


# ------------------------------------------------------------------------------------------------
# C. gather
# ------------------------------------------------------------------------------------------------
GATHER_DS = (64, 128, 256, 512, 1024, 2048)
C0 = 8                     # column offset of the table and output windows; ld = D + C0


def guarded_index_rows(n):
    """idx [n, 1] = 0 .. n - 1 (one bag per row), one element into a SENT32-filled allocation."""
    raw = torch.full((1 + n + 3,), SENT32, dtype=torch.int32, device="cuda")
    raw[1:1 + n] = torch.arange(n, dtype=torch.int32, device="cuda")
    return raw, raw[1:1 + n].view(n, 1)


def table_window(bits):
    """The bf16 table with exactly these patterns as a NaN-guarded window (ld = D + 8, column
    offset 8)."""
    codes = torch.where(bits >= 1 << 15, bits - (1 << 16), bits).to(torch.int16).cuda()
    view = guarded_input(codes.view(torch.bfloat16), bits.shape[1] + C0, c0=C0)
    assert torch.equal(view.contiguous().view(torch.int16), codes) and view.data_ptr() % 16 == 0
    return view


@pytest.mark.parametrize("D", GATHER_DS)
def test_gather_every_bf16_code(hip, D):
    """Bags of one row over a table holding all 65536 bf16 patterns: 0.0f + x, rounded back.  Every
    code returns bitwise -- subnormals included -- except -0.0, which the +0.0 accumulator turns
    into +0.0, and the NaNs, which stay NaNs."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    R = 65536 // D
    bits = torch.arange(65536, dtype=torch.int64).view(R, D)
    nan = bf16_is_nan(bits)
    exp = torch.where(bits == 0x8000, torch.zeros_like(bits), bits)
    ref_exp, ref_nan = f64_to_bf16_expected(torch.zeros(R, D, dtype=torch.float64) + bits_to_f32(bits << 16).double())
    assert torch.equal(ref_nan, nan) and torch.equal(ref_exp[~nan], exp[~nan])      # the float64 sum agrees
    assert int(nan.sum()) == 2 * 127 and int(exp[0, 1]) == 0x0001 and int(exp[0x8000 // D, 0x8000 % D]) == 0
    table = table_window(bits)
    idx_raw, idx = guarded_index_rows(R)
    raw, out = guarded_output(R, D, D + C0, C0, "cuda")
    loadgen.embedding_bag(table, idx, out=out)
    torch.cuda.synchronize()
    assert_cells(out, exp, nan, ("codes", D))
    assert guards_intact(raw, out_window(R, D, C0), SENT16), ("write outside the window", D)


def bf16_bits_of(values):
    b = values.to(torch.bfloat16)
    assert torch.equal(b.float(), values)
    return bf16_to_bits(b)


@functools.lru_cache(maxsize=None)
def pair_case(D):
    """(table patterns [R, D], idx, offsets, expected patterns, NaN mask, special bags): ordinary
    bags of three rows of integers in [-4, 4] alternate with five two-row bags.  A special row
    carries its special value in the columns c with c % 3 == 0 and ordinary integers elsewhere, so
    a NaN that crosses columns in the lane-group reduction shows as well."""
    g = torch.Generator().manual_seed(D + 2)
    ordinary = lambda rows: torch.randint(-4, 5, (rows, D), generator=g).float()
    special = torch.arange(D) % 3 == 0
    inf, big = 0x7F80, BF16_MAX
    x = ordinary(1)[0]
    pairs = [(torch.full((D,), inf), torch.full((D,), inf | 0x8000)),                 # +Inf, -Inf -> NaN
             (bf16_bits_of(x), bf16_bits_of(-x)),                                     # x, -x -> +0.0
             (torch.full((D,), big), torch.full((D,), big)),                          # max, max -> +Inf
             (torch.full((D,), 0x7FC1), bf16_bits_of(ordinary(1)[0])),                # NaN, finite -> NaN
             (torch.full((D,), 0x0003), torch.full((D,), 0x0005))]                    # subnormals -> 0x0008
    rows, idx, lengths = [], [], []
    for k, (p, q) in enumerate(pairs):
        base = len(rows)
        rows += list(bf16_bits_of(ordinary(3)))
        idx += [base, base + 1, base + 2]
        lengths.append(3)
        if k != 1:                                                  # (x, -x) cancels in every column
            fill = bf16_bits_of(ordinary(2))
            p, q = torch.where(special, p, fill[0]), torch.where(special, q, fill[1])
        rows += [p, q]
        idx += [base + 3, base + 4]
        lengths.append(2)
    rows += list(bf16_bits_of(ordinary(3)))
    idx += [len(rows) - 3, len(rows) - 2, len(rows) - 1]
    lengths.append(3)
    bits = torch.stack(rows)
    idx = torch.tensor(idx, dtype=torch.int32)
    offsets = torch.tensor([0] + lengths, dtype=torch.int32).cumsum(0).to(torch.int32)
    vals = bits_to_f32(bits << 16).double()
    o = offsets.tolist()
    ref = torch.stack([torch.zeros(D, dtype=torch.float64) + vals[idx[o[b]:o[b + 1]].long()].sum(0)
                       for b in range(len(lengths))])
    exp, nan = f64_to_bf16_expected(ref)
    s = special
    assert nan[1][s].all() and not nan[1][~s].any() and nan[7][s].all() and not nan[7][~s].any()
    assert not exp[3].any() and bool((exp[5][s] == inf).all()) and bool((exp[9][s] == 0x0008).all())
    assert int(nan.sum()) == 2 * int(s.sum()) and not nan[0::2].any()
    finite = ref[0::2]
    assert finite.abs().max() <= 12 and torch.equal(finite, finite.round())
    return bits, idx, offsets, exp, nan


@pytest.mark.parametrize("D", [64, 1024])
def test_gather_two_row_bags(hip, D):
    """Two rows of one bag sit in two lane groups at D = 64 (added by the cross-lane reduction)
    and in one lane's registers at D = 1024; the ordinary bags around them keep their exact sums."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    bits, idx, offsets, exp, nan = pair_case(D)
    B = offsets.numel() - 1
    table = table_window(bits)
    raw, out = guarded_output(B, D, D + C0, C0, "cuda")
    loadgen.embedding_bag(table, idx.cuda(), offsets.cuda(), out=out)
    torch.cuda.synchronize()
    assert_cells(out, exp, nan, ("pairs", D))
    assert guards_intact(raw, out_window(B, D, C0), SENT16), ("write outside the window", D)


# ------------------------------------------------------------------------------------------------
# D. triad
# ------------------------------------------------------------------------------------------------
F32_MAX = 0x7F7FFFFF
# (b pattern, c pattern, expected a pattern; None = NaN) with s = 2.5
TRIAD_PLANTS = ((0x80000000, 0x80000000, 0x80000000),               # -0.0 + 2.5 * -0.0 = -0.0, fused or not
                (0x7F800000, 0x3F800000, 0x7F800000),               # +Inf + 2.5
                (0x7F800000, 0xFF800000, None),                     # +Inf - Inf
                (0x7FC00000, 0x00000000, None),                     # NaN + 0
                (0x00000003, 0x00000000, 0x00000003),               # a subnormal survives
                (0x00000000, 0x00000004, 0x0000000A),               # 2.5 * 4 ulp = 10 ulp, a subnormal product
                (F32_MAX, F32_MAX, 0x7F800000))                     # 3.5 * max overflows


def triad_plant_positions(n):
    """Element offsets at which the seven pairs are planted (seven consecutive elements each): the
    first float4, the run ending with the last float4, and the first element of the ragged last
    trip of each unroll factor the variants use (1, 2, 3, 4 and 8 float4 per thread, one block)."""
    n4 = n // 4
    trips = sorted({(n4 // (256 * u)) * (256 * u) for u in (1, 2, 3, 4, 8)})
    assert all(0 < t < n4 for t in trips)
    pos = [0, n - len(TRIAD_PLANTS)] + [4 * t for t in trips]
    assert all(q - p >= len(TRIAD_PLANTS) for p, q in zip(sorted(pos), sorted(pos)[1:]))
    return pos


@functools.lru_cache(maxsize=None)
def planted_triad():
    n = triad_n(1)
    raw, a, b, c, _ = triad_buffers(n, seed=n + 1)
    bi, ci = b.view(torch.int32), c.view(torch.int32)
    as_i32 = lambda u: u - (1 << 32) if u >= 1 << 31 else u
    want = {}
    for p in triad_plant_positions(n):
        for k, (pb, pc, pa) in enumerate(TRIAD_PLANTS):
            bi[p + k], ci[p + k] = as_i32(pb), as_i32(pc)
            want[p + k] = pa
    ref = (b.double().cpu() + TRIAD_S * c.double().cpu()).float()   # exact, or the one overflow
    exp = f32_to_bits(ref)
    nan = f32_is_nan(exp)
    for p, pa in want.items():                                      # the float64 reference agrees with the table
        assert bool(nan[p]) if pa is None else int(exp[p]) == pa, (p, pa, int(exp[p]))
    assert int(nan.sum()) == 2 * len(triad_plant_positions(n))
    return raw, a, b, c, ref.view(torch.int32).cuda(), nan.cuda()


@pytest.mark.parametrize("variant", range(11))
def test_triad_signed_zero_nonfinite_subnormal(hip, variant):
    from k8s_gpu_scheduler_amd.ops import loadgen
    raw, a, b, c, exp, nan = planted_triad()
    raw.fill_(SENT32)
    with knobs(hip, triad_variant=variant):
        loadgen.triad(a, b, c, TRIAD_S, blocks=1)
    got = a.view(torch.int32)
    bad = (torch.where(nan, ~f32_is_nan(f32_to_bits(a)), got != exp)).nonzero().view(-1)[:8].tolist()
    assert not bad, (variant, [(i, f"{int(got[i]) & 0xFFFFFFFF:#010x}", f"{int(exp[i]) & 0xFFFFFFFF:#010x}") for i in bad])
    assert torch.equal(got[~nan], exp[~nan]) and bool(a[nan].isnan().all())
    before = TRIAD_GUARD[0]
    assert guards_intact(raw, slice(before, before + a.numel()), SENT32), ("write outside a", variant)
