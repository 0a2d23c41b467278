"""CPU-only tests of the reference of test_gpu_numeric_edges.py: the integer definition of the
fp32 -> bf16 conversion agrees with torch's, the comparison rejects the three usual wrong encoders
on named entries of the edge table, the table holds every rounding class it is there for, and the
NaN entries (compared by class only) stay a small, fixed part of it."""
import pytest
import torch

import test_gpu_numeric_edges as E


def torch_bf16_bits(u):
    return E.bf16_to_bits(E.bits_to_f32(u).to(torch.bfloat16))


def position(table, pattern):
    hit = (table == pattern).nonzero()
    assert len(hit) >= 1, f"{pattern:#010x} is not in the table"
    return int(hit[0])


def test_bit_views_round_trip():
    u = torch.tensor([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x3F800000, 0x7F800001])
    assert torch.equal(E.f32_to_bits(E.bits_to_f32(u)), u)
    assert E.bits_to_f32(u)[5].item() == 1.0 and E.bits_to_f32(u)[0].item() == 0.0
    b = torch.tensor([0, 0x8000, 0x7F80, 0xFFFF, 0x0001])
    assert torch.equal(E.bf16_to_bits(E.bits_to_f32(b << 16).to(torch.bfloat16)), b)


def test_rne_definition_agrees_with_torch_on_the_table_and_on_random_patterns():
    table = E.edge_table()
    g = torch.Generator().manual_seed(20)
    for u in (table, torch.randint(0, 1 << 32, (1 << 20,), generator=g, dtype=torch.int64)):
        nan = E.f32_is_nan(u)
        assert torch.equal(nan, E.bits_to_f32(u).isnan())
        mine, theirs = E.bf16_bits_rne(u), torch_bf16_bits(u)
        assert torch.equal(mine[~nan], theirs[~nan])
        assert E.bf16_is_nan(mine[nan]).all() and E.bf16_is_nan(theirs[nan]).all()
        assert not E.bf16_is_nan(mine[~nan]).any()


def test_table_is_fixed_and_shuffled():
    a, b = E.edge_table(), E.edge_table()
    assert torch.equal(a, b) and a.shape == (E.TABLE_N,) and a.dtype == torch.int64
    assert int(a.min()) >= 0 and int(a.max()) < 1 << 32
    assert len(set(a.tolist())) > E.TABLE_N - 4                      # the seeded fill repeats next to nothing
    nan = E.f32_is_nan(a)
    # a NaN shares a packed conversion pair (cells 2 i, 2 i + 1) with a finite value
    partner = nan[torch.arange(E.TABLE_N) ^ 1]
    assert int((nan & ~partner).sum()) >= 5


def test_nan_entries_stay_under_the_cap():
    """NaN entries are compared by class only: 10 planted ones plus whatever the seeded fill holds,
    at most 5 % of the table, so the class-only comparison cannot swallow the test."""
    table = E.edge_table()
    assert E.NAN_CAP == 25
    for relu in (False, True):
        exp, nan = E.epilogue_expected(table, relu)
        assert int(nan.sum()) == (0 if relu else int(E.f32_is_nan(table).sum()))
        assert int(nan.sum()) <= E.NAN_CAP
        assert not E.bf16_is_nan(exp[~nan]).any()
    assert 2 * len(E.EDGE_NANS) <= int(E.f32_is_nan(table).sum()) <= E.NAN_CAP


# (fp32 pattern, its bf16 encoding) by class
CLASSES = {"tie to even, up": (0x3F818000, 0x3F82),
           "tie to even, down": (0x3F808000, 0x3F80),
           "carry into the exponent": (0x3F7FFFFF, 0x3F80),
           "overflow to Inf": (0x7F7F8000, 0x7F80),
           "overflow to -Inf": (0xFF7FFFFF, 0xFF80),
           "largest value that stays finite": (0x7F7F7FFF, 0x7F7F),
           "subnormal to bf16 subnormal": (0x00010000, 0x0001),
           "subnormal rounded up to a bf16 subnormal": (0x0000FFFF, 0x0001),
           "subnormal to the smallest normal": (0x007FFFFF, 0x0080),
           "subnormal to +0": (0x00007FFF, 0x0000),
           "subnormal tie to +0": (0x00008000, 0x0000),
           "negative subnormal to -0": (0x80000001, 0x8000)}


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_table_holds_every_rounding_class(name):
    pattern, want = CLASSES[name]
    table = E.edge_table()
    i = position(table, pattern)
    exp, nan = E.epilogue_expected(table, False)
    assert int(exp[i]) == want and not nan[i]
    assert int(torch_bf16_bits(table[i:i + 1])) == want


def test_table_holds_nans_with_the_payload_in_the_dropped_bits_only():
    table = E.edge_table()
    _, nan = E.epilogue_expected(table, False)
    for pattern in (0x7F80FFFF, 0x7F800001, 0xFF80FFFF, 0xFF800001):
        assert pattern & 0x007F0000 == 0 and nan[position(table, pattern)]
    for pattern in (0x7F800000, 0xFF800000):                          # the infinities are not NaNs
        i = position(table, pattern)
        assert not nan[i] and int(E.bf16_bits_rne(table)[i]) == pattern >> 16


def test_epilogue_model_zero_relu_and_nan():
    u = torch.tensor([0x80000000, 0x00000000, 0x80000001, 0x00000001, 0xBF800000, 0x3F800000, 0x7FC00000,
                      0xFFC00000, 0x7F800000, 0xFF800000, 0x00010000, 0x80010000])
    exp, nan = E.epilogue_expected(u, False)
    assert exp.tolist()[:6] == [0x0000, 0x0000, 0x8000, 0x0000, 0xBF80, 0x3F80]      # -0.0 + 0.0 = +0.0
    assert nan.tolist() == [False] * 6 + [True, True] + [False] * 4
    assert exp.tolist()[8:] == [0x7F80, 0xFF80, 0x0001, 0x8001]                      # subnormals are kept
    exp, nan = E.epilogue_expected(u, True)
    assert not nan.any()                                                              # relu(NaN) = +0.0
    assert exp.tolist() == [0, 0, 0, 0, 0, 0x3F80, 0, 0, 0x7F80, 0, 0x0001, 0]


def truncate(u):
    return u >> 16


def round_half_up(u):
    return torch.where(E.f32_is_nan(u), (u >> 16) | 0x0040, (u + 0x8000) >> 16)


def rne_without_nan_guard(u):
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF


# encoder, a table entry that tells it from the definition, what it makes of that entry
WRONG = [pytest.param(truncate, 0x3F80FFFF, 0x3F80, id="truncation"),
         pytest.param(truncate, 0x7F80FFFF, 0x7F80, id="truncation-nan-to-inf"),
         pytest.param(round_half_up, 0x3F808000, 0x3F81, id="round-half-up"),
         # (0x7F80FFFF + 0x7FFF carries into the kept mantissa and stays a NaN, 0x7F81; the smaller payload does not)
         pytest.param(rne_without_nan_guard, 0x7F800001, 0x7F80, id="no-nan-guard-to-inf"),
         pytest.param(rne_without_nan_guard, 0x7FFFFFFF, 0x8000, id="no-nan-guard-to-minus-zero")]


@pytest.mark.parametrize("encoder,pattern,makes", WRONG)
def test_comparison_rejects_wrong_encoders(encoder, pattern, makes):
    table = E.edge_table()
    exp, nan = E.epilogue_expected(table, False)
    v = torch.where(table == 0x80000000, torch.zeros_like(table), table)
    assert bool(E.edges_match(E.bf16_bits_rne(v), exp, nan).all())
    assert bool(E.edges_match(torch_bf16_bits(v), exp, nan).all())                    # torch's encoder passes too
    got = encoder(v)
    i = position(table, pattern)
    assert int(got[i]) == makes
    ok = E.edges_match(got, exp, nan)
    assert not ok[i] and not ok.all()
    assert f"src={pattern:#010x}" in E.edge_mismatches(got.view(1, -1), exp, nan, table, limit=E.TABLE_N)


def test_comparison_sees_one_unwritten_cell_and_a_nan_in_the_wrong_place():
    table = E.edge_table()
    exp, nan = E.epilogue_expected(table, False)
    good = exp.repeat(4, 1)
    assert bool(E.edges_match(good, exp, nan).all())
    hole = good.clone()
    hole[2, 17] = E.SENT16
    assert int((~E.edges_match(hole, exp, nan)).sum()) == 1
    finite = int((~nan).nonzero()[0])
    stray = good.clone()
    stray[3, finite] = 0x7FC0                                                         # a NaN where a number belongs
    assert not E.edges_match(stray, exp, nan)[3, finite]
    lost = good.clone()
    lost[0, int(nan.nonzero()[0])] = 0x7F80                                           # Inf where a NaN belongs
    assert int((~E.edges_match(lost, exp, nan)).sum()) == 1


def test_f64_reference_to_bf16():
    inf = float("inf")
    ref = torch.tensor([1.0, -3.0, 257.0, inf, -inf, float("nan"), 1e39, 0.0, 2.0 ** -133], dtype=torch.float64)
    exp, nan = E.f64_to_bf16_expected(ref)
    assert nan.tolist() == [False] * 5 + [True] + [False] * 3
    assert exp[~nan].tolist() == [0x3F80, 0xC040, 0x4380, 0x7F80, 0xFF80, 0x7F80, 0x0000, 0x0001]
    exp, nan = E.f64_to_bf16_expected(ref, relu=True)
    assert not nan.any() and exp.tolist() == [0x3F80, 0, 0x4380, 0x7F80, 0, 0, 0x7F80, 0, 0x0001]


def test_triad_plants_sit_where_the_kernels_change_path():
    n = E.triad_n(1)
    pos = E.triad_plant_positions(n)
    k = len(E.TRIAD_PLANTS)
    assert k == 7 and pos[0] == 0 and pos[1] + k == n               # the first float4, the last float4
    n4 = n // 4
    for u in (1, 2, 3, 4, 8):                                       # the first element of each ragged last trip
        trip = 256 * u
        assert 4 * (n4 // trip) * trip in pos and n4 % trip
    # the planted sums in float64: what the table says, NaN where it says None
    for pb, pc, pa in E.TRIAD_PLANTS:
        b, c = (E.bits_to_f32(torch.tensor([p])).double() for p in (pb, pc))
        r = E.f32_to_bits((b + E.TRIAD_S * c).float())
        assert bool(E.f32_is_nan(r)) if pa is None else int(r) == pa
