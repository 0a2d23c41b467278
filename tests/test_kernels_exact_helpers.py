"""CPU-only tests of the helpers of test_gpu_kernels_exact.py: the comparison fails on a single
wrong element, the guard check on a single changed guard cell, and the representable regime's cap
(max|a @ bt.T + bias| <= 256) holds for every shape the GPU module parametrises."""
import pytest
import torch

import test_gpu_kernels_exact as X


def representable_shapes():
    """Every (M, N, K, fp8) the GPU module runs in the representable regime."""
    shapes = set()
    for p in X.forced_tile_cases():
        _, M, N, K, _ = p.values
        shapes.add((M, N, K, False))
    for p in X.PICKER_CASES:
        _, M, N, _ = p.values
        shapes.update((M, N, K, False) for K in (64, 128, 320))
    shapes.update({(256, 256, 2048, False), (512, 768, 4096, False), (1024, 1024, 2048, False), (1024, 512, 256, False)})
    for p in X.padded_tile_cases():
        _, M, N, _ = p.values
        shapes.add((M, N, X.PAD_K, False))
    shapes.update({(512, 512, X.PAD_K, False), (512, 256, X.PAD_K, False), (256, 256, X.PAD_K, False),
                   (512, 512, 1024, False), (1024, 512, X.PAD_K, False)})
    for p in X.FP8_CASES:
        M, N, _, _ = p.values
        shapes.update((M, N, K, True) for K in (128, 256, 384))
    for tm, tn in [(7, 3), (19, 5), (9, 1), (8, 1), (1, 8), (3, 8), (6, 4), (24, 16), (40, 24)]:
        shapes.add((64 * tm, 64 * tn, 64, False))
    shapes.update({(1024, 512, 128, False)})
    return sorted(shapes)


def test_representable_cap_holds_for_every_shape():
    shapes = representable_shapes()
    assert len(shapes) > 60
    worst = 0.0
    for M, N, K, fp8 in shapes:
        a, bt, bias = X.build_operands(M, N, K, "rep", fp8)
        assert a.abs().max() <= (4 if fp8 else 1) and torch.equal(a, a.round())
        assert bias.abs().max() <= 8 and torch.equal(bias, bias.round())
        ref = X.reference(a, bt)
        cap = (ref + bias.double()).abs().max().item()
        assert cap <= X.REP_CAP, (M, N, K, fp8, cap)
        X.expected(ref, bias, False, True, "rep")          # the helper's own assert agrees
        worst = max(worst, cap)
    assert worst > 32, worst                               # the data is not degenerate either


def test_representable_cap_is_enforced():
    ref = torch.zeros(4, 4, dtype=torch.float64)
    ref[2, 1] = 257.0
    with pytest.raises(AssertionError):
        X.expected(ref, torch.zeros(4), False, False, "rep")


@pytest.mark.parametrize("fp8", [False, True])
def test_operands_are_exact_in_their_formats_and_seeded(fp8):
    dt = X.FP8 if fp8 else torch.bfloat16
    for regime in X.REGIMES:
        a, bt, bias = X.build_operands(128, 192, 256, regime, fp8)
        assert torch.equal(a.to(dt).float(), a) and torch.equal(bt.to(dt).float(), bt)
        a2, bt2, bias2 = X.build_operands(128, 192, 256, regime, fp8)
        assert torch.equal(a, a2) and torch.equal(bt, bt2) and torch.equal(bias, bias2)
        # fp32 accumulation of these operands is exact, in this order or any other
        assert torch.equal((a @ bt.T).double(), X.reference(a, bt))
    a, _, bias = X.build_operands(128, 192, 256, "rnd", fp8)
    assert a.abs().max() == (4 if fp8 else 2)
    assert torch.equal(bias * 4, (bias * 4).round()) and bias.abs().max() <= 2


def test_rounded_regime_exercises_bf16_rounding_and_ties():
    a, bt, bias = X.build_operands(512, 768, 4096, "rnd")
    r = X.reference(a, bt) + bias.double()
    assert r.abs().max() < 2 ** 24 / 4
    exp = X.expected(X.reference(a, bt), bias, False, True, "rnd")
    changed = (exp.double() != r).double().mean().item()
    assert changed > 0.2, changed
    # a tie: the exact value lies halfway between two bf16 neighbours (spacing 2 above 256)
    ties = ((r.abs() >= 256) & (r.abs() < 512) & (r.remainder(2) == 1)).sum().item()
    assert ties > 1000, ties


@pytest.mark.parametrize("regime", X.REGIMES)
def test_comparison_fails_on_one_wrong_element(regime):
    a, bt, bias = X.build_operands(64, 128, 128, regime)
    ref = X.reference(a, bt)
    exp = X.expected(ref, bias, True, True, regime)
    out = exp.to(torch.bfloat16)
    assert X.exact_match(out, exp, regime)
    wrong = ref.clone()
    wrong[37, 101] += 1.0                                   # the reference output with one element changed by 1
    bad = X.expected(wrong, bias, False, True, regime).to(torch.bfloat16)
    good = X.expected(ref, bias, False, True, regime)
    assert X.exact_match(good.to(torch.bfloat16), good, regime)
    assert not X.exact_match(bad, good, regime)
    assert "first at [37, 101]" in X.first_mismatch(bad, good)
    hole = out.clone()
    hole[5, 7] = X.NAN                                      # an unwritten element of a NaN-prefilled output
    assert not X.exact_match(hole, exp, regime)
    ulp = out.clone()
    ulp.view(torch.int16)[63, 127] ^= 1                     # one bf16 ulp
    assert not X.exact_match(ulp, exp, regime)


def test_guard_check_fails_on_one_changed_guard_cell():
    M, N = 64, 128
    for (extra, c0) in (X.WIDE_C, X.NARROW_C):
        raw, out = X.guarded_output(M, N, N + extra, c0, "cpu")
        assert out.shape == (M, N) and out.stride() == (N + extra, 1) and out.dtype == torch.bfloat16
        win = X.out_window(M, N, c0)
        out.copy_(torch.ones(M, N))                         # writing the window leaves the guards alone
        assert X.guards_intact(raw, win, X.SENT16)
        assert torch.equal(raw[win].view(torch.bfloat16).float(), torch.ones(M, N))
        ld = N + extra
        after = 2 * ld + c0 + (M - 1) * ld + N              # the cell right behind the window's last element
        for cell in [(1, c0), (2 + M, c0 + N - 1), (2, c0 - 1), (after // ld, after % ld), (0, 0),
                     (raw.shape[0] - 1, raw.shape[1] - 1)]:
            before = raw[cell].item()
            raw[cell] ^= 1
            assert not X.guards_intact(raw, win, X.SENT16), cell
            raw[cell] = before
        assert X.guards_intact(raw, win, X.SENT16)


def test_vector_guard_check():
    raw, a = X.guarded_vector(1020, 64, 1024, "cpu")
    assert a.numel() == 1020 and a.data_ptr() % 16 == raw.data_ptr() % 16
    a.fill_(3.0)
    win = slice(64, 64 + 1020)
    assert X.guards_intact(raw, win, X.SENT32)
    for cell in (63, 64 + 1020, 0, raw.numel() - 1):
        raw[cell] = 0
        assert not X.guards_intact(raw, win, X.SENT32), cell
        raw[cell] = X.SENT32


@pytest.mark.parametrize("fp8", [False, True])
def test_guarded_input_is_a_nan_fenced_view(fp8):
    a, _, _ = X.build_operands(64, 64, 128, "rnd", fp8)
    t = a.to(X.FP8 if fp8 else torch.bfloat16)
    unit = 16 if fp8 else 8
    v = X.guarded_input(t, 128 + 9 * unit, c0=unit)
    assert v.shape == t.shape and v.stride() == (128 + 9 * unit, 1) and v.dtype == t.dtype
    assert torch.equal(v.float(), a)
    assert (v.data_ptr() - v.untyped_storage().data_ptr()) % 16 == 0
    whole = torch.empty(0, dtype=t.dtype).set_(v.untyped_storage()).float()
    assert int(whole.isnan().sum()) == whole.numel() - t.numel()


def test_e4m3fn_table_matches_the_ocp_definition():
    """The decode test compares the kernel with torch's view of each byte code; this pins that
    table to the OCP e4m3fn definition (bias 7, no infinities, 0x7F / 0xFF = NaN)."""
    table = torch.arange(256, dtype=torch.uint8).view(X.FP8).float()
    for code in range(256):
        s, e, m = code >> 7, (code >> 3) & 0xF, code & 7
        if (code & 0x7F) == 0x7F:
            assert table[code].isnan()
            continue
        v = (m / 8.0) * 2.0 ** -6 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7)
        assert table[code].item() == (-v if s else v), hex(code)
        assert table[code].to(torch.bfloat16).float() == table[code]      # exact in bf16
    assert tuple(X.NAN_CODES) == (0x7F, 0xFF)


def test_triad_lengths_take_a_partial_fourth_trip():
    for blocks in (1, 3):
        n4 = X.triad_n(blocks) // 4
        for U in (1, 2, 3, 4, 8):
            trip = blocks * 256 * U
            assert n4 > 3 * trip and n4 % trip, (blocks, U)         # more than three trips, the last one partial
        last = n4 - 3 * blocks * 256 * 8                            # the 8x kernel's fourth trip
        assert 0 < last < 256 * 8 and last % 256                    # one block, its last unrolled step partial
    # integer operands in [-1024, 1024] and s = 2.5: fused and unfused multiply-add agree
    c = torch.arange(-1024, 1025, dtype=torch.float64)
    assert torch.equal((X.TRIAD_S * c).float().double(), X.TRIAD_S * c)
