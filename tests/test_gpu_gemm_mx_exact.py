"""gemm_mx on the GPU: fp8 and fp4 activations on fp4 weights with REAL block scales, on both tiles (64 x 64: a lone
128 x 192 problem; 128 x 128: 256 x 256 at a 4-CU share -- reached through the public arguments only), K in
{128, 256, 384, 640}.

  scale map      one non-zero element per (row, block) of A and of W and scale bytes that change with every row and
                 block, asymmetric in every respect (positions, values, bytes, M != N): a wrong lane, byte, nibble or
                 block assignment changes the output bits.  Exact: at most K / 32 products of <= 6 significant bits
                 spread over 10 binades
  integer regime arbitrary fp4 codes, fp8 activations that are multiples of 0.5 with |v| <= 8, scale bytes 127 / 128
                 on both sides, bias a multiple of 0.25: every product is a multiple of 2^-2 of magnitude <= 192 and
                 the sums over K <= 640 stay below 2^17, so they are exact in fp32 in any order and under any sane
                 internal alignment; the output is the bf16 nearest-even rounding of the float64 result
  tables         every element code against a one-hot partner; every scale byte 1 .. 254 on either side with a partner
                 byte that brings the total exponent into [-8, 8]; a zero block with scale byte 0
  true regime    randn quantised by the reference, against the float64 product of the dequantised operands, within
                 |out - ref| <= 2^-8 |ref| + (1 + 2^-8) K 2^-23 sum |a_k w_k| (tests/test_gpu_moe_gemm_exact.py derives
                 it for an fp32 adder: the bf16 rounding and K fp32 roundings of partial sums)
  strides        padded A, W, scales and C in guarded allocations
"""
import functools

import pytest
import torch

from k8s_gpu_scheduler_amd.ops import loadgen
from test_gpu_kernels_exact import SENT16, guards_intact

pytestmark = pytest.mark.gpu

# MEASURED on an MI355X (printed by the tests named):
MEASURED = """
  true regime (test_true_regime_within_the_derived_bound), max |out - ref| / bound over both tiles and K in
  {128, 256, 384, 640}: 0.9792 with fp8 activations, 0.9868 with fp4 -- the bf16 rounding's share alone; the
  accumulation term was never needed, so the scaled instruction's adder is no worse than an fp32 one on these sums.
  outside the contract (test_scale_bytes_outside_the_contract_are_printed), both activation formats alike: scale byte
  0 under non-zero elements is an ordinary 2^-127 (with partner byte 254 the product is exactly 1.0, with 127 it is
  2^-127 = 5.877e-39, an fp32 subnormal, kept); byte 255 on either side makes every product of the block NaN.
  The module: 42 tests in 2.5 s.
"""

BF = torch.bfloat16
U8 = torch.uint8
FORMATS = ("fp8", "fp4")
# (M, N, cu_budget, workgroups): the 64 x 64 tile and the 128 x 128 one
TILES = [pytest.param(128, 192, 0, 6, id="64x64-128x192"), pytest.param(256, 256, 4, 4, id="128x128-256x256")]
KS = [128, 256, 384, 640]
ACTS = [(False, False), (False, True), (True, False), (True, True)]      # (relu, bias)
FP4_VALUES = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)


def pack(codes: torch.Tensor, fmt: str) -> torch.Tensor:
    """Element codes int64 [rows, K] -> the operand's element array."""
    if fmt == "fp8":
        return codes.to(U8).view(loadgen.FP8)
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).to(U8)


def fp8_code(v: torch.Tensor) -> torch.Tensor:
    """The e4m3fn codes of values that are exactly representable."""
    q = v.to(torch.float32).to(loadgen.FP8)
    assert torch.equal(q.to(torch.float64), v.to(torch.float64))
    return q.view(U8).to(torch.int64)


def reference(a_q, a_s, w_q, w_s, fmt):
    """float64 product of the dequantised operands and sum |a_k w_k| (both on the CPU)."""
    a = loadgen.dequantize_mx_reference(a_q.cpu(), a_s.cpu(), fmt)
    w = loadgen.dequantize_mx_reference(w_q.cpu(), w_s.cpu(), "fp4")
    return a @ w.t(), a.abs() @ w.abs().t()


def to_bf16_exact(v: torch.Tensor) -> torch.Tensor:
    """bf16 nearest-even of float64 values that are exact in fp32 (no double rounding)."""
    f = v.to(torch.float32)
    assert torch.equal(f.to(torch.float64), v)
    return f.to(BF)


def run(ops, fmt, cu_budget=0, bias=None, relu=False, out=None):
    a_q, a_s, w_q, w_s = (t.cuda() if not t.is_cuda else t for t in ops)
    r = loadgen.gemm_mx(a_q, a_s, w_q, w_s, fmt, out=out, bias=bias, relu=relu, cu_budget=cu_budget)
    torch.cuda.synchronize()
    return r


def same(out, exp, what):
    """Equal as values (+0.0 == -0.0: the sign of a zero sum is the accumulator's)."""
    out, exp = out.cpu().float(), exp.float()
    bad = (out != exp).nonzero()
    assert len(bad) == 0, f"{what}: {len(bad)} of {out.numel()} differ, first at {bad[0].tolist()}: " \
                          f"{out[tuple(bad[0])].item()} vs {exp[tuple(bad[0])].item()}"


# ------------------------------------------------------------------------------------------------ the scale map
def scale_map_operands(M, N, K, fmt):
    nb = K // 32
    m, n, kb = torch.arange(M).view(M, 1), torch.arange(N).view(N, 1), torch.arange(nb).view(1, nb)
    pos_a = (5 * kb + m % 3) % 32                                        # the one non-zero of (row, block)
    pos_w = (5 * kb + 2 * (n % 2)) % 32                                  # meets A's where m % 3 == 2 (n % 2)
    ca = torch.zeros(M, K, dtype=torch.int64)
    cw = torch.zeros(N, K, dtype=torch.int64)
    if fmt == "fp8":
        va = fp8_code(((m * 3 + kb * 5) % 7 + 1).double() * 0.5 * (1 - 2 * ((m + kb) % 2)).double())      # +-0.5 .. +-3.5
    else:
        va = ((m * 3 + kb * 5) % 7 + 1) | (((m + kb) % 2) << 3)                                           # codes 1 .. 7, signed
    vw = ((n * 5 + kb * 3) % 7 + 1) | (((n // 2 + kb) % 2) << 3)
    ca.scatter_(1, kb * 32 + pos_a, va.expand(M, nb).contiguous())
    cw.scatter_(1, kb * 32 + pos_w, vw.expand(N, nb).contiguous())
    sa = (124 + (m * 5 + kb * 3) % 7).to(U8)                             # changes with every row and every block
    sw = (125 + (n * 3 + kb * 2) % 5).to(U8)
    return pack(ca, fmt), sa.contiguous(), pack(cw, "fp4"), sw.contiguous()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("M,N,cu_budget,blocks", TILES)
@pytest.mark.parametrize("K", [128, 384])
def test_scale_map(hip, M, N, cu_budget, blocks, K, fmt):
    assert hip.gemm_mx_workgroups(M, N, K, cu_budget) == blocks
    ops = scale_map_operands(M, N, K, fmt)
    ref, _ = reference(*ops, fmt)
    assert int((ref != 0).sum()) >= M * N // 5                           # enough products meet
    out = run(ops, fmt, cu_budget)
    exp = ref.to(torch.float32)
    assert torch.equal(exp.to(torch.float64), ref)
    same(out, exp.to(BF), f"scale map {fmt} {M}x{N}x{K}")


@pytest.fixture(scope="module")
def hip():
    from k8s_gpu_scheduler_amd import _native
    return _native.hip(required=True)


# ------------------------------------------------------------------------------------------------ the integer regime
@functools.lru_cache(maxsize=None)
def integer_case(M, N, K, fmt):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K + len(fmt))
    if fmt == "fp8":
        ca = fp8_code(torch.randint(-16, 17, (M, K), generator=g).double() * 0.5)
    else:
        ca = torch.randint(0, 16, (M, K), generator=g)
    cw = torch.randint(0, 16, (N, K), generator=g)
    sa = torch.randint(127, 129, (M, K // 32), generator=g).to(U8)
    sw = torch.randint(127, 129, (N, K // 32), generator=g).to(U8)
    bias = torch.randint(-64, 65, (N,), generator=g).float() * 0.25
    ops = (pack(ca, fmt), sa, pack(cw, "fp4"), sw)
    ref, _ = reference(*ops, fmt)
    assert float(ref.abs().max()) < 2.0 ** 17
    return tuple(t.cuda() for t in ops), bias.cuda(), ref


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("M,N,cu_budget,blocks", TILES)
@pytest.mark.parametrize("K", KS)
def test_integer_regime_exact(hip, M, N, cu_budget, blocks, K, fmt):
    assert hip.gemm_mx_workgroups(M, N, K, cu_budget) == blocks
    ops, bias, ref = integer_case(M, N, K, fmt)
    if K >= 256:
        # many outputs really need the rounding: they are not bf16 values
        inexact = (ref.to(torch.float32).to(BF).to(torch.float64) != ref).sum().item()
        assert inexact > M * N // 8, inexact
    for relu, use_bias in ACTS:
        v = ref + bias.cpu().double() if use_bias else ref
        exp = to_bf16_exact(v)
        if relu:
            exp = torch.where(exp > 0, exp, torch.zeros_like(exp))
        out = run(ops, fmt, cu_budget, bias=bias if use_bias else None, relu=relu)
        same(out, exp, f"integer {fmt} {M}x{N}x{K} relu={relu} bias={use_bias}")


# ------------------------------------------------------------------------------------------------ code and scale tables
def one_hot(rows, K, fmt, code, block_of_row=None):
    """Row r: `code` at position r % 32 of block block_of_row(r) (block 0 when None), zeros elsewhere."""
    c = torch.zeros(rows, K, dtype=torch.int64)
    r = torch.arange(rows)
    blk = torch.zeros(rows, dtype=torch.int64) if block_of_row is None else block_of_row
    c[r, blk * 32 + r % 32] = code
    return c


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_element_code_against_a_one_hot_partner(hip, fmt):
    K = 128
    unit = torch.full((256, 4), 127, dtype=U8)
    # A side: row m holds code m (fp8: all 256 bytes but the two NaN codes; fp4: m % 16) in all of block 0;
    # W row n is 1.0 (fp4 code 2) at position n % 32: out[m, n] = value(m), whatever the position
    codes = torch.arange(256)
    if fmt == "fp8":
        codes = torch.where((codes & 0x7F) == 0x7F, torch.zeros_like(codes), codes)
        vals = codes.to(U8).view(loadgen.FP8).to(torch.float64)
    else:
        codes = codes % 16
        vals = torch.where(codes >= 8, -FP4_VALUES[codes % 8], FP4_VALUES[codes % 8])
    ca = torch.zeros(256, K, dtype=torch.int64)
    ca[:, :32] = codes.view(256, 1)
    ops = (pack(ca, fmt), unit, pack(one_hot(64, K, "fp4", 2), "fp4"), unit[:64])
    out = run(ops, fmt)
    same(out, vals.view(256, 1).expand(256, 64).to(BF), f"A codes {fmt}")
    # W side: row n holds fp4 code n % 16 in all of block 0; A row m is 1.0 at position m % 32
    cw = torch.zeros(64, K, dtype=torch.int64)
    cw[:, :32] = (torch.arange(64) % 16).view(64, 1)
    wv = torch.where(torch.arange(64) % 16 >= 8, -FP4_VALUES[torch.arange(64) % 8], FP4_VALUES[torch.arange(64) % 8])
    one = 0x38 if fmt == "fp8" else 2
    ops = (pack(one_hot(64, K, fmt, one), fmt), unit[:64], pack(cw, "fp4"), unit[:64])
    out = run(ops, fmt)
    same(out, wv.view(1, 64).expand(64, 64).to(BF), f"W codes {fmt}")


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("side", ["a", "w"])
def test_every_scale_byte_with_a_partner(hip, fmt, side):
    """Row r of the tested side is one-hot (1.5) in block r with scale byte clamp(r, 1, 254); the partner rows hold 3.0
    at position r % 32 of every block r, with the byte that brings the total exponent to d = row % 17 - 8 (clamped into
    1 .. 254, which keeps the total inside [-8, 8]): one non-zero product per output, 4.5 * 2^total."""
    R, P, K = 256, 64, 256 * 32
    byte = torch.arange(R).clamp(1, 254)
    d = torch.arange(P) % 17 - 8
    partner = (254 - byte.view(1, R) + d.view(P, 1)).clamp(1, 254)      # [P, R]: per partner row and block
    total = byte.view(1, R) + partner - 254
    assert int(total.min()) >= -8 and int(total.max()) <= 8
    a_one = 0x3C if fmt == "fp8" else 3                                  # 1.5
    a_three = 0x44 if fmt == "fp8" else 5                                # 3.0
    tested = torch.full((R, R), 127, dtype=torch.int64)
    tested[torch.arange(R), torch.arange(R)] = byte
    pos = torch.arange(R) * 32 + torch.arange(R) % 32
    cp = torch.zeros(P, K, dtype=torch.int64)
    if side == "a":
        cp[:, pos] = 5
        ops = (pack(one_hot(R, K, fmt, a_one, torch.arange(R)), fmt), tested.to(U8), pack(cp, "fp4"), partner.to(U8))
        exp = (4.5 * torch.exp2(total.double())).t()                    # [R, P]
    else:
        cp[:, pos] = a_three
        ops = (pack(cp, fmt), partner.to(U8), pack(one_hot(R, K, "fp4", 3, torch.arange(R)), "fp4"), tested.to(U8))
        exp = 4.5 * torch.exp2(total.double())                          # [P, R]
    ref, _ = reference(*ops, fmt)
    assert torch.equal(ref, exp)
    same(run(ops, fmt), to_bf16_exact(exp), f"scale bytes on {side}, {fmt} activations")


@pytest.mark.parametrize("fmt", FORMATS)
def test_zero_block_with_scale_byte_zero_contributes_nothing(hip, fmt):
    (a_q, a_s, w_q, w_s), _, _ = integer_case(128, 192, 384, fmt)
    a_q, a_s, w_q, w_s = a_q.clone(), a_s.clone(), w_q.clone(), w_s.clone()
    ab, wb = (32 if fmt == "fp8" else 16), 16                           # bytes of a block
    a_q.view(U8)[:, 2 * ab:3 * ab] = 0                                  # block 2 of every A row: zeros under byte 0
    a_s[:, 2] = 0
    w_q[:, 7 * wb:8 * wb] = 0                                           # block 7 of every W row
    w_s[:, 7] = 0
    a_q.view(U8)[64:, 5 * ab:6 * ab] = 0                                # padding-like rows: several zero blocks
    a_s[64:, 5] = 0
    ref, _ = reference(a_q, a_s, w_q, w_s, fmt)
    same(run((a_q, a_s, w_q, w_s), fmt), to_bf16_exact(ref), f"zero blocks {fmt}")


@pytest.mark.parametrize("fmt", FORMATS)
def test_scale_bytes_outside_the_contract_are_printed(hip, fmt):
    """Byte 0 under non-zero elements and byte 255: printed for the MEASURED block, not asserted."""
    K = 128
    unit = torch.full((64, 4), 127, dtype=U8)
    one = 0x38 if fmt == "fp8" else 2
    w = pack(one_hot(64, K, "fp4", 2), "fp4")
    a = pack(one_hot(64, K, fmt, one), fmt)
    for name, sa, sw in (("a byte 0, w byte 254", 0, 254), ("a byte 0, w byte 127", 0, 127), ("a byte 255", 255, 127),
                         ("w byte 255", 127, 255), ("w byte 0, a byte 254", 254, 0)):
        s_a, s_w = unit.clone(), unit.clone()
        s_a[:, 0], s_w[:, 0] = sa, sw
        out = run((a, s_a, w, s_w), fmt).cpu().double()
        print(f"gemm_mx {fmt} activations, {name}: products {sorted(set(out[torch.arange(32), torch.arange(32)].tolist()))}, "
              f"2^(sa + sw - 254) = {2.0 ** (sa + sw - 254) if 255 not in (sa, sw) else 'NaN'}")


# ------------------------------------------------------------------------------------------------ the true regime
@functools.lru_cache(maxsize=None)
def true_case(M, N, K, fmt):
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g).to(BF)
    w = (torch.randn(N, K, generator=g) * 0.05).to(BF)
    a_q, a_s = loadgen.quantize_mx_reference(a, fmt)
    w_q, w_s = loadgen.quantize_mx_reference(w, "fp4")
    ref, mag = reference(a_q, a_s, w_q, w_s, fmt)
    return (a_q.cuda(), a_s.cuda(), w_q.cuda(), w_s.cuda()), ref, mag


@pytest.mark.parametrize("fmt", FORMATS)
def test_true_regime_within_the_derived_bound(hip, fmt):
    worst = 0.0
    for M, N, cu_budget in ((128, 192, 0), (256, 256, 4)):
        for K in KS:
            ops, ref, mag = true_case(M, N, K, fmt)
            out = run(ops, fmt, cu_budget).cpu().double()
            bound = 2.0 ** -8 * ref.abs() + (1 + 2.0 ** -8) * K * 2.0 ** -23 * mag
            ratio = ((out - ref).abs() / bound).max().item()
            worst = max(worst, ratio)
            assert ratio <= 1.0, (fmt, M, N, K, ratio)
    print(f"gemm_mx true regime, {fmt} activations: max |out - ref| / bound = {worst:.4f}")


# ------------------------------------------------------------------------------------------------ strides
def padded(t: torch.Tensor, pad: int, c0: int, fill: int) -> torch.Tensor:
    """A copy of the byte matrix t as a window of a `fill`-filled allocation with `pad` more columns."""
    rows, cols = t.shape
    big = torch.full((rows + 3, cols + pad), fill, dtype=U8, device="cuda")
    big[1:1 + rows, c0:c0 + cols] = t.view(U8)
    return big[1:1 + rows, c0:c0 + cols].view(t.dtype)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("M,N,cu_budget,blocks", TILES)
def test_padded_operands_and_guarded_output(hip, M, N, cu_budget, blocks, fmt):
    K = 384
    (a_q, a_s, w_q, w_s), bias, ref = integer_case(M, N, K, fmt)
    # element rows stay 16-byte aligned (padding and offset multiples of 16); the fill is fp8's NaN / fp4's -6, -6;
    # scale rows get odd strides and offsets, filled with byte 255
    ops = (padded(a_q, 48, 16, 0x7F if fmt == "fp8" else 0xFF), padded(a_s, 5, 3, 255), padded(w_q, 32, 16, 0xFF),
           padded(w_s, 7, 2, 255))
    assert ops[1].stride(0) % 2 == 1 and ops[3].stride(0) % 2 == 1
    ld, c0 = N + 12, 4                                                   # 8-byte aligned C rows
    raw = torch.full((2 + M + 3, ld), SENT16, dtype=torch.int16, device="cuda")
    view = raw.view(BF)[2:2 + M, c0:c0 + N]
    for relu, use_bias in ((False, False), (True, True)):
        raw.fill_(SENT16)
        out = run(ops, fmt, cu_budget, bias=bias if use_bias else None, relu=relu, out=view)
        assert out is view
        exp = to_bf16_exact(ref + bias.cpu().double() if use_bias else ref)
        if relu:
            exp = torch.where(exp > 0, exp, torch.zeros_like(exp))
        same(view, exp, f"padded {fmt} {M}x{N}")
        assert guards_intact(raw, (slice(2, 2 + M), slice(c0, c0 + N)), SENT16)


@pytest.mark.parametrize("fmt", FORMATS)
def test_launches_repeat_bit_for_bit(hip, fmt):
    ops, _, _ = true_case(256, 256, 640, fmt)
    first = run(ops, fmt, 4).view(torch.int16).clone()
    for _ in range(2):
        assert torch.equal(run(ops, fmt, 4).view(torch.int16), first)
