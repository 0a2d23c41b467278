"""The MX operands without a GPU: the quantisation rule's CPU reference (ops.loadgen.quantize_mx_reference /
dequantize_mx_reference) against torch's own fp8 cast and a brute-force fp4 search, crafted scale and tie cases, the
"quant_mx" / "gemm_mx" op kinds and the LLM_MX table written out literally, the executor's rows, and every ValueError
of the two wrappers (which must fire before any native call)."""
import math

import pytest
import torch

from k8s_gpu_scheduler_amd import _native
from k8s_gpu_scheduler_amd.models import workloads as W
from k8s_gpu_scheduler_amd.ops import loadgen
from k8s_gpu_scheduler_amd.parallel import executor

BF = torch.bfloat16
FORMATS = ("fp8", "fp4")
EMAX = {"fp8": 8, "fp4": 2}
FMAX = {"fp8": 448.0, "fp4": 6.0}
FP4_MAGS = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def all_patterns() -> torch.Tensor:
    """All 65,536 bf16 patterns as [64, 1024]: 2,048 blocks of 32 consecutive patterns."""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF).view(64, 1024)


def codes(q: torch.Tensor, fmt: str) -> torch.Tensor:
    """One element code per element, int64 [rows, K]."""
    b = q.view(torch.uint8).to(torch.int64)
    if fmt == "fp8":
        return b
    return torch.stack((b & 0xF, b >> 4), dim=2).reshape(b.shape[0], -1)


def block(values, fill=0.0) -> torch.Tensor:
    """One bf16 row of 32: the given values, then `fill`."""
    v = list(values) + [fill] * (32 - len(values))
    return torch.tensor([v], dtype=torch.float64).to(BF)


# ------------------------------------------------------------------------------------------------ the reference
def test_reference_scale_bytes_on_all_patterns():
    x = all_patterns()
    e = ((x.view(torch.int16).to(torch.int64) & 0xFFFF) >> 7 & 0xFF).view(64, 32, 32).amax(dim=2)
    for fmt in FORMATS:
        q, s = loadgen.quantize_mx_reference(x, fmt)
        assert s.dtype == torch.uint8 and tuple(s.shape) == (64, 32)
        want = torch.where(e == 255, torch.full_like(e, 255), (e - EMAX[fmt]).clamp(min=0))
        assert torch.equal(s.to(torch.int64), want)
        assert int((s == 255).sum()) == 8                               # the Inf / NaN blocks of both signs
        assert int((s == 0).sum()) == {"fp4": 24, "fp8": 72}[fmt]
        assert int(s[s != 255].max()) <= 253
        # a non-finite block is all-zero bytes
        dead = (s == 255).repeat_interleave(32, dim=1)
        assert int(codes(q, fmt)[dead].abs().sum()) == 0


def scaled_exact(x: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """v * 2^(127 - b) in float64 (exact), NaN blocks dropped to 0."""
    f = torch.ldexp(torch.ones((), dtype=torch.float64), 127 - s.to(torch.int64).clamp(max=253))
    v = x.to(torch.float64) * f.repeat_interleave(32, dim=1)
    return torch.where(torch.isfinite(v), v, torch.zeros_like(v))


def test_reference_fp8_elements_are_torchs_cast_of_the_clamped_rescaled_value():
    x = all_patterns()
    q, s = loadgen.quantize_mx_reference(x, "fp8")
    assert q.dtype == loadgen.FP8 and tuple(q.shape) == (64, 1024)
    live = (s != 255).repeat_interleave(32, dim=1)
    v = scaled_exact(x, s)
    assert float(v.abs().max()) < 512.0                                 # below 2^(emax + 1)
    # exact in fp32 wherever it matters: an fp32 subnormal is far below half of e4m3's smallest step, 2^-10
    want = v.clamp(-448.0, 448.0).to(torch.float32).to(loadgen.FP8).view(torch.uint8).to(torch.int64)
    sign = (x.view(torch.int16).to(torch.int64) >> 15) & 1
    want = (want & 0x7F) | (sign << 7)                                  # the input's sign bit, also on a zero
    got = codes(q, "fp8")
    assert torch.equal(got[live], want[live])
    assert int(((got & 0x7F) == 0x7F).sum()) == 0                       # never the NaN code
    assert int(((got & 0x7F) == 0x7E)[live].sum()) > 0                  # saturation is reached


def test_reference_fp4_elements_are_the_nearest_even_magnitude():
    x = all_patterns()
    q, s = loadgen.quantize_mx_reference(x, "fp4")
    assert q.dtype == torch.uint8 and tuple(q.shape) == (64, 512)
    live = (s != 255).repeat_interleave(32, dim=1)
    v = scaled_exact(x, s).abs()
    mags = torch.tensor(FP4_MAGS, dtype=torch.float64)
    d = (v.unsqueeze(-1) - mags).abs()                                  # [64, 1024, 8], exact in float64
    best = d.min(dim=-1).values
    near = d == best.unsqueeze(-1)                                      # one or two candidates
    idx = torch.arange(8)
    lo = torch.where(near, idx, 8).min(dim=-1).values
    hi = torch.where(near, idx, -1).max(dim=-1).values
    # a tie goes to the even code (mantissa bit 0); past 6 the nearest is 6
    want = torch.where(lo == hi, lo, torch.where(lo % 2 == 0, lo, hi))
    sign = (x.view(torch.int16).to(torch.int64) >> 15) & 1
    got = codes(q, "fp4")
    assert torch.equal(got[live], (want | (sign << 3))[live])
    assert int((lo != hi)[live].sum()) > 0                              # ties exist among the patterns


@pytest.mark.parametrize("fmt", FORMATS)
def test_reference_scale_bytes_for_crafted_amax(fmt):
    emax = EMAX[fmt]
    rows, want = [], []
    for e in range(-126, 128):                                          # 2^e, and just below it
        rows.append(block([2.0 ** e, -(2.0 ** e) / 4]))
        want.append(max(e + 127 - emax, 0))
        below = torch.tensor([[2.0 ** e]], dtype=torch.float64).to(BF).view(torch.int16) - 1      # the pattern before 2^e
        r = block([0.0])
        r[0, 5] = below.view(BF)[0, 0]
        rows.append(r)
        want.append(max(e - 1 + 127 - emax, 0))
    rows += [block([2.0 ** -130, 2.0 ** -133]), block([0.0]), block([-0.0] * 32), block([float("inf"), 1.0]),
             block([1.0, float("-inf")]), block([3.0, float("nan")])]
    want += [0, 0, 0, 255, 255, 255]
    x = torch.cat(rows, dim=0)
    q, s = loadgen.quantize_mx_reference(x, fmt)
    assert s[:, 0].tolist() == want
    assert int(codes(q, fmt)[-3:].sum()) == 0                           # the non-finite blocks: 0x00 bytes
    neg0 = 0x80 if fmt == "fp8" else 0x8
    assert codes(q, fmt)[-4].tolist() == [neg0] * 32                    # -0.0 keeps its sign
    # 2^e itself: the amax of its block lands on 2^emax (code of 1.0 * 2^emax), or below it where b was clamped to 0
    top = codes(q, fmt)[0::2][:254, 0]
    one_at_emax = {"fp8": (8 + 7) << 3, "fp4": (2 + 1) << 1}[fmt]
    assert top[emax + 126:].tolist() == [one_at_emax] * (254 - emax - 126)


@pytest.mark.parametrize("shift", [-40, -1, 0, 3, 60])
def test_reference_hand_written_fp4_cases(shift):
    k = 2.0 ** shift
    # amax 4 (exponent 2) pins b = 127 + shift: elements are the values divided by k
    vals = [4.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -0.75, -5.0, 0.26, 0.24, -0.0, 0.0, 2.0 ** -20, -(2.0 ** -20)]
    want = [6, 0, 2, 2, 4, 4, 6, 6, 0x8, 0xA, 0xE, 1, 0, 0x8, 0, 0, 0x8]
    #       4  ties to the even code: 0.25->0  0.75->1  1.25->1  1.75->2  2.5->2  3.5->4  5->4
    q, s = loadgen.quantize_mx_reference(block([v * k for v in vals]), "fp4")
    assert int(s[0, 0]) == 127 + shift
    assert codes(q, "fp4")[0, :len(vals)].tolist() == want
    # saturation: amax 7.5 (exponent 2) stays in the block, 6.5 and 7 too
    q, s = loadgen.quantize_mx_reference(block([7.5 * k, 6.5 * k, -7.0 * k, 6.0 * k]), "fp4")
    assert int(s[0, 0]) == 127 + shift and codes(q, "fp4")[0, :4].tolist() == [7, 7, 0xF, 7]


@pytest.mark.parametrize("shift", [-40, 0, 60])
def test_reference_hand_written_fp8_cases(shift):
    k = 2.0 ** shift
    # amax 256 (exponent 8) pins b = 127 + shift; e4m3: 1.0 = 0x38, step 2^-3 there; smallest step 2^-9
    vals = [256.0, 1.0625, 1.1875, 17.0, 19.0, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -10 * 1.5, -(2.0 ** -10), 2.0 ** -6 - 2.0 ** -11,
            -0.0, 2.0 ** -30, -(2.0 ** -30)]
    want = [0x78, 0x38, 0x3A, 0x58, 0x5A, 0x00, 0x02, 0x01, 0x80, 0x08, 0x80, 0x00, 0x80]
    #       256   ties: 1.0625 -> 1.0, 1.1875 -> 1.25, 17 -> 16, 19 -> 20; 2^-10 -> 0, 3 * 2^-10 -> 2 * 2^-9 (even);
    #       1.5 * 2^-10 -> 2^-9; a negative that rounds to zero keeps its sign; 2^-6 - 2^-11 rounds up into the first normal
    q, s = loadgen.quantize_mx_reference(block([v * k for v in vals]), "fp8")
    assert int(s[0, 0]) == 127 + shift
    assert codes(q, "fp8")[0, :len(vals)].tolist() == want
    q, s = loadgen.quantize_mx_reference(block([496.0 * k, 464.0 * k, -480.0 * k, 448.0 * k, 400.0 * k]), "fp8")
    assert int(s[0, 0]) == 127 + shift and codes(q, "fp8")[0, :5].tolist() == [0x7E, 0x7E, 0xFE, 0x7E, 0x7C]


def test_reference_underflow_beside_a_huge_amax():
    big = 2.0 ** 120
    for fmt, zero_neg in (("fp8", 0x80), ("fp4", 0x8)):
        q, s = loadgen.quantize_mx_reference(block([big, 1.0, -1.0, 2.0 ** -126, -(2.0 ** -133)]), fmt)
        assert int(s[0, 0]) == 247 - EMAX[fmt]
        assert codes(q, fmt)[0, 1:5].tolist() == [0, zero_neg, 0, zero_neg]


@pytest.mark.parametrize("fmt", FORMATS)
def test_reference_is_idempotent_and_dequantises_exactly(fmt):
    g = torch.Generator().manual_seed(7)
    for x in (all_patterns(), torch.randn(16, 256, generator=g).to(BF)):
        q, s = loadgen.quantize_mx_reference(x, fmt)
        d = loadgen.dequantize_mx_reference(q, s, fmt)
        assert d.dtype == torch.float64 and d.shape == x.shape
        live = (s != 255).repeat_interleave(32, dim=1)
        assert torch.isnan(d[~live]).all() and torch.isfinite(d[live]).all()
        back = torch.where(live, d, torch.zeros_like(d)).to(BF)
        assert torch.equal(back.to(torch.float64)[live], d[live])       # every dequantised value is a bf16 value
        q2, s2 = loadgen.quantize_mx_reference(back, fmt)
        blocks_live = s != 255
        # a block whose elements all became zero re-quantises with b = 0: compare the values, and the bytes of the rest
        d2 = loadgen.dequantize_mx_reference(q2, s2, fmt)
        assert torch.equal(d2[live], d[live])
        same_scale = blocks_live & (s2 == s)
        keep = same_scale.repeat_interleave(32, dim=1)
        assert torch.equal(codes(q2, fmt)[keep], codes(q, fmt)[keep])
        moved = blocks_live & (s2 != s)
        amax = d.abs().view(x.shape[0], -1, 32).amax(dim=2)
        assert bool((amax[moved] < 2.0 ** (s[moved].to(torch.float64) - 127 + EMAX[fmt])).all())     # only where amax rounded down


def test_reference_randn_error_and_saturation():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(512, 1024, generator=g).to(BF)
    ref = x.to(torch.float64)
    for fmt, want in (("fp4", 0.114), ("fp8", 0.029)):
        q, s = loadgen.quantize_mx_reference(x, fmt)
        d = loadgen.dequantize_mx_reference(q, s, fmt)
        rel = float(((d - ref).pow(2).mean() / ref.pow(2).mean()).sqrt())
        assert abs(rel - want) < 0.004, (fmt, rel)
    q, s = loadgen.quantize_mx_reference(x, "fp4")
    sat = float((scaled_exact(x, s).abs() > 6.0).double().mean())       # the elements the clamp at 6 changes
    assert 0.018 < sat < 0.028, sat


def test_reference_rejects_what_it_cannot_quantise():
    with pytest.raises(ValueError, match="fmt"):
        loadgen.quantize_mx_reference(torch.zeros(1, 32, dtype=BF), "fp6")
    with pytest.raises(ValueError, match="multiple of 32"):
        loadgen.quantize_mx_reference(torch.zeros(1, 48, dtype=BF), "fp8")
    with pytest.raises(ValueError, match="bf16"):
        loadgen.quantize_mx_reference(torch.zeros(1, 32), "fp8")
    with pytest.raises(ValueError, match="do not match"):
        loadgen.dequantize_mx_reference(torch.zeros(2, 32, dtype=torch.uint8), torch.zeros(2, 1, dtype=torch.uint8), "fp4")
    d = loadgen.dequantize_mx_reference(torch.tensor([[0x21] * 16], dtype=torch.uint8), torch.tensor([[128]], dtype=torch.uint8), "fp4")
    assert d[0, :4].tolist() == [1.0, 2.0, 1.0, 2.0]                    # element 2i in the LOW nibble of byte i


# ------------------------------------------------------------------------------------------------ ops and tables
def test_op_costs_of_the_two_kinds():
    q8, q4 = W.Op("quant_mx", 256, 4096, fmt="fp8"), W.Op("quant_mx", 2048, 14336, fmt="fp4")
    assert q8.flops == 5.0 * 256 * 4096 and q4.flops == 5.0 * 2048 * 14336
    assert q8.bytes == 2 * 256 * 4096 + 256 * 4096 + 256 * 4096 / 32
    assert q4.bytes == 2 * 2048 * 14336 + 2048 * 14336 / 2 + 2048 * 14336 / 32
    assert not q8.on_mfma and not q8.is_gemm and q8.mfma_rate() == 1.0
    assert q8.workgroups(0) == 128 and q4.workgroups(64) == 3584
    assert W.default_quantize_mx_workgroups(1, 32) == 1 and W.default_quantize_mx_workgroups(0, 32) == 0
    assert W.default_quantize_mx_workgroups(3, 8192 + 32) == 4
    g8, g4 = W.Op("gemm_mx", 256, 6144, 4096, relu=False, fmt="fp8"), W.Op("gemm_mx", 2048, 4096, 14336, relu=False, fmt="fp4")
    assert g8.flops == 2.0 * 256 * 6144 * 4096 and g4.flops == 2.0 * 2048 * 4096 * 14336
    assert g8.bytes == (1 + 1 / 32) * 256 * 4096 + (0.5 + 1 / 32) * 6144 * 4096 + 2 * 256 * 6144
    assert g4.bytes == (0.5 + 1 / 32) * 2048 * 14336 + (0.5 + 1 / 32) * 4096 * 14336 + 2 * 2048 * 4096
    assert g8.on_mfma and g4.on_mfma and not g8.is_gemm
    assert g8.mfma_rate() == 2.0 and g4.mfma_rate() == 4.0
    for o in (g8, g4):
        for budget in (0, 4, 64, 256):
            assert o.workgroups(budget) == W.default_gemm_workgroups(o.M, o.N, o.K, budget, fp8=True)
    assert g8.workgroups(0) == 384 and g4.workgroups(0) == 512 and W.Op("gemm_mx", 256, 256, 128, fmt="fp4").workgroups(4) == 4
    assert W.Op("gemm", 64, 64, 64).fmt == ""                           # the new field has a default
    # 0.27 of the bf16 weight bytes
    assert abs((0.5 + 1 / 32) / 2 - 0.2656) < 1e-4


def test_llm_mx_table_written_out():
    def ops(r, f, append, attention):
        def qg(N, K):
            return [W.Op("quant_mx", r, K, fmt=f), W.Op("gemm_mx", r, N, K, relu=False, fmt=f)]
        return tuple([W.Op("add_rmsnorm", r, 4096)] + qg(6144, 4096) + [append, attention] + qg(4096, 4096)
                     + [W.Op("add_rmsnorm", r, 4096)] + qg(28672, 4096) + [W.Op("swiglu", r, 14336)] + qg(4096, 14336))
    dec = W.Workload("llm_mx_block_decode_256", "llm_mx_block_decode", "hip", 256,
                     ops(256, "fp8", W.Op("rope_append", 256, 32, 1024, rows=8, q=1), W.Op("attn", 256, 32, 1024, rows=8)), 2.25)
    pre = W.Workload("llm_mx_block_prefill_2048", "llm_mx_block_prefill", "hip", 2048,
                     ops(2048, "fp4", W.Op("rope_append", 2, 32, 4096, rows=8, q=1024),
                         W.Op("prefill", 2, 32, 4096, rows=8, q=1024)), 1.0)
    assert W.LLM_MX == {"llm_mx_block_decode_256": dec, "llm_mx_block_prefill_2048": pre}
    # the same block as LLM_BLOCK with every projection replaced by the pair
    for mx, bf in (("llm_mx_block_decode_256", "llm_block_decode_256"), ("llm_mx_block_prefill_2048", "llm_block_prefill_2048")):
        want = []
        for o in W.LLM_BLOCK[bf].ops:
            f = W.LLM_MX[mx].ops[1].fmt
            want += [W.Op("quant_mx", o.M, o.K, fmt=f), W.Op("gemm_mx", o.M, o.N, o.K, relu=False, fmt=f)] if o.kind == "gemm" else [o]
        assert W.LLM_MX[mx].ops == tuple(want)
    assert not set(W.LLM_MX) & set(W.EXTRA)
    for w in W.LLM_MX.values():
        assert W.get(w.name) is w
        assert W.workload_for_pod(f"pod-{w.name.replace('_', '-')}-17") is w
        assert W.roofline_seconds(w, 1.0) > 0 and 0 < W.cu_fill(w) <= 1


def _declared_bytes(w: W.Workload) -> float:
    """What executor._Buffers allocates for the workload, from the operand layouts of its OP_KINDS rows."""
    total = 0.0
    for o in w.ops:
        if o.kind == "add_rmsnorm":
            total += 4 * 2 * o.M * o.N + 2 * o.N
        elif o.kind == "swiglu":
            total += 2 * o.M * 3 * o.N
        elif o.kind == "quant_mx":
            total += o.bytes
        elif o.kind == "gemm_mx":
            total += o.bytes + 4 * o.N
        elif o.kind in ("attn", "prefill", "rope_append"):
            rows = o.M * (o.q or 1)
            total += 2 * 2 * o.M * o.K * o.rows * 128 + 2 * 2 * rows * o.N * 128            # caches, q / out
            if o.kind == "rope_append":
                total += 2 * rows * 2 * o.rows * 128 + 4 * 128 * o.K                          # the K / V part of qkv, cos_sin
        else:
            raise AssertionError(o)
    return total


def test_llm_mx_declared_footprints_cover_the_operands():
    for w in W.LLM_MX.values():
        gib = _declared_bytes(w) / 2 ** 30
        assert gib <= w.hbm_gib < gib + 0.25, (w.name, gib)


def test_new_names_change_no_existing_lookup():
    tables = (W.CATALOG, W.EXTRA, W.STAGED, W.LONG_CONTEXT, W.LLM_LAYER, W.LLM_BLOCK, W.LLM_HEAD, W.LLM_MOE)
    old = [n for t in tables for n in t]
    for new in W.LLM_MX:
        assert not any(o in new for o in old), new                      # an older name would win the lookup of a new pod
        assert not any(new in o for o in old), new
    assert not any(a != b and a in b for a in W.LLM_MX for b in W.LLM_MX)
    for t in tables:
        for n, w in t.items():
            assert W.workload_for_pod(f"x-{n.replace('_', '-')}-0").name in (n, W.workload_for_pod(n).name)
            assert W.get(n) is w


def test_op_kinds_rows_build_operands_on_the_cpu():
    assert executor.OP_KINDS["quant_mx"][2] == 0 and executor.OP_KINDS["gemm_mx"][2] == 0
    assert {o.kind for w in W.LLM_MX.values() for o in w.ops} <= set(executor.OP_KINDS)
    ops = (W.Op("quant_mx", 5, 96, fmt="fp8"), W.Op("quant_mx", 3, 64, fmt="fp4"),
           W.Op("gemm_mx", 64, 320, 256, relu=False, fmt="fp8"), W.Op("gemm_mx", 320, 64, 128, relu=False, fmt="fp4"))
    w = W.Workload("mx_rows", "pin", "hip", 64, ops, 0.1)
    bufs = executor._Buffers(w, torch.device("cpu"))
    again = executor._Buffers(w, torch.device("cpu"))
    (_, t0), (_, t1), (_, t2), (_, t3) = bufs.ops
    q, s, x = t0
    assert (q.dtype, tuple(q.shape), s.dtype, tuple(s.shape), x.dtype, tuple(x.shape)) == \
        (loadgen.FP8, (5, 96), torch.uint8, (5, 3), BF, (5, 96))
    assert tuple(t1[0].shape) == (3, 32) and t1[0].dtype == torch.uint8 and tuple(t1[1].shape) == (3, 2)
    for (o, t), (_, u) in zip(bufs.ops[2:], again.ops[2:]):
        c, a_q, a_s, w_q, w_s, bias = t
        assert executor.op_output(o, t) is c and c.dtype == BF and tuple(c.shape) == (o.M, o.N)
        assert a_q.dtype == loadgen.mx_element_dtype(o.fmt) and tuple(a_q.shape) == (o.M, loadgen.mx_row_bytes(o.fmt, o.K))
        assert w_q.dtype == torch.uint8 and tuple(w_q.shape) == (o.N, o.K // 2)
        assert tuple(a_s.shape) == (o.M, o.K // 32) and tuple(w_s.shape) == (o.N, o.K // 32)
        for sc in (a_s, w_s):
            assert sc.dtype == torch.uint8 and 120 <= int(sc.min()) and int(sc.max()) <= 127
        if o.fmt == "fp8":
            assert int(((a_q.view(torch.uint8) & 0x7F) == 0x7F).sum()) == 0          # no fp8 NaN code
            assert len(a_q.view(torch.uint8).unique()) > 200
        assert bias.dtype == torch.float32 and float(bias.abs().sum()) == 0.0
        assert all(torch.equal(p.view(torch.uint8), r.view(torch.uint8)) for p, r in zip(t[1:], u[1:]))      # seeded
        big = w_q if o.N > executor.MX_PATTERN_ROWS else a_q                       # 320 rows repeat a block of 256
        assert torch.equal(big.view(torch.uint8)[256:320], big.view(torch.uint8)[:64])
        d = loadgen.dequantize_mx_reference(a_q, a_s, o.fmt)
        assert torch.isfinite(d).all()

    calls = []
    saved = loadgen.quantize_mx, loadgen.gemm_mx
    loadgen.quantize_mx = lambda x, fmt, **kw: calls.append(("q", fmt, sorted(kw)))
    loadgen.gemm_mx = lambda *a, **kw: calls.append(("g", a[4], kw["relu"], kw["cu_budget"], sorted(kw)))
    try:
        executor.enqueue_ops(bufs, 1, "st", 64)
    finally:
        loadgen.quantize_mx, loadgen.gemm_mx = saved
    assert calls == [("q", "fp8", ["out", "scales", "stream"]), ("q", "fp4", ["out", "scales", "stream"]),
                     ("g", "fp8", False, 64, ["bias", "cu_budget", "out", "relu", "stream"]),
                     ("g", "fp4", False, 64, ["bias", "cu_budget", "out", "relu", "stream"])]


@pytest.mark.skipif(_native.hip(required=False) is None, reason="HIP extension not built")
def test_default_workgroups_match_the_native_rules():
    h = _native.hip()
    assert (h.MX_FP8, h.MX_FP4) == (0, 4)
    for T, D in ((0, 32), (1, 32), (5, 96), (67, 4096), (256, 4096), (2048, 14336), (8192, 8192), (3, 8224)):
        assert h.quantize_mx_workgroups(T, D) == W.default_quantize_mx_workgroups(T, D), (T, D)
    for bad in ((1, 0), (1, 48), (-1, 32)):
        with pytest.raises(RuntimeError):
            h.quantize_mx_workgroups(*bad)
    for M, N, K in ((64, 64, 128), (128, 192, 384), (256, 256, 640), (256, 6144, 4096), (2048, 28672, 4096),
                    (2048, 4096, 14336), (4096, 4096, 4096), (8192, 8192, 8192)):
        for budget in (0, 4, 32, 64, 128, 256):
            assert h.gemm_mx_workgroups(M, N, K, budget) == W.default_gemm_mx_workgroups(M, N, K, budget), (M, N, K, budget)
            assert h.gemm_mx_workgroups(M, N, K, budget) == h.gemm_workgroups(M, N, K, budget, True, False)
    for bad in ((64, 64, 64), (32, 64, 128), (64, 0, 128)):
        with pytest.raises(RuntimeError):
            h.gemm_mx_workgroups(*bad, 0)


# ------------------------------------------------------------------------------------------------ the wrappers
@pytest.fixture
def no_native(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the native module was touched")
    monkeypatch.setattr(_native, "hip", boom)


@pytest.fixture
def host_operands_pass(monkeypatch, no_native):
    """The checks after the device check run on host tensors once it is stubbed out."""
    monkeypatch.setattr(loadgen, "_check_devices", lambda name, *ts: torch.device("cpu"))


def test_wrappers_reject_cpu_tensors(no_native):
    with pytest.raises(ValueError, match="quantize_mx expects device tensors"):
        loadgen.quantize_mx(torch.zeros(2, 32, dtype=BF), "fp8")
    a, s = torch.zeros(64, 128, dtype=torch.uint8).view(loadgen.FP8), torch.zeros(64, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="gemm_mx expects device tensors"):
        loadgen.gemm_mx(a, s, torch.zeros(64, 64, dtype=torch.uint8), s, "fp8")
    with pytest.raises(ValueError, match="fmt = 'fp6'"):                # before anything else
        loadgen.quantize_mx(torch.zeros(2, 32, dtype=BF), "fp6")
    with pytest.raises(ValueError, match="fmt = 'bf16'"):
        loadgen.gemm_mx(a, s, a, s, "bf16")


def test_quantize_mx_value_errors(host_operands_pass):
    Q = loadgen.quantize_mx
    x = torch.zeros(4, 64, dtype=BF)
    for bad, msg in ((torch.zeros(4, 48, dtype=BF), "multiple of 32"), (torch.zeros(4, 0, dtype=BF), "multiple of 32"),
                     (torch.zeros(4, 64), "x must be bf16"), (torch.zeros(64, dtype=BF), "x must be 2-D"),
                     (torch.zeros(64, 4, dtype=BF).t(), "contiguous rows"),
                     (torch.zeros(4, 68, dtype=BF)[:, :64], "row stride 68"),
                     (torch.zeros(4 * 64 + 8, dtype=BF)[4:4 + 256].view(4, 64), "16-byte aligned")):
        with pytest.raises(ValueError, match=msg):
            Q(bad, "fp8")
    with pytest.raises(ValueError, match="out must be torch.float8_e4m3fn"):
        Q(x, "fp8", out=torch.zeros(4, 64, dtype=torch.uint8))
    with pytest.raises(ValueError, match="out must be torch.uint8"):
        Q(x, "fp4", out=torch.zeros(4, 32, dtype=torch.uint8).view(loadgen.FP8))
    with pytest.raises(ValueError, match=r"out must be \[4, 32\]"):
        Q(x, "fp4", out=torch.zeros(4, 64, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"out must be \[4, 32\]"):
        Q(x, "fp4", out=torch.zeros(3, 32, dtype=torch.uint8))
    with pytest.raises(ValueError, match="out must have contiguous rows"):
        Q(x, "fp4", out=torch.zeros(32, 4, dtype=torch.uint8).t())
    with pytest.raises(ValueError, match="out row stride"):
        Q(x, "fp4", out=torch.zeros(4, 32, dtype=torch.uint8).expand(4, 4, 32)[0].as_strided((4, 32), (16, 1)))
    with pytest.raises(ValueError, match="scales must be torch.uint8"):
        Q(x, "fp4", scales=torch.zeros(4, 2, dtype=torch.int8))
    with pytest.raises(ValueError, match=r"scales must be \[4, 2\]"):
        Q(x, "fp4", scales=torch.zeros(4, 3, dtype=torch.uint8))
    raw = torch.zeros(4 * 128 + 64, dtype=torch.uint8)
    xv = raw[:512].view(BF).view(4, 64)
    with pytest.raises(ValueError, match="out overlaps x"):
        Q(xv, "fp4", out=raw[384:512].view(4, 32))
    with pytest.raises(ValueError, match="scales overlaps x"):
        Q(xv, "fp4", scales=raw[504:512].view(4, 2))
    both = torch.zeros(4, 40, dtype=torch.uint8)
    with pytest.raises(ValueError, match="out overlaps scales"):       # in the gap a padded row stride leaves
        Q(x, "fp4", out=both[:, :32], scales=both[:, 32:34])
    with pytest.raises(ValueError, match="more than 2\\^31 - 1 rows"):
        Q(torch.empty(2 ** 31, 32, dtype=BF, device="meta"), "fp8")
    with pytest.raises(ValueError, match="more than 2\\^31 - 1 workgroups"):
        Q(torch.empty(2 ** 31 - 1, 32768, dtype=BF, device="meta"), "fp8")
    with pytest.raises(AssertionError, match="native module was touched"):
        Q(x, "fp8")                                                     # every check passed
    with pytest.raises(AssertionError, match="native module was touched"):     # odd row strides are legal for q and scales
        Q(x, "fp4", out=torch.zeros(4, 37, dtype=torch.uint8)[:, :32], scales=torch.zeros(4, 3, dtype=torch.uint8)[:, :2])
    q, s = Q(x[:0], "fp4")                                              # T == 0 launches nothing
    assert tuple(q.shape) == (0, 32) and q.dtype == torch.uint8 and tuple(s.shape) == (0, 2)
    q, s = Q(x[:0], "fp8")
    assert tuple(q.shape) == (0, 64) and q.dtype == loadgen.FP8


def _mx_args(M=64, N=64, K=128, fmt="fp8"):
    a = torch.zeros(M, loadgen.mx_row_bytes(fmt, K), dtype=torch.uint8).view(loadgen.mx_element_dtype(fmt))
    return [a, torch.zeros(M, K // 32, dtype=torch.uint8), torch.zeros(N, K // 2, dtype=torch.uint8),
            torch.zeros(N, K // 32, dtype=torch.uint8), fmt]


def test_gemm_mx_value_errors(host_operands_pass):
    G = loadgen.gemm_mx

    def bad(i, t, msg, fmt="fp8", **kw):
        args = _mx_args(fmt=fmt)
        args[i] = t
        with pytest.raises(ValueError, match=msg):
            G(*args, **kw)
    u8 = torch.uint8
    bad(0, torch.zeros(64, dtype=u8), "must be 2-D")
    bad(2, torch.zeros(64, 64, 1, dtype=u8), "must be 2-D")
    bad(0, torch.zeros(32, 128, dtype=u8).view(loadgen.FP8), "positive multiples")
    bad(2, torch.zeros(96, 64, dtype=u8), "positive multiples")
    bad(2, torch.zeros(64, 32, dtype=u8), "positive multiples")             # K = 64
    bad(0, torch.zeros(64, 128, dtype=u8), "a_q must be torch.float8_e4m3fn")
    bad(0, torch.zeros(64, 64, dtype=u8).view(loadgen.FP8), "a_q must be torch.uint8", fmt="fp4")
    bad(0, torch.zeros(64, 64, dtype=u8).view(loadgen.FP8), r"a_q must be \[64, 128\]")     # fp4-sized rows for fp8
    bad(0, torch.zeros(64, 128, dtype=u8), r"a_q must be \[64, 64\]", fmt="fp4")
    bad(2, torch.zeros(64, 64, dtype=torch.int8), "w_q must be torch.uint8")
    bad(0, torch.zeros(128, 64, dtype=u8).view(loadgen.FP8).t(), "a_q must have contiguous rows")
    bad(0, torch.zeros(64, 136, dtype=u8).view(loadgen.FP8)[:, :128], "a_q row stride 136")
    bad(2, torch.zeros(64, 72, dtype=u8)[:, :64], "w_q row stride 72")
    bad(2, torch.zeros(64 * 64 + 16, dtype=u8)[8:8 + 4096].view(64, 64), "w_q must be 16-byte aligned")
    bad(1, torch.zeros(64, 4, dtype=torch.int8), "a_scales must be torch.uint8")
    bad(1, torch.zeros(64, 3, dtype=u8), r"a_scales must be \[64, 4\]")
    bad(3, torch.zeros(32, 4, dtype=u8), r"w_scales must be \[64, 4\]")
    bad(3, torch.zeros(4, 64, dtype=u8).t(), "w_scales must have contiguous rows")
    bad(1, torch.zeros(1, 4, dtype=u8).expand(64, 4), "a_scales row stride 0")
    for out, msg in ((torch.zeros(64, 64), "out must be bf16"), (torch.zeros(64, 128, dtype=BF), "out must be bf16"),
                     (torch.zeros(64, 64, dtype=BF).t(), "8-byte aligned rows"),
                     (torch.zeros(64, 66, dtype=BF)[:, :64], "8-byte aligned rows"),
                     (torch.zeros(64 * 64 + 4, dtype=BF)[1:1 + 4096].view(64, 64), "8-byte aligned rows")):
        with pytest.raises(ValueError, match=msg):
            G(*_mx_args(), out=out)
    for bias in (torch.zeros(64, dtype=torch.float64), torch.zeros(32), torch.zeros(128)[::2], torch.zeros(1, 64),
                 torch.zeros(68)[1:65]):
        with pytest.raises(ValueError, match="bias must be a contiguous, 16-byte aligned fp32 vector"):
            G(*_mx_args(), bias=bias)
    raw = torch.zeros(64 * 128, dtype=u8)
    args = _mx_args()
    args[0] = raw.view(loadgen.FP8).view(64, 128)
    with pytest.raises(ValueError, match="out overlaps a_q"):
        G(*args, out=raw.view(BF).view(64, 64))
    args = _mx_args()
    args[3] = raw[:256].view(64, 4)
    with pytest.raises(ValueError, match="out overlaps w_scales"):
        G(*args, out=raw.view(BF).view(64, 64))
    with pytest.raises(AssertionError, match="native module was touched"):
        G(*_mx_args(), bias=torch.zeros(64), relu=True, cu_budget=4)
    args = _mx_args(128, 192, 384, "fp4")                               # padded rows and odd scale strides are legal
    args[0] = torch.zeros(128, 208, dtype=u8)[:, :192]
    args[1] = torch.zeros(128, 13, dtype=u8)[:, :12]
    args[3] = torch.zeros(192, 17, dtype=u8)[:, :12]
    with pytest.raises(AssertionError, match="native module was touched"):
        G(*args, out=torch.zeros(128, 196, dtype=BF)[:, :192])


def test_format_helpers():
    assert loadgen.MX_BLOCK == 32 == W.MX_BLOCK and loadgen.MX_FORMATS == ("fp8", "fp4")
    assert loadgen.mx_element_dtype("fp8") == loadgen.FP8 and loadgen.mx_element_dtype("fp4") == torch.uint8
    assert loadgen.mx_row_bytes("fp8", 256) == 256 and loadgen.mx_row_bytes("fp4", 256) == 128
    with pytest.raises(ValueError):
        loadgen.mx_row_bytes("fp6", 32)
    assert math.isclose(2.0 ** (0 - 127), float(loadgen.dequantize_mx_reference(
        torch.tensor([[0x38] * 32], dtype=torch.uint8), torch.tensor([[0]], dtype=torch.uint8), "fp8")[0, 0]))
