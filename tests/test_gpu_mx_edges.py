"""The MX kernels -- loadgen.quantize_mx and gemm_mx -- where their exact modules do not reach (run with `-m gpu` on an
MI355X): operands placed past 4 GiB, gemm_mx on a side stream and replayed from a graph, and both beside a co-running
load.  The cases, references and comparisons are those of test_gpu_quantize_mx_exact.py (QM) and
test_gpu_gemm_mx_exact.py (MX: the integer regime, `padded`, `same`, `to_bf16_exact`); the launch-path and co-run
plumbing is that of test_gpu_moe_edges.py (ED) and the co-run harness (CO), unchanged.

  past 4 GiB   one operand per test in an UNINITIALISED allocation of which only the windows are filled.
               quantize_mx: x with a row stride of 2^30 + 8 elements (T = 3, D = 96: row 2 starts past 4 GiB), and q
               with a row stride of 2^31 + 8 bytes, which the wrapper admits (any stride >= the row).  gemm_mx takes
               `int` strides: a and w element rows 2^26 + 16 bytes apart and c rows 2^25 + 8 elements apart at
               M = N = 128, so rows 64 and later start past 4 GiB -- 128 x 128 runs as four 64 x 64 tiles on the whole
               chip and as one 128 x 128 tile at a 1-CU share --, integer regime, both activation formats; the scale
               arrays stay small.
  launch paths gemm_mx on a side stream, then one capture and two replays, both tiles and formats at K = 640.
  co-run       CO.R launches against CO.BASE_PAIRS, bit-exact: quantize_mx at 67 x 4096 in guarded windows, both
               formats; gemm_mx on both tiles x both formats at K = 640 with padded operands and a guarded C.
"""
import functools

import pytest
import torch

import test_gpu_corun_exact as CO
import test_gpu_gemm_mx_exact as MX
import test_gpu_moe_edges as ED
import test_gpu_quantize_mx_exact as QM
from k8s_gpu_scheduler_amd.ops import loadgen
from test_gpu_kernels_exact import NAN, SENT16, guards_intact
from test_gpu_paged_large_addresses import need_free

pytestmark = pytest.mark.gpu

# MEASURED on an MI355X (printed by CO.corun; victim slowdown = co-run event time / alone host time):
MEASURED = """
  The module: 44 tests in 3.3 s, none skipped (a test with an operand past 4 GiB takes 0.02 .. 0.1 s here and up to
  1.4 s in the whole suite, its allocation most of it).
  Every comparison bit-exact; no kernel needed a change.  The six co-run victims (quantize_mx in both formats, gemm_mx
  on both tiles x both formats):
  aggressor | mode        victim slowdown  aggressor slowdown  passes
  stream    | same-slice   0.32 .. 0.42     0.89 .. 0.96        5 .. 6
  stream    | unmasked     0.63 .. 0.79     0.70 .. 0.89        9 .. 12
  mfma      | same-slice   0.23 .. 0.38     0.38 .. 0.59       27 .. 34
  mfma      | unmasked     0.20 .. 0.31     0.42 .. 0.45       33 .. 43
  (a victim slowdown below 1: the lone time is the host's, enqueueing included, as in the co-run module.)
"""

BF, U8 = torch.bfloat16, torch.uint8
FORMATS = MX.FORMATS
GIB = 1 << 30
X_LD = 2 ** 30 + 8                                                      # elements: row 2 starts past 4 GiB
Q_LD = 2 ** 31 + 8                                                      # bytes
EL_LD = 2 ** 26 + 16                                                    # bytes, < 2^31: rows 64 and later start past 4 GiB
C_LD = 2 ** 25 + 8                                                      # elements: the same
SMALL = [pytest.param(0, 4, id="64x64"), pytest.param(1, 1, id="128x128")]    # (cu_budget, workgroups) of 128 x 128


@pytest.fixture(scope="module")
def hip():
    from k8s_gpu_scheduler_amd import _native
    return _native.hip(required=True)


# ------------------------------------------------------------------------------------------------
# launch objects
# ------------------------------------------------------------------------------------------------
class QuantCase:
    """67 x 4096 of QM.case in a NaN-guarded window; q and the scales are windows of SENT8-filled allocations (8-byte
    aligned q rows: one store per lane)."""

    def __init__(self, fmt):
        self.fmt = fmt
        x, self.qr, self.sr = QM.case("67x4096", fmt)
        self.T, D = x.shape
        big = torch.full((self.T + 5, D + 24), NAN, dtype=BF, device="cuda")
        big[2:2 + self.T, 8:8 + D] = x
        self.x = big[2:2 + self.T, 8:8 + D]

    def launch(self, tag=None):
        return QuantLaunch(self, tag)


class QuantLaunch:
    def __init__(self, case, tag):
        self.case, self.tag = case, tag
        T, qc, sc = case.T, case.qr.shape[1], case.sr.shape[1]
        self.qraw = torch.empty((T + 4, qc + 24), dtype=U8, device="cuda")
        self.sraw = torch.empty((T + 4, sc + 3), dtype=U8, device="cuda")
        self.q = self.qraw[1:1 + T, 8:8 + qc].view(loadgen.mx_element_dtype(case.fmt))
        self.s = self.sraw[1:1 + T, 1:1 + sc]
        self.want_q = torch.full(tuple(self.qraw.shape), QM.SENT8, dtype=U8)
        self.want_q[1:1 + T, 8:8 + qc] = case.qr
        self.want_s = torch.full(tuple(self.sraw.shape), QM.SENT8, dtype=U8)
        self.want_s[1:1 + T, 1:1 + sc] = case.sr

    def reset(self):
        self.qraw.fill_(QM.SENT8)
        self.sraw.fill_(QM.SENT8)

    def enqueue(self, st):
        loadgen.quantize_mx(self.case.x, self.case.fmt, out=self.q, scales=self.s, stream=st)

    def check(self, tag):
        assert torch.equal(self.qraw.cpu(), self.want_q), (tag, self.case.fmt, self.tag, "q window or its guard cells differ")
        assert torch.equal(self.sraw.cpu(), self.want_s), (tag, self.case.fmt, self.tag, "scale window or its guard cells differ")


@functools.lru_cache(maxsize=None)
def quant_case(fmt):
    return QuantCase(fmt)


class GemmMxCase:
    """MX.integer_case with the padded operands of MX.test_padded_operands_and_guarded_output."""

    def __init__(self, M, N, K, cu_budget, fmt):
        self.M, self.N, self.K, self.cu_budget, self.fmt = M, N, K, cu_budget, fmt
        (a_q, a_s, w_q, w_s), self.bias, self.ref = MX.integer_case(M, N, K, fmt)
        self.ops = (MX.padded(a_q, 48, 16, 0x7F if fmt == "fp8" else 0xFF), MX.padded(a_s, 5, 3, 255),
                    MX.padded(w_q, 32, 16, 0xFF), MX.padded(w_s, 7, 2, 255))

    def expected(self, act):
        exp = MX.to_bf16_exact(self.ref + self.bias.cpu().double() if act else self.ref)
        return torch.where(exp > 0, exp, torch.zeros_like(exp)) if act else exp

    def launch(self, tag=0):
        return GemmMxLaunch(self, tag)


class GemmMxLaunch:
    """Launch `tag`: odd ones with bias and relu, even ones without."""

    def __init__(self, case, tag):
        self.case, self.tag, self.act = case, tag, bool(tag % 2)
        M, N = case.M, case.N
        self.raw = torch.empty((2 + M + 3, N + 12), dtype=torch.int16, device="cuda")
        self.out = self.raw.view(BF)[2:2 + M, 4:4 + N]
        self.exp = case.expected(self.act)

    def reset(self):
        self.raw.fill_(SENT16)

    def enqueue(self, st):
        c = self.case
        loadgen.gemm_mx(*c.ops, c.fmt, out=self.out, bias=c.bias if self.act else None, relu=self.act, stream=st,
                        cu_budget=c.cu_budget)

    def check(self, tag):
        c = self.case
        torch.cuda.synchronize()
        MX.same(self.out, self.exp, f"{tag} {self.tag}: {c.fmt} {c.M}x{c.N}x{c.K}")
        assert guards_intact(self.raw, (slice(2, 2 + c.M), slice(4, 4 + c.N)), SENT16), (tag, self.tag, "write outside C")


@functools.lru_cache(maxsize=None)
def gemm_mx_case(M, N, K, cu_budget, fmt):
    return GemmMxCase(M, N, K, cu_budget, fmt)


# ------------------------------------------------------------------------------------------------
# offsets past 4 GiB
# ------------------------------------------------------------------------------------------------
def byte_rows(rows, cols, ld, c0=16, tail=0):
    """(raw, view): an UNINITIALISED uint8 allocation and its window [rows, cols] at byte c0, row stride ld."""
    raw = torch.empty(((rows - 1) * ld + c0 + cols + tail,), dtype=U8, device="cuda")
    view = raw.as_strided((rows, cols), (ld, 1), c0)
    assert view.data_ptr() % 16 == 0
    return raw, view


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("big", ("x", "q"))
def test_quantize_mx_rows_past_4_gib(big, fmt):
    need_free(5 * GIB, f"quantize_mx with {big} rows past 4 GiB")
    x, qr, sr = QM.case("3x96", fmt)
    T, qc = 3, qr.shape[1]
    raw = None
    try:
        q = s = None
        if big == "x":
            raw = torch.empty(((T - 1) * X_LD + 8 + 96,), dtype=torch.int16, device="cuda")
            xv = raw.view(BF).as_strided((T, 96), (X_LD, 1), 8)
            xv.copy_(x)
            assert 2 * X_LD * 2 > 2 ** 32 and xv.data_ptr() % 16 == 0
            q, s = loadgen.quantize_mx(xv, fmt)
            torch.cuda.synchronize()
            QM.check(q, s, qr, sr, f"x row stride 2^30 + 8, {fmt}")
        else:
            raw, win = byte_rows(T, 8 + qc + 8, Q_LD)                   # 8 guard bytes on each side of every row
            win.fill_(QM.SENT8)
            q = win[:, 8:8 + qc].view(loadgen.mx_element_dtype(fmt))
            assert q.stride(0) == Q_LD > 2 ** 31 and 2 * Q_LD > 2 ** 32
            _, s = loadgen.quantize_mx(x, fmt, out=q)
            torch.cuda.synchronize()
            want = torch.full((T, 8 + qc + 8), QM.SENT8, dtype=U8)
            want[:, 8:8 + qc] = qr
            assert torch.equal(win.cpu(), want), f"q row stride 2^31 + 8, {fmt}: q window or its guard bytes differ"
            assert torch.equal(s.cpu(), sr)
    finally:
        del raw
        xv = q = win = None
        torch.cuda.empty_cache()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("cu_budget,blocks", SMALL)
@pytest.mark.parametrize("big", ("a", "w", "c"))
def test_gemm_mx_rows_past_4_gib(hip, big, cu_budget, blocks, fmt):
    M = N = 128
    K = 256
    assert hip.gemm_mx_workgroups(M, N, K, cu_budget) == blocks
    need_free(9 * GIB, f"gemm_mx with {big} rows past 4 GiB")
    (a_q, a_s, w_q, w_s), bias, ref = MX.integer_case(M, N, K, fmt)
    exp = MX.to_bf16_exact(ref)
    raw = None
    try:
        out = None
        if big in ("a", "w"):
            src = a_q if big == "a" else w_q
            raw, view = byte_rows(src.shape[0], src.shape[1], EL_LD)
            view.copy_(src.view(U8))
            view = view.view(src.dtype)
            assert EL_LD < 2 ** 31 and EL_LD % 16 == 0 and 64 * EL_LD > 2 ** 32 and view.stride(0) == EL_LD
            a_q, w_q = (view, w_q) if big == "a" else (a_q, view)
            out = MX.run((a_q, a_s, w_q, w_s), fmt, cu_budget)
            MX.same(out, exp, f"{big} rows 2^26 + 16 bytes apart, {fmt}, {blocks} workgroups")
        else:
            raw16 = raw = torch.empty(((M - 1) * C_LD + 8 + N + 8,), dtype=torch.int16, device="cuda")
            graw = raw16.as_strided((M, 8 + N + 8), (C_LD, 1), 0)       # 8 guard cells on each side of every row window
            graw.fill_(SENT16)
            out = raw16.view(BF).as_strided((M, N), (C_LD, 1), 8)
            assert C_LD < 2 ** 31 and 64 * C_LD * 2 > 2 ** 32
            MX.run((a_q, a_s, w_q, w_s), fmt, cu_budget, out=out)
            MX.same(out, exp, f"c rows 2^25 + 8 elements apart, {fmt}, {blocks} workgroups")
            got = graw.cpu()
            assert bool((got[:, :8] == SENT16).all()) and bool((got[:, 8 + N:] == SENT16).all())
    finally:
        del raw
        view = out = graw = raw16 = a_q = w_q = None
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------
# other launch paths
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("M,N,cu_budget,blocks", MX.TILES)
def test_gemm_mx_side_stream_and_graph_replay(hip, M, N, cu_budget, blocks, fmt):
    assert hip.gemm_mx_workgroups(M, N, 640, cu_budget) == blocks
    ED.side_stream_and_graph_replay(gemm_mx_case(M, N, 640, cu_budget, fmt).launch(1))


# ------------------------------------------------------------------------------------------------
# beside a co-running load
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aggressor,mode", ED.PAIRS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_quantize_mx_corun(hip, fmt, aggressor, mode):
    c = quant_case(fmt)
    ED.corun(hip, f"quantize_mx-{fmt}-67x4096", [c.launch(r) for r in range(CO.R)], aggressor, mode)


@pytest.mark.parametrize("aggressor,mode", ED.PAIRS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("M,N,cu_budget,blocks", MX.TILES)
def test_gemm_mx_corun(hip, M, N, cu_budget, blocks, fmt, aggressor, mode):
    assert hip.gemm_mx_workgroups(M, N, 640, cu_budget) == blocks
    c = gemm_mx_case(M, N, 640, cu_budget, fmt)
    ED.corun(hip, f"gemm_mx-{fmt}-{M}x{N}x640", [c.launch(r) for r in range(CO.R)], aggressor, mode)
