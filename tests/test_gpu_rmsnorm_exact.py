"""Exact-arithmetic, guarded-buffer tests of the residual add + RMSNorm (run with `-m gpu` on an MI355X), in
the style of test_gpu_rope_append_exact.py and of test_gpu_kernels_exact.py, whose guard helpers and
sentinels are used.

Every launch runs guarded: x and residual are windows (column offset 8, row stride D + 8) of NaN-filled
allocations, the weight is a window (offset 8) of a NaN-filled vector, y and residual_out are windows of the
same geometry of SENT16-filled allocations that are compared bitwise afterwards, guards included.

Shapes: D in DS x T in TS, with and without a residual.  D / 8 chunks of 16 bytes over 256 threads that own
the chunks t, t + 256, t + 512, t + 768: one chunk in one thread (8), two (16), one thread short of a chunk
each (2040), exactly one chunk per thread (2048), one thread with two chunks (2056), two chunks per thread
(4096), the ragged last chunk (8184: thread 255 has three) and the full four (8192).
test_the_shapes_cover_the_chunk_layouts asserts this.

Value regimes:

  integer  x and residual integers in [-8, 8], weight randn in bf16, eps in (1e-5, 1e-6, 0.0) (with eps == 0.0
           element 0 of every row is 1 + 1: no row is all zero).  hb is an integer of magnitude <= 16 and
           ss = sum hb^2 <= 2^21 an integer: exact in fp32 whatever the order.  residual_out and y are compared
           bitwise with an fp32 CPU emulation of the contract (emulate: float32 divide, add, sqrt, divide, two
           multiplies, one bf16 cast).
  true     x and residual randn, weight = 1 + 0.1 * randn.  residual_out is bit-equal to
           (x.float() + r.float()).bfloat16(); |y - ref| <= (2^-8 + 2^-11) * |ref| against float64 computed from
           residual_out's values: 2^-8 is the one bf16 rounding; a sum of at most 8192 non-negative fp32 terms is
           off by at most 2^-11 relative in any order, so r by at most 2^-12; the remaining fp32 roundings are
           below 2^-22 together.  The measured maximum of error / bound is printed (MEASURED below).
"""
import functools

import pytest
import torch

import test_gpu_corun_exact as CO
from test_gpu_kernels_exact import NAN, SENT16, guarded_input, guarded_output, guards_intact

pytestmark = pytest.mark.gpu

# MEASURED on an MI355X (printed by the tests):
MEASURED = """
  true regime, max |y - ref| / bound per (T, D, residual): 0.4933 (D = 8) .. 0.8851, 0.868 .. 0.885 from D = 2040 on;
  llm_block_decode_256, 8 picked rows of its two norms: 0.8773 and 0.8814; llm_block_prefill_2048: 0.8832 and 0.8842.
  Every integer-regime, NaN-rule, zero-row, in-place, large-address and co-run output bit-exact.
  The module: 59 tests in 7 s.
"""

C0 = 8                      # column offset of every window, and the padding of its rows
R0 = 2                      # guard rows in front of the windows (guarded_input / guarded_output)
DS = (8, 16, 2040, 2048, 2056, 4096, 8184, 8192)
TS = (1, 3, 5)
EPS = (1e-5, 1e-6, 0.0)
REGIMES = ("integer", "true")
TRUE_BOUND = 2.0 ** -8 + 2.0 ** -11
INF = float("inf")


@pytest.fixture(scope="module")
def hip():
    from k8s_gpu_scheduler_amd import _native
    return _native.hip(required=True)


def bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------
# the references (also imported by test_norm_act_cpu.py)
# ------------------------------------------------------------------------------------------------
def eps32(eps):
    return torch.tensor(float(eps), dtype=torch.float32)


def f32(op, a, b=None):
    """One IEEE fp32 operation on fp32 tensors, computed in float64 and rounded once to fp32.  For +, *, / and
    sqrt of fp32 operands that IS the fp32 operation (53 >= 2 * 24 + 2 bits: the second rounding is innocuous),
    and it does not depend on how the host's vector units evaluate an fp32 division or square root."""
    assert a.dtype == torch.float32 and (b is None or b.dtype == torch.float32)
    return (op(a.double()) if b is None else op(a.double(), b.double())).float()


def emulate(x, w, residual, eps, sequential=False):
    """The contract in fp32 on the CPU: (residual_out bf16 or None, y bf16, ss fp32) of bf16 x [T, D], w [D] and
    residual -- an fp32 add, the sum, an fp32 divide, add, square root and divide, two fp32 multiplies, one bf16
    cast.  The order of the sum is torch's, or with sequential=True left to right; in the integer regime every
    order gives the same bits."""
    ro = None if residual is None else f32(torch.add, x.float(), residual.float()).to(torch.bfloat16)
    hb = x.float() if residual is None else ro.float()
    sq = f32(torch.mul, hb, hb)
    ss = sq.cumsum(-1, dtype=torch.float32)[:, -1] if sequential else sq.sum(-1, dtype=torch.float32)
    mean = f32(torch.div, ss, torch.tensor(float(hb.shape[1])))
    r = f32(torch.div, torch.tensor(1.0), f32(torch.sqrt, f32(torch.add, mean, eps32(eps))))
    assert r.dtype == torch.float32 and r.shape == ss.shape
    return ro, f32(torch.mul, f32(torch.mul, hb, r[:, None]), w.float()[None, :]).to(torch.bfloat16), ss


def reference(hb, w, eps):
    """float64 y of the bf16 stream hb [T, D] (residual_out, or x without a residual), with the fp32 eps."""
    h = hb.double()
    r = 1.0 / torch.sqrt((h * h).mean(-1) + eps32(eps).double())
    return h * r[:, None] * w.double()[None, :]


def operands(regime, T, D, residual, eps, seed):
    """(x, residual or None, weight) as bf16 CPU tensors."""
    g = torch.Generator().manual_seed(seed)
    if regime == "integer":
        x = torch.randint(-8, 9, (T, D), generator=g).float()
        r = torch.randint(-8, 9, (T, D), generator=g).float()
        w = torch.randn(D, generator=g)
        if eps == 0.0:
            x[:, 0] = r[:, 0] = 1.0
    else:
        x = torch.randn(T, D, generator=g).to(torch.bfloat16).float()
        r = torch.randn(T, D, generator=g).to(torch.bfloat16).float()
        w = 1 + 0.1 * torch.randn(D, generator=g)
        x[x == 0] = 1.0                                              # no zero in either stream: no zero output
        r = torch.where((x + r).to(torch.bfloat16).float() == 0, x, r)
    return x.to(torch.bfloat16), (r.to(torch.bfloat16) if residual else None), w.to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------
# guarded operands
# ------------------------------------------------------------------------------------------------
def guarded_weight(w):
    big = torch.full((w.numel() + 2 * C0,), NAN, dtype=torch.bfloat16, device="cuda")
    big[C0:C0 + w.numel()] = w.cuda()
    return big[C0:C0 + w.numel()]


class Case:
    def __init__(self, regime, T, D, residual, eps, seed, plant=None):
        """plant(x, r, w) may change the bf16 CPU operands in place."""
        self.regime, self.T, self.D, self.eps, self.has_res = regime, T, D, eps, residual
        x, r, w = operands(regime, T, D, residual, eps, seed)
        if plant:
            plant(x, r, w)
        self.x_host, self.r_host, self.w_host = x, r, w
        self.exp_ro, self.exp_y, ss = emulate(x, w, r, eps)
        if regime == "integer" and not plant:
            assert bool((ss < 2 ** 24).all()) and torch.equal(ss, ss.round()) and bool(self.exp_y.float().isfinite().all())
            assert eps != 0.0 or bool((ss > 0).all())
        if regime == "true":
            self.ref = reference(x if r is None else self.exp_ro, w, eps)
            self.bound = TRUE_BOUND * self.ref.abs()
        self.x = guarded_input(x.cuda(), D + C0, c0=C0)
        self.res = guarded_input(r.cuda(), D + C0, c0=C0) if residual else None
        self.w = guarded_weight(w)
        self.outs = self.new_outputs()
        assert self.x.data_ptr() % 16 == 0 and self.w.data_ptr() % 16 == 0 and self.w.is_contiguous()
        assert T == 1 or self.x.stride(0) == D + C0

    def new_outputs(self):
        """(raw_y, y, raw_ro, ro): [T, D] windows in SENT16-filled allocations of their own (ro only with a residual)."""
        raw_y, y = guarded_output(self.T, self.D, self.D + C0, C0, "cuda")
        raw_ro, ro = guarded_output(self.T, self.D, self.D + C0, C0, "cuda") if self.has_res else (None, None)
        return raw_y, y, raw_ro, ro

    @staticmethod
    def resentinel(outs):
        for raw in (outs[0], outs[2]):
            if raw is not None:
                raw.fill_(SENT16)

    def launch(self, outs, **kw):
        from k8s_gpu_scheduler_amd.ops import loadgen
        _, y, _, ro = outs
        kw.setdefault("eps", self.eps)
        return loadgen.add_rmsnorm(self.x, self.w, self.res, out=y, residual_out=ro, **kw)

    def run(self, **kw):
        self.resentinel(self.outs)
        return self.launch(self.outs, **kw)

    def results(self, outs=None):
        """(y, residual_out or None) on the CPU, the guards of both checked."""
        raw_y, y, raw_ro, ro = self.outs if outs is None else outs
        torch.cuda.synchronize()
        win = (slice(R0, R0 + self.T), slice(C0, C0 + self.D))
        assert guards_intact(raw_y, win, SENT16), "write outside y's window"
        assert raw_ro is None or guards_intact(raw_ro, win, SENT16), "write outside residual_out's window"
        return y.cpu(), (None if ro is None else ro.cpu())

    def check(self, what, outs=None):
        y, ro = self.results(outs)
        if self.has_res:
            same = bits(ro) == bits(self.exp_ro)
            assert bool(same.all()), (what, "residual_out", int((~same).sum()), (~same).nonzero()[0].tolist())
        if self.regime == "integer":
            same = bits(y) == bits(self.exp_y)
            if not bool(same.all()):
                r, c = (~same).nonzero()[0].tolist()
                raise AssertionError((what, f"y: {int((~same).sum())} elements differ, first at [{r}, {c}]: got "
                                            f"{y[r, c].item()}, expected {self.exp_y[r, c].item()}"))
            return
        err = (y.double() - self.ref).abs()
        ratio = (err / self.bound.clamp_min(1e-300)).max().item()
        print(f"add_rmsnorm, true regime {what}: max |y - ref| / bound = {ratio:.4f}")
        assert bool((err <= self.bound).all()), (what, ratio)

    def untouched(self, outs=None):
        raw_y, _, raw_ro, _ = self.outs if outs is None else outs
        torch.cuda.synchronize()
        none = (slice(0, 0), slice(0, 0))
        return guards_intact(raw_y, none, SENT16) and (raw_ro is None or guards_intact(raw_ro, none, SENT16))


@functools.lru_cache(maxsize=None)
def case(regime, T, D, residual, eps=1e-5):
    return Case(regime, T, D, residual, eps, seed=9000 + 1000 * REGIMES.index(regime) + 10 * DS.index(D) + T + 5 * residual
                + EPS.index(eps) * 100)


# ------------------------------------------------------------------------------------------------
# 1. the regimes over every shape
# ------------------------------------------------------------------------------------------------
def test_the_shapes_cover_the_chunk_layouts():
    chunks = [d // 8 for d in DS]
    assert all(d % 8 == 0 and 8 <= d <= 8192 for d in DS)
    assert 1 in chunks                                               # one chunk in one thread
    assert 256 in chunks                                             # exactly one chunk per thread
    assert 257 in chunks                                             # one thread with two chunks
    assert 1024 in chunks                                            # the full four chunks
    assert any(c > 768 and c % 256 for c in chunks)                  # the ragged last chunk
    assert any(c < 256 and c > 64 and c % 64 for c in chunks)        # a wave partly without a chunk
    assert 1 in TS and any(t > 1 and t % 2 for t in TS) and len(set(EPS)) == 3 and 0.0 in EPS


@pytest.mark.parametrize("residual", [True, False], ids=["residual", "plain"])
@pytest.mark.parametrize("D", DS)
def test_integer_regime(hip, D, residual):
    for T in TS:
        for eps in EPS:
            c = case("integer", T, D, residual, eps)
            c.run()
            c.check(("integer", T, D, residual, eps))


@pytest.mark.parametrize("residual", [True, False], ids=["residual", "plain"])
@pytest.mark.parametrize("D", DS)
def test_true_regime(hip, D, residual):
    for T in TS:
        c = case("true", T, D, residual)
        c.run()
        c.check(("true", T, D, residual))


# ------------------------------------------------------------------------------------------------
# 2. fused == unfused, in place == out of place, determinism
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2056, 8192])
def test_fused_equals_unfused(hip, D):
    from k8s_gpu_scheduler_amd.ops import loadgen
    c = case("true", 5, D, True)
    c.run()
    y, ro = c.results()
    y2 = loadgen.add_rmsnorm(c.outs[3], c.w, eps=c.eps)              # from the rounded stream, no residual
    torch.cuda.synchronize()
    assert torch.equal(bits(y2.cpu()), bits(y)) and bool(y.float().isfinite().all())


@pytest.mark.parametrize("D", [2056, 8192])
def test_in_place_residual_equals_out_of_place(hip, D):
    from k8s_gpu_scheduler_amd.ops import loadgen
    c = case("true", 5, D, True)
    c.run()
    y, ro = c.results()
    res = guarded_input(c.r_host.cuda(), D + C0, c0=C0)
    raw_y, y2 = guarded_output(5, D, D + C0, C0, "cuda")
    got = loadgen.add_rmsnorm(c.x, c.w, res, eps=c.eps, out=y2, residual_out=res)
    torch.cuda.synchronize()
    assert got[0] is y2 and got[1] is res
    assert torch.equal(bits(y2.cpu()), bits(y)) and torch.equal(bits(res.cpu()), bits(ro))
    assert guards_intact(raw_y, (slice(R0, R0 + 5), slice(C0, C0 + D)), SENT16)
    whole = torch.empty(0, dtype=torch.bfloat16, device="cuda").set_(res.untyped_storage()).float()
    assert int(whole.isnan().sum()) == whole.numel() - 5 * D          # the NaN fence around residual is intact


def test_two_launches_are_bit_identical(hip):
    for D in (2056, 8192):
        c = case("true", 5, D, True)
        a, b = c.new_outputs(), c.new_outputs()
        c.launch(a)
        c.launch(b)
        (ya, ra), (yb, rb) = c.results(a), c.results(b)
        assert torch.equal(bits(ya), bits(yb)) and torch.equal(bits(ra), bits(rb))


# ------------------------------------------------------------------------------------------------
# 3. the NaN rule, zero rows
# ------------------------------------------------------------------------------------------------
def assert_same_where_finite(got, exp, what):
    """NaN where the emulation has NaN (sign and payload unspecified), the same bits everywhere else."""
    nan = exp.float().isnan()
    assert torch.equal(got.float().isnan(), nan), (what, "NaN cells differ")
    assert torch.equal(bits(got)[~nan], bits(exp)[~nan]), (what, "finite cells differ")


def plant_rows(x, r, w):
    x[0, 5] = NAN                       # a NaN in x
    r[1, 2055] = NAN                    # ... and in the residual, in the last chunk
    x[2, 7] = INF                       # ss = Inf, r = 0: zeros, and NaN (Inf * 0) in its own element
    r[2, 300] = -INF
    x[3, 9], r[3, 9] = INF, -INF        # Inf - Inf: a NaN that the add makes


def plant_weight(x, r, w):
    w[3], w[9], w[2050] = NAN, INF, -INF


def test_nan_rule(hip):
    T, D, seed = 6, 2056, 9901
    clean = Case("integer", T, D, True, 1e-5, seed)
    rows = Case("integer", T, D, True, 1e-5, seed, plant=plant_rows)
    wts = Case("integer", T, D, True, 1e-5, seed, plant=plant_weight)
    for c in (clean, rows, wts):
        c.run()
    cy, cro = clean.results()
    clean.check("clean")
    # planted rows: the emulation says what IEEE gives; the contract's own statements on top
    y, ro = rows.results()
    assert_same_where_finite(y, rows.exp_y, "rows y")
    assert_same_where_finite(ro, rows.exp_ro, "rows residual_out")
    for row in (0, 1, 3):
        assert bool(y[row].float().isnan().all()), f"row {row} of y is not all NaN"
    assert bool(y[2, 7].isnan()) and bool(y[2, 300].isnan()) and int(y[2].float().isnan().sum()) == 2
    assert bool((y[2].float().nan_to_num(0.0) == 0).all())          # r = 1 / sqrt(Inf) = 0
    nan_ro = ro.float().isnan()
    assert nan_ro.nonzero().tolist() == [[0, 5], [1, 2055], [3, 9]]   # only its own element
    assert ro[2, 7].item() == INF and ro[2, 300].item() == -INF
    assert torch.equal(bits(y[4:]), bits(cy[4:])) and torch.equal(bits(ro[4:]), bits(cro[4:]))    # no other row
    keep = torch.ones(T, D, dtype=torch.bool)
    keep[0, 5] = keep[1, 2055] = keep[2, 7] = keep[2, 300] = keep[3, 9] = False
    assert torch.equal(bits(ro)[keep], bits(cro)[keep])
    # planted weights: their own column of every row of y, nothing of residual_out
    y, ro = wts.results()
    assert_same_where_finite(y, wts.exp_y, "weight y")
    assert torch.equal(bits(ro), bits(cro))
    cols = torch.ones(D, dtype=torch.bool)
    cols[[3, 9, 2050]] = False
    assert torch.equal(bits(y[:, cols]), bits(cy[:, cols])) and bool(y[:, 3].float().isnan().all())
    assert not bool(y[:, [9, 2050]].float().isfinite().any())


def test_all_zero_row(hip):
    """Row 1 is all zero, with both signs of zero in the rounded sum: zeros with the sign of hb * w for eps > 0,
    NaN (0 * Inf) for eps == 0; the other rows as ever."""
    def zero_row(x, r, w):
        x[1] = r[1] = 0.0
        bits(x)[1, ::2] = bits(r)[1, ::2] = -32768                    # -0.0 + -0.0 = -0.0, +0.0 + +0.0 = +0.0
    T, D, seed = 3, 2056, 9902
    for eps in (1e-5, 0.0):
        c = Case("integer", T, D, True, eps, seed, plant=zero_row)
        c.run()
        y, ro = c.results()
        assert torch.equal(bits(ro), bits(c.exp_ro)) and bits(ro)[1, ::2].eq(-32768).all() and bits(ro)[1, 1::2].eq(0).all()
        assert_same_where_finite(y, c.exp_y, ("zero row", eps))
        if eps:
            want = torch.where((c.w_host.float() < 0) ^ (torch.arange(D) % 2 == 0), -32768, 0).to(torch.int16)
            assert torch.equal(bits(y)[1], want) and bool((want == 0).any()) and bool((want != 0).any())
        else:
            assert bool(y[1].float().isnan().all())
        assert bool(y[[0, 2]].float().isfinite().all())


# ------------------------------------------------------------------------------------------------
# 4. other launch paths
# ------------------------------------------------------------------------------------------------
def test_side_stream_and_graph_replay(hip):
    c = case("integer", 5, 2056, True)
    s = torch.cuda.Stream()
    c.resentinel(c.outs)
    torch.cuda.synchronize()
    c.launch(c.outs, stream=s)
    s.synchronize()
    c.check("side stream")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        c.launch(c.outs, stream=s)
    for k in range(2):
        if k == 0:                       # separate outputs: the second replay writes over the first, idempotent
            c.resentinel(c.outs)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        s.synchronize()
        c.check(("replay", k))


@pytest.mark.parametrize("breakage", ["eps-negative", "eps-nan", "y-is-x", "y-is-residual_out", "residual_out-is-x",
                                      "weight-short", "weight-fp32", "odd-stride", "misaligned"])
def test_a_bad_call_raises_and_launches_nothing(hip, breakage):
    from k8s_gpu_scheduler_amd.ops import loadgen
    c = case("integer", 5, 2056, True)
    _, y, _, ro = c.outs
    x, w, res, kw = c.x, c.w, c.res, {"eps": 1e-5}
    if breakage == "eps-negative":
        kw["eps"] = -1e-5
    elif breakage == "eps-nan":
        kw["eps"] = NAN
    elif breakage == "y-is-x":
        x = y
    elif breakage == "y-is-residual_out":
        ro = y
    elif breakage == "residual_out-is-x":
        x = ro
    elif breakage == "weight-short":
        w = w[:-8]
    elif breakage == "weight-fp32":
        w = w.float()
    elif breakage == "odd-stride":
        x = torch.zeros(5, 2056 + 4, dtype=torch.bfloat16, device="cuda")[:, :2056]
    else:
        x = torch.zeros(5 * 2056 + 8, dtype=torch.bfloat16, device="cuda")[4:4 + 5 * 2056].view(5, 2056)
    c.resentinel(c.outs)
    with pytest.raises((ValueError, TypeError)):
        loadgen.add_rmsnorm(x, w, res, out=y, residual_out=ro, **kw)
    assert c.untouched()


def test_residual_out_without_residual_raises(hip):
    from k8s_gpu_scheduler_amd.ops import loadgen
    c = case("integer", 5, 2056, True)
    c.resentinel(c.outs)
    with pytest.raises(ValueError, match="without a residual"):
        loadgen.add_rmsnorm(c.x, c.w, out=c.outs[1], residual_out=c.outs[3])
    assert c.untouched()


def test_workgroups_match_the_python_rule(hip):
    from k8s_gpu_scheduler_amd.models import workloads as W
    for T in (0, 1, 3, 256, 2048, 2 ** 31 - 1):
        assert hip.add_rmsnorm_workgroups(T) == W.default_add_rmsnorm_workgroups(T) == T


# ------------------------------------------------------------------------------------------------
# 5. row offsets beyond 4 GiB
# ------------------------------------------------------------------------------------------------
BIG_LD = 2 ** 30 + 8


def big_window(T, D):
    """(raw, view): a [T, D] bf16 window, row stride 2^30 + 8, column offset 8, of one UNINITIALISED int16
    allocation -- row 2 starts past 4 GiB."""
    raw = torch.empty(((T - 1) * BIG_LD + D + 2 * C0,), dtype=torch.int16, device="cuda")
    return raw, raw.view(torch.bfloat16).as_strided((T, D), (BIG_LD, 1), C0)


def test_row_offsets_beyond_4_gib(hip):
    """x and y get the big stride (an input and an output), the residual streams keep D + 8.  Only the windows
    and the 8 cells on either side of each row of y are initialised."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    T, D = 3, 4096
    c = Case("integer", T, D, True, 1e-5, 9903)
    raw_x, x = big_window(T, D)
    raw_y, y = big_window(T, D)
    assert 2 * BIG_LD * 2 > 2 ** 32 and x.data_ptr() % 16 == 0
    x.copy_(c.x_host.cuda())
    fence = raw_y.as_strided((T, D + 2 * C0), (BIG_LD, 1), 0)
    fence.fill_(SENT16)
    _, _, raw_ro, ro = c.outs
    raw_ro.fill_(SENT16)
    loadgen.add_rmsnorm(x, c.w, c.res, eps=c.eps, out=y, residual_out=ro)
    torch.cuda.synchronize()
    f = fence.cpu()
    assert bool((f[:, :C0] == SENT16).all()) and bool((f[:, C0 + D:] == SENT16).all()), "write outside y's rows"
    assert torch.equal(f[:, C0:C0 + D], bits(c.exp_y)) and torch.equal(bits(ro.cpu()), bits(c.exp_ro))
    assert guards_intact(raw_ro, (slice(R0, R0 + T), slice(C0, C0 + D)), SENT16)
    del raw_x, raw_y, x, y, fence
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------
# 6. beside a co-running load
# ------------------------------------------------------------------------------------------------
class NormLaunch:
    """One launch on a Case's inputs into outputs of its own (reset / enqueue / check, as the co-run module's
    CaseLaunch has)."""

    def __init__(self, c, what):
        self.case, self.what = c, what
        self.outs = c.new_outputs()

    def reset(self):
        self.case.resentinel(self.outs)

    def enqueue(self, st):
        self.case.launch(self.outs, stream=st)

    def check(self, tag):
        self.case.check((tag, self.what), self.outs)


@pytest.mark.parametrize("aggressor,mode", [pytest.param(a, m, id=f"{a}-{m}") for a, m in CO.BASE_PAIRS])
def test_add_rmsnorm_corun(hip, aggressor, mode):
    c = Case("integer", 256, 4096, True, 1e-5, 9904)
    victim = CO.Load("add-rmsnorm-integer", {}, [NormLaunch(c, ("integer", 256, 4096, r)) for r in range(CO.R)])
    try:
        CO.corun(hip, victim, CO.aggressor_for(aggressor, mode), mode)
    finally:
        CO.restore_knobs(hip)


# ------------------------------------------------------------------------------------------------
# 7. pod path
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("workload", ["llm_block_decode_256", "llm_block_prefill_2048"])
def test_executor_llm_block_norm_output(hip, workload):
    """The executor's operands of both add_rmsnorm ops and, after one iteration, 8 picked rows of y (op_output)
    and residual_out against the reference."""
    from k8s_gpu_scheduler_amd.models import workloads as W
    from k8s_gpu_scheduler_amd.parallel.executor import _Buffers, enqueue_ops, op_output
    dev = torch.device("cuda", 0)
    w = W.get(workload)
    a = _Buffers(w, dev)
    norms = [(o, t) for o, t in a.ops if o.kind == "add_rmsnorm"]
    assert len(norms) == 2 and [i for i, (o, _) in enumerate(a.ops) if o.kind == "add_rmsnorm"] == [0, 5]
    for o, t in norms:
        y, ro, x, res, wt = t
        assert op_output(o, t) is y and x.shape == res.shape == y.shape == ro.shape == (o.M, o.N) and wt.shape == (o.N,)
        y.view(torch.int16).fill_(SENT16)
        ro.view(torch.int16).fill_(SENT16)
    enqueue_ops(a, 1, torch.cuda.current_stream(), 0)
    torch.cuda.synchronize()
    for k, (o, t) in enumerate(norms):
        y, ro, x, res, wt = (v.cpu() for v in t)
        rows = torch.tensor([0, 1, o.M // 3, o.M // 2, o.M // 2 + 1, o.M - 3, o.M - 2, o.M - 1])
        exp_ro = (x[rows].float() + res[rows].float()).to(torch.bfloat16)
        assert torch.equal(bits(ro[rows]), bits(exp_ro))
        ref = reference(exp_ro, wt, 1e-5)
        err = (y[rows].double() - ref).abs()
        ratio = (err / (TRUE_BOUND * ref.abs()).clamp_min(1e-300)).max().item()
        print(f"{workload} add_rmsnorm {k}, 8 rows: max |y - ref| / bound = {ratio:.4f}")
        assert bool((err <= TRUE_BOUND * ref.abs()).all()), ratio
        assert not bool((bits(y) == SENT16).all(-1).any()) and not bool((bits(ro) == SENT16).all(-1).any())   # every row written
    del a, norms, t, y, ro
    torch.cuda.empty_cache()
