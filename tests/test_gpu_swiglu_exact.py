"""Exact-arithmetic, guarded-buffer tests of SwiGLU (run with `-m gpu` on an MI355X), in the style of
test_gpu_rmsnorm_exact.py and of test_gpu_kernels_exact.py, whose guard helpers and sentinels are used.

Every launch runs guarded: gate_up is a window (column offset 8, row stride 2 F + 8) of a NaN-filled
allocation, out a window (column offset 8, row stride F + 8) of a SENT16-filled allocation that is compared
bitwise afterwards, guards included.

Shapes (T, F) of SHAPES.  The work is flattened over (row, 16-byte chunk of 8 outputs), a workgroup takes
1,024 consecutive chunks, thread t the chunks t, t + 256, t + 512, t + 768: a single chunk (1, 8); two
(1, 16); rows of 127 and 129 chunks that end inside a thread's second chunk and put row boundaries inside
one workgroup (3, 1016), (3, 1032), and rows of exactly half a wave's reach (3, 1024); exactly one workgroup
(1, 8192); one chunk into the second (1, 8200); a ragged ninth workgroup (5, 14336).
test_the_shapes_cover_the_grid_walk asserts this.

Value regimes:

  saturated  g is drawn from {+0, -0, +-128, +-129, +-256, +-512}, u holds the integers of [-127, 127] in a
             per-row random order (repeated along the row) times a per-row power of two.  The expectation is
             built from the contract's consequences, not from an exponential: g = +-0 gives s = +-0;
             g >= 128 gives e == 0, s == g and out = bf16(g * u), an exact fp32 product; g <= -128 gives
             e == +Inf and s = -0.0.  Compared on the int16 views, so the zero signs are pinned too.  Pins the
             j <-> F + j pairing, every address and the grid walk.  (+-129 is in the set because a power of two
             times an integer below 128 has at most 7 significant bits and never rounds in bf16: 129 * 127
             needs a rounding and 129 * 3 = 387 is a rounding tie.)
  true       randn g and u: |out - ref| <= (2^-8 + 2^-16) * |ref| against float64 g / (1 + exp(-g)) * u on the
             bf16 inputs.  2^-8 is the one bf16 rounding.  The fp32 product g * log2e and the constant put at
             most |g| * 2^-23 relative into e, under 2^-20 for |g| <= 8; v_exp_f32 is documented at 1 ulp; the
             relative error of 1 + e is below that of e; the division and the product add 2^-24 each: together
             below 2^-19.  2^-16 leaves a factor of 8, because the instruction's accuracy is taken from
             documentation, not from a measurement.  The measured maximum of error / bound is printed
             (MEASURED below).
"""
import functools
import json
import subprocess
import sys

import pytest
import torch

import test_gpu_corun_exact as CO
from test_gpu_kernels_exact import NAN, SENT16, guarded_input, guarded_output, guards_intact

pytestmark = pytest.mark.gpu

# MEASURED on an MI355X (printed by the tests):
MEASURED = """
  true regime, max |out - ref| / bound per (T, F): 0.7106 (1, 8), 0.8266 (1, 16), 0.9400 .. 0.9909 for the larger
  shapes -- every error was below 2^-8 * |ref|, the bf16 rounding's share alone, so the 2^-16 allowed for the fp32
  terms, v_exp_f32 among them, was not needed.  llm_block_decode_256, 8 picked rows: 0.9917; llm_block_prefill_2048: 0.9917.
  Every saturated-regime, large-address and co-run output bit-exact.
  The module: 37 tests in 14 s, 7 s of them the two podrun processes.
"""

C0, R0 = 8, 2
SHAPES = ((1, 8), (1, 16), (3, 1016), (3, 1024), (3, 1032), (1, 8192), (1, 8200), (5, 14336))
REGIMES = ("saturated", "true")
G_VALUES = (0.0, -0.0, 128.0, -128.0, 129.0, -129.0, 256.0, -256.0, 512.0, -512.0)
TRUE_BOUND = 2.0 ** -8 + 2.0 ** -16
LOG2E = 1.44269504088896340736
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
def emulate(gate_up):
    """The contract in fp32 on the CPU, with torch's exp2 in the hardware exponential's place."""
    F = gate_up.shape[1] // 2
    g, u = gate_up[:, :F].float(), gate_up[:, F:].float()
    e = torch.exp2(-g * torch.tensor(LOG2E, dtype=torch.float32))
    return ((g / (1.0 + e)) * u).to(torch.bfloat16)


def reference(gate_up):
    F = gate_up.shape[1] // 2
    g, u = gate_up[:, :F].double(), gate_up[:, F:].double()
    return g / (1.0 + torch.exp(-g)) * u


def saturated_expected(gate_up):
    """bf16 out of a saturated gate_up, from the contract's consequences alone."""
    F = gate_up.shape[1] // 2
    g, u = gate_up[:, :F].float(), gate_up[:, F:].float()
    assert bool(((g == 0) | (g.abs() >= 128)).all()) and bool(g.isfinite().all())
    s = torch.where(g <= -128, torch.tensor(-0.0), g)                # g >= 128: s == g; g = +-0: s = +-0
    p = s * u
    assert torch.equal(p.double(), s.double() * u.double())          # an exact fp32 product
    return p.to(torch.bfloat16)


def operands(regime, T, F, seed):
    """gate_up bf16 [T, 2F] on the CPU."""
    g = torch.Generator().manual_seed(seed)
    if regime == "saturated":
        gate = torch.tensor(G_VALUES)[torch.randint(len(G_VALUES), (T, F), generator=g)]
        order = torch.rand(T, 255, generator=g).argsort(-1) - 127                       # the integers of [-127, 127]
        up = order.repeat(1, -(-F // 255))[:, :F].float() * (2.0 ** (torch.arange(T) % 7 - 3))[:, None]
    else:
        gate = torch.randn(T, F, generator=g).to(torch.bfloat16).float()
        up = torch.randn(T, F, generator=g).to(torch.bfloat16).float()
        gate[gate == 0] = 1.0
        up[up == 0] = 1.0
    gu = torch.cat([gate, up], dim=1).to(torch.bfloat16)
    assert torch.equal(gu.float(), torch.cat([gate, up], dim=1))     # exact in bf16 (+-0 compare equal; kept by the cast)
    return gu


class Case:
    def __init__(self, regime, T, F, seed, plant=None):
        self.regime, self.T, self.F = regime, T, F
        gu = operands(regime, T, F, seed)
        if plant:
            plant(gu)
        self.gu_host = gu
        if regime == "saturated" and not plant:
            self.exp = saturated_expected(gu)
        else:
            self.exp = emulate(gu)
        if regime == "true":
            self.ref = reference(gu)
            self.bound = TRUE_BOUND * self.ref.abs()
        self.gate_up = guarded_input(gu.cuda(), 2 * F + C0, c0=C0)
        self.outs = self.new_outputs()
        assert self.gate_up.data_ptr() % 16 == 0

    def new_outputs(self):
        return guarded_output(self.T, self.F, self.F + C0, C0, "cuda")

    @staticmethod
    def resentinel(outs):
        outs[0].fill_(SENT16)

    def launch(self, outs, **kw):
        from k8s_gpu_scheduler_amd.ops import loadgen
        return loadgen.swiglu(self.gate_up, out=outs[1], **kw)

    def run(self, **kw):
        self.resentinel(self.outs)
        return self.launch(self.outs, **kw)

    def results(self, outs=None):
        raw, out = self.outs if outs is None else outs
        torch.cuda.synchronize()
        assert guards_intact(raw, (slice(R0, R0 + self.T), slice(C0, C0 + self.F)), SENT16), "write outside out's window"
        return out.cpu()

    def check(self, what, outs=None):
        got = self.results(outs)
        if self.regime == "saturated":
            same = bits(got) == bits(self.exp)
            if not bool(same.all()):
                r, c = (~same).nonzero()[0].tolist()
                raise AssertionError((what, f"{int((~same).sum())} elements differ, first at [{r}, {c}]: got "
                                            f"{got[r, c].item()}, expected {self.exp[r, c].item()}"))
            return
        err = (got.double() - self.ref).abs()
        ratio = (err / self.bound.clamp_min(1e-300)).max().item()
        print(f"swiglu, true regime {what}: max |out - ref| / bound = {ratio:.4f}")
        assert bool((err <= self.bound).all()), (what, ratio)

    def untouched(self, outs=None):
        raw, _ = self.outs if outs is None else outs
        torch.cuda.synchronize()
        return guards_intact(raw, (slice(0, 0), slice(0, 0)), SENT16)


@functools.lru_cache(maxsize=None)
def case(regime, T, F):
    return Case(regime, T, F, seed=9500 + 100 * REGIMES.index(regime) + SHAPES.index((T, F)))


# ------------------------------------------------------------------------------------------------
# 1. the regimes over every shape
# ------------------------------------------------------------------------------------------------
def test_the_shapes_cover_the_grid_walk():
    from k8s_gpu_scheduler_amd.models.workloads import default_swiglu_workgroups as wg
    chunks = {(t, f): t * f // 8 for t, f in SHAPES}
    assert all(f % 8 == 0 for _, f in SHAPES)
    assert chunks[(1, 8)] == 1 and chunks[(1, 16)] == 2                               # a single chunk; two threads
    assert any(256 < t * (f // 8) < 512 and (f // 8) % 256 for t, f in SHAPES)        # ends inside a thread's second chunk
    assert any(t > 1 and (f // 8) % 64 and t * (f // 8) <= 1024 for t, f in SHAPES)   # a row boundary inside a wave's load
    assert any(t > 1 and wg(t, f) == 1 for t, f in SHAPES)                            # a row boundary inside a workgroup
    assert any(c == 1024 for c in chunks.values()) and any(c == 1025 for c in chunks.values())   # one workgroup; one chunk more
    assert any(wg(t, f) == 9 and (t * f // 8) % 1024 for t, f in SHAPES)              # a ragged ninth workgroup
    assert any((f // 8) % 1024 and t * (f // 8) > 1024 and t > 1 for t, f in SHAPES)  # a row boundary not at a workgroup's edge


@pytest.mark.parametrize("T,F", SHAPES)
@pytest.mark.parametrize("regime", REGIMES)
def test_regimes(hip, regime, T, F):
    c = case(regime, T, F)
    c.run()
    c.check((regime, T, F))


def test_two_launches_are_bit_identical(hip):
    c = case("true", 5, 14336)
    a, b = c.new_outputs(), c.new_outputs()
    c.launch(a)
    c.launch(b)
    assert torch.equal(bits(c.results(a)), bits(c.results(b)))


# ------------------------------------------------------------------------------------------------
# 2. non-finite values
# ------------------------------------------------------------------------------------------------
def test_nonfinite_values_touch_only_their_own_element(hip):
    T, F, seed = 3, 1032, 9701
    cells = {(0, 5): ("g", NAN), (0, 700): ("u", NAN), (1, 0): ("g", INF), (1, 1031): ("g", -INF), (2, 8): ("u", INF),
             (2, 519): ("u", -INF), (1, 300): ("gu", (INF, 0.0))}

    def plant(gu):
        for (r, j), (which, v) in cells.items():
            if which == "gu":
                gu[r, j], gu[r, F + j] = v
            else:
                gu[r, j + (F if which == "u" else 0)] = v
    clean, dirty = Case("true", T, F, seed), Case("true", T, F, seed, plant=plant)
    clean.run()
    dirty.run()
    was, got = clean.results(), dirty.results()
    hit = torch.zeros(T, F, dtype=torch.bool)
    for cell in cells:
        hit[cell] = True
    assert torch.equal(bits(got)[~hit], bits(was)[~hit]), "a non-finite value reached another element"
    assert not bool(got[hit].float().isfinite().any())
    assert bool(got[0, 5].isnan()) and bool(got[0, 700].isnan())
    assert bool(got[1, 1031].isnan()), "g = -Inf must give NaN (-Inf / Inf), as torch.nn.functional.silu does"
    assert bool(torch.nn.functional.silu(torch.tensor(-INF)).isnan())
    g, u = dirty.gu_host[:, :F].float(), dirty.gu_host[:, F:].float()
    assert got[1, 0].item() == (INF if u[1, 0] > 0 else -INF)                         # +Inf * u
    assert bool(got[1, 300].isnan())                                                  # +Inf * 0
    silu = lambda v: v / (1 + torch.exp(-v))                                          # noqa: E731
    assert got[2, 8].item() == (INF if silu(g[2, 8]) > 0 else -INF) and got[2, 519].item() == (-INF if silu(g[2, 519]) > 0 else INF)


# ------------------------------------------------------------------------------------------------
# 3. other launch paths
# ------------------------------------------------------------------------------------------------
def test_side_stream_and_graph_replay(hip):
    c = case("saturated", 3, 1032)
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
        if k == 0:                       # the second replay writes over the first: idempotent
            c.resentinel(c.outs)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        s.synchronize()
        c.check(("replay", k))


@pytest.mark.parametrize("breakage", ["out-in-gate_up", "odd-F", "fp32", "out-shape", "odd-stride", "misaligned", "out-stride"])
def test_a_bad_call_raises_and_launches_nothing(hip, breakage):
    from k8s_gpu_scheduler_amd.ops import loadgen
    c = case("saturated", 3, 1032)
    T, F = 3, 1032
    gu, out = c.gate_up, c.outs[1]
    if breakage == "out-in-gate_up":
        out = gu[:, :F]
    elif breakage == "odd-F":
        gu = gu[:, :2 * F - 8]
    elif breakage == "fp32":
        gu = gu.float()
    elif breakage == "out-shape":
        out = out[:2]
    elif breakage == "odd-stride":
        gu = torch.zeros(T, 2 * F + 4, dtype=torch.bfloat16, device="cuda")[:, :2 * F]
    elif breakage == "misaligned":
        gu = torch.zeros(T * 2 * F + 8, dtype=torch.bfloat16, device="cuda")[4:4 + T * 2 * F].view(T, 2 * F)
    else:
        out = torch.zeros(T, 2 * F, dtype=torch.bfloat16, device="cuda")[:, ::2]
    before = bits(c.gate_up.cpu()).clone()
    c.resentinel(c.outs)
    with pytest.raises((ValueError, TypeError)):
        loadgen.swiglu(gu, out=out)
    assert c.untouched() and torch.equal(bits(c.gate_up.cpu()), before)


def test_workgroups_match_the_python_rule(hip):
    from k8s_gpu_scheduler_amd.models import workloads as W
    for T, F in SHAPES + ((0, 8), (256, 14336), (2048, 14336), (7, 8184), (2 ** 31 - 1, 8192)):
        assert hip.swiglu_workgroups(T, F) == W.default_swiglu_workgroups(T, F), (T, F)
    assert [hip.swiglu_workgroups(*s) for s in SHAPES] == [1, 1, 1, 1, 1, 1, 2, 9]
    assert hip.swiglu_workgroups(256, 14336) == 448 and hip.swiglu_workgroups(2048, 14336) == 3584


# ------------------------------------------------------------------------------------------------
# 4. row offsets beyond 4 GiB
# ------------------------------------------------------------------------------------------------
BIG_LD = 2 ** 30 + 8


def test_row_offsets_beyond_4_gib(hip):
    """gate_up with a row stride of 2^30 + 8 in an UNINITIALISED allocation of which only the window is filled:
    row 2 starts past 4 GiB."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    T, F = 3, 1024
    c = Case("saturated", T, F, 9702)
    raw = torch.empty(((T - 1) * BIG_LD + 2 * F + 2 * C0,), dtype=torch.int16, device="cuda")
    gu = raw.view(torch.bfloat16).as_strided((T, 2 * F), (BIG_LD, 1), C0)
    assert 2 * BIG_LD * 2 > 2 ** 32 and gu.data_ptr() % 16 == 0
    gu.copy_(c.gu_host.cuda())
    c.resentinel(c.outs)
    loadgen.swiglu(gu, out=c.outs[1])
    c.check("row stride 2^30 + 8")
    del raw, gu
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------
# 5. beside a co-running load
# ------------------------------------------------------------------------------------------------
class SwigluLaunch:
    """One launch on a Case's input into an output of its own (reset / enqueue / check, as the co-run module's
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
def test_swiglu_corun(hip, aggressor, mode):
    c = Case("saturated", 256, 2048, 9703)
    victim = CO.Load("swiglu-saturated", {}, [SwigluLaunch(c, ("saturated", 256, 2048, r)) for r in range(CO.R)])
    try:
        CO.corun(hip, victim, CO.aggressor_for(aggressor, mode), mode)
    finally:
        CO.restore_knobs(hip)


# ------------------------------------------------------------------------------------------------
# 6. pod path
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("workload", ["llm_block_decode_256", "llm_block_prefill_2048"])
def test_executor_llm_block_swiglu_output(hip, workload):
    """The executor's operands of the swiglu op and, after one iteration, 8 picked rows of its output against the
    reference."""
    from k8s_gpu_scheduler_amd.models import workloads as W
    from k8s_gpu_scheduler_amd.parallel.executor import _Buffers, enqueue_ops, op_output
    dev = torch.device("cuda", 0)
    a = _Buffers(W.get(workload), dev)
    (o, t), = [(o, t) for o, t in a.ops if o.kind == "swiglu"]
    out, gate_up = t
    assert a.ops[7][0] is o and op_output(o, t) is out
    assert gate_up.shape == (o.M, 2 * o.N) and out.shape == (o.M, o.N) and gate_up.dtype == out.dtype == torch.bfloat16
    out.view(torch.int16).fill_(SENT16)
    enqueue_ops(a, 1, torch.cuda.current_stream(), 0)
    torch.cuda.synchronize()
    rows = torch.tensor([0, 1, o.M // 3, o.M // 2, o.M // 2 + 1, o.M - 3, o.M - 2, o.M - 1], device=dev)
    ref = reference(gate_up[rows].cpu())
    err = (out[rows].cpu().double() - ref).abs()
    ratio = (err / (TRUE_BOUND * ref.abs()).clamp_min(1e-300)).max().item()
    print(f"{workload} swiglu, 8 rows: max |out - ref| / bound = {ratio:.4f}")
    assert bool((err <= TRUE_BOUND * ref.abs()).all()), ratio
    assert not bool((out.view(torch.int16) == SENT16).all(-1).any())                     # every row was written
    del a, t, out, gate_up
    torch.cuda.empty_cache()


@pytest.mark.parametrize("workload", ["llm_block_decode_256", "llm_block_prefill_2048"])
def test_podrun_llm_block(workload):
    p = subprocess.run([sys.executable, "-m", "k8s_gpu_scheduler_amd.ops.podrun", "--workload", workload,
                        "--iters", "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    assert res["workload"] == workload and res["iters"] == 2 and res["throughput"] > 0
