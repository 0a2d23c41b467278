"""Exact-arithmetic, guarded-buffer tests of every kernel while another pod's kernels run beside it
(run with `-m gpu` on an MI355X).

The exact modules (test_gpu_kernels_exact.py, test_gpu_gather_exact.py, test_gpu_decode_attn_exact.py)
launch one kernel at a time on an idle chip.  The bench never does: Burstable pods share all 256
CUs, Guaranteed pods share L2, fabric and HBM.  The pipelined GEMM kernels are correct only if
hand-counted vmcnt / lgkmcnt waits and one barrier per K-tile order the LDS-DMA writes against the
ds_reads, and a wait that is one too low passes whenever the DMA happens to land first -- which
depends on the memory load.  Here the same inputs (integer operands, `torch.equal` against float64,
NaN prefill, sentinel guards: one wrong element of any size fails) run as the *victim* on one
stream while an *aggressor* load runs on another, and the test proves with events that they
overlapped.

`corun(victim, aggressor, mode)`:

  streams    same-slice  both on their own MaskedStream(cu_slice_mask(0, 1)): the same 32 CUs, so
                         even a 6-block victim shares CUs with aggressor waves
             unmasked    two plain streams (Burstable: all 256 CUs).  The runtime spreads plain
                         streams over 4 hardware queues, and two on one queue run one after the
                         other (6 of 110 pairs did): the victim's stream is drawn from torch's
                         pool until a trivial kernel on it ends inside 16 triad passes on the
                         aggressor's (`runs_beside`)
             disjoint    masks of units 0 and 1 (Guaranteed: only L2 / fabric / HBM are shared)
             and a third, plain *gate* stream (below).  All are closed / dropped in `finally`.
  sizing     the victim block alone is timed by the host clock (first enqueue to sync), one
             aggressor pass alone by HIP events; ceil(4 t_victim / t_pass) + 2 passes are
             enqueued (`aggressor_passes`; more than 512 fails the test).  That count runs once
             as a rehearsal on which nothing is asserted, and the same rule is then fed with
             what the rehearsal measured wherever that asks for more passes: the victim's co-run
             time if longer than its time alone, the co-run time per pass if shorter than the
             lone pass.  Both happen.  The triad's 8192-block grid keeps every wave slot of
             shared CUs full, and a GEMM workgroup gets in only as a pass tails off: victims took
             up to 6.3 times their lone time (same-slice) and ended with the aggressor.  And a
             lone pass of a few launches is bound by its enqueueing: queued behind the gate the
             mixed pass took a quarter, the MFMA pass half of its lone time.
  order      the aggressor passes are enqueued first under the aggressor's knobs, then the victim's
             launches under the victim's: the set_* knobs are host statics read at launch.
  gate       a short aggressor pass (the 1024^3 MFMA pass takes ~10 us on the whole chip) is over
             before the host has enqueued the next, so without more the aggressor would have
             drained when the first victim launch arrives.  The aggressor stream therefore first
             waits for an event behind a run of HBM triad passes on the gate stream, sized to
             outlast twice the host time the rehearsal's enqueueing took (plus 0.5 ms for host
             jitter), and the victim stream waits for the aggressor's start event.  When the gate
             opens both queues are full.
  overlap    events before / after the aggressor passes and before / after the victim launches,
             all measured from one clock event: the victim interval must lie inside the aggressor
             interval (`victim_inside`), else the test fails as "no overlap" before any value is
             compared.
  checks     one sync, then every victim launch's own output (NaN-prefilled, or the window of a
             sentinel-filled allocation whose guards are compared bitwise) and the aggressor's
             last output are compared exactly.  No host sync happens between launches.

Every load also runs once alone on its stream first (loading its kernels) and is checked there, so
a failure says whether it needs the co-runner.

Victims run R = 4 launches per (regime, act): 16 launches per GEMM test (gather: 4 per case and
regime, 16; attention and triad: 4).  Aggressors: `stream` = the HBM triad over 3 x 96 MiB (more than the 256 MiB Infinity Cache),
`mfma` = the bf16 GEMM forced to tile 16 at 1024 x 1024 x 1088 (two 80 KiB blocks per CU), `mixed`
= one gather pass (the pooled case's bags 256 times over) and one decode-attention pass (the pair
case's sequences 64 times over).

Part 2 runs the DeviceExecutor's own co-run path (four pods, then two that wait for them, eager
and as captured graphs) on two tiny workloads and compares every op's output with a reference that
is independent of the kernels: exact for the gather and the triad, the attention module's derived
bound for the attention, and for the GEMMs

    |out - ref| <= 2^-8 |ref| + 1.01 (K + 1) 2^-23 (|a| @ |bt|^T),   ref = relu(a @ bt^T + bias)

in float64: half a bf16 ulp plus the any-order fp32 summation bound at unit roundoff 2^-23 (which
also covers a truncating accumulator).  `gemm_bound`, `victim_inside` and `aggressor_passes` are
tested on the CPU in test_corun_exact_helpers.py.

Measured on an MI355X (printed by every test; see MEASURED below).
"""
import contextlib
import functools
import math
import time

import pytest
import torch

import test_gpu_decode_attn_exact as ATT
import test_gpu_gather_exact as GAT
from test_gpu_kernels_exact import (FP8, NAN, PAD_ACTS, REGIMES, SENT16, SENT32, TILE_BM, TILE_BN, TRIAD_GUARD, TRIAD_S,
                                    WIDE_C, exact_match, expected, first_mismatch, gpu_case, guarded_input,
                                    guarded_output, guarded_vector, guards_intact, knobs, out_window, restore_knobs,
                                    small_triad, triad_buffers, triad_n)

pytestmark = pytest.mark.gpu

# MEASURED on an MI355X (victim slowdown = co-run event time / alone host time; aggressor slowdown
# = co-run event time of the n passes / n x the lone pass; ratio = largest error / bound):
MEASURED = """
  aggressor | mode        cases  victim slowdown  aggressor slowdown  passes   victim span / aggressor span (max)
  stream    | same-slice    46    0.47 .. 17.86     0.89 .. 1.02       4 .. 66    0.58  (tile 13, K = 320)
  stream    | unmasked      46    0.92 ..  5.47     0.74 .. 0.86      10 .. 130   0.31
  stream    | disjoint      14    0.34 ..  0.94     0.93 .. 0.98       6 .. 15    0.19
  mfma      | same-slice    46    0.30 ..  1.75     0.36 .. 0.68      15 .. 150   0.29
  mfma      | unmasked      46    0.29 ..  0.99     0.40 .. 0.59      22 .. 188   0.25
  mfma      | disjoint      14    0.29 ..  0.93     0.45 .. 0.67      40 .. 158   0.23
  mixed     | same-slice    14    0.66 ..  3.57     0.44 .. 0.82       7 .. 30    0.31
  mixed     | unmasked      14    0.49 ..  1.20     0.17 .. 0.33      23 .. 87    0.30
  mixed     | disjoint      14    0.25 ..  0.92     0.56 .. 0.78       7 .. 20    0.20
  stream    | graph replay   3    2.97 ..  3.23     0.87 .. 0.88      56          0.26
  (a victim slowdown below 1: the lone time is the host's, enqueueing included; queued behind the
  gate the launches run back to back.  With the first rule alone -- 4 lone victim times -- the
  stream aggressor's victims on shared CUs, at 5.1 and 6.3 lone times, outlasted the aggressor.)
  executor co-run, eager and graphs alike: largest GEMM error / bound 0.9247 (bf16 512 x 512 x 320)
  and 0.9463 (fp8 256 x 256 x 256) -- a bf16 half-ulp at a mantissa just above a power of two is
  nearly 2^-8 of the value; attention max|out - ref| = 0.00116 against the bound 0.01550; gather and
  triad bit-exact.  The whole module: 257 tests in 13 s, R = 4 kept everywhere.
"""

R = 4                                   # victim launches per (regime, act)
MAX_PASSES = 512                        # aggressor passes per co-run; needing more fails the test
MAX_GATE_PASSES = 4096
GATE_SLACK_S = 0.5e-3                   # host jitter the gate allows for on top of the measured enqueue time
MODES = ("same-slice", "unmasked", "disjoint")
FORCED_TILES = (1, 3, 10, 11, 12, 13, 14, 15, 16)
FORCED_KS = (128, 320, 1088)            # 2 K-tiles, 5 (the ring size), a long loop
WIDE_VICTIM_TILES = (10, 14, 16)        # also run against `mixed` and under `disjoint`
STREAM_FLOATS = 24 << 20                # per array: 3 x 96 MiB > the 256 MiB Infinity Cache
MFMA_SHAPE = (1024, 1024, 1088)
GATHER_REPEAT, ATTN_REPEAT = 256, 64    # the mixed aggressor's cases, repeated on the device
BASE_PAIRS = [(a, m) for a in ("stream", "mfma") for m in ("same-slice", "unmasked")]
ALL_PAIRS = [(a, m) for a in ("stream", "mfma", "mixed") for m in MODES]


# ------------------------------------------------------------------------------------------------
# helpers (CPU-tested in test_corun_exact_helpers.py)
# ------------------------------------------------------------------------------------------------
def victim_inside(a0, a1, v0, v1):
    """True iff the victim interval [v0, v1] is a proper interval inside the aggressor's [a0, a1]."""
    return a0 <= v0 < v1 <= a1


def aggressor_passes(t_victim, t_pass, cap=MAX_PASSES):
    """Aggressor passes to enqueue in front of a victim block that takes t_victim alone, a pass
    taking t_pass alone: four victim times (the factor absorbs the mutual slowdown) and two
    passes.  Needing more than `cap` is an error, not something to clip."""
    assert t_victim > 0 and t_pass > 0, (t_victim, t_pass)
    n = math.ceil(4 * t_victim / t_pass) + 2
    if n > cap:
        raise AssertionError(f"{n} aggressor passes needed (cap {cap}): the victim block takes {t_victim * 1e3:.3f} ms "
                             f"alone, one aggressor pass {t_pass * 1e3:.4f} ms")
    return n


def gate_passes(t_hold, t_gate_pass, t_gate_enqueue, cap=MAX_GATE_PASSES):
    """Gate passes that keep the gate stream busy for t_hold (twice over) after the host has
    enqueued them: each pass buys its device time less its own enqueue time."""
    lead = t_gate_pass - t_gate_enqueue
    assert lead > 0.25 * t_gate_pass, f"the gate pass ({t_gate_pass * 1e6:.1f} us) hardly outlasts its enqueue ({t_gate_enqueue * 1e6:.1f} us)"
    n = math.ceil(2 * t_hold / lead) + 2
    assert n <= cap, f"{n} gate passes needed (cap {cap}) to hold {t_hold * 1e3:.3f} ms"
    return n


def gemm_bound(a, bt, bias):
    """(ref, bound) in float64 for out = bf16(relu(a @ bt^T + bias)) accumulated in fp32 in any
    order: half a bf16 ulp of the reference plus (K + 1) unit roundoffs 2^-23 of |a| @ |bt|^T."""
    a, bt = a.double(), bt.double()
    K = a.shape[1]
    ref = (a @ bt.T + bias.double()).clamp_min(0.0)
    bound = 2.0 ** -8 * ref.abs() + 1.01 * (K + 1) * 2.0 ** -23 * (a.abs() @ bt.abs().T)
    return ref, bound


def victim_shapes():
    """Every (M, N, K, fp8) this module runs in the representable regime (the cap of `expected` is
    checked for them on the CPU)."""
    shapes = {(2 * TILE_BM[t], 3 * TILE_BN[t], K, False) for t in FORCED_TILES for K in FORCED_KS}
    shapes.add((2 * TILE_BM[9], 3 * TILE_BN[9], 320, False))
    shapes.update((512, 512, K, False) for K in FORCED_KS)
    shapes.update((M, N, K, True) for (M, N) in ((128, 192), (256, 256)) for K in (128, 384))
    shapes.update({(256, 256, 2048, False), (1024, 512, 256, False), MFMA_SHAPE + (False,)})
    return sorted(shapes)


def tiny_workloads():
    """The two workloads of the executor test: GEMM + triad + fp8 GEMM, and a gather over more table
    rows than one generated block plus an attention over more cache blocks than one pattern (75,
    no multiple of it)."""
    from k8s_gpu_scheduler_amd.models.workloads import Op, Workload
    return (Workload("t_mix", "test", "hip", 512, (Op("gemm", 512, 512, 320), Op("triad", n_floats=1 << 20),
                                                   Op("gemm8", 256, 256, 256)), 0.1),
            Workload("t_idx", "test", "hip", 300, (Op("gather", 300, 128, 8, rows=5000),
                                                   Op("attn", 5, 8, 480, rows=2)), 0.1))


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


class GemmLaunch:
    def __init__(self, fn, a, bt, bias, relu, cu_budget, exp, regime, pad, what):
        M, N = exp.shape
        self.fn, self.a, self.bt, self.bias, self.relu, self.cu_budget = fn, a, bt, bias, relu, cu_budget
        self.exp, self.regime, self.pad, self.what = exp, regime, pad, what
        if pad is None:
            self.raw, self.out = None, torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
        else:
            self.raw, self.out = guarded_output(M, N, N + pad[0], pad[1], "cuda")

    def reset(self):
        if self.raw is None:
            self.out.fill_(NAN)
        else:
            self.raw.fill_(SENT16)

    def enqueue(self, st):
        self.fn(self.a, self.bt, out=self.out, bias=self.bias, relu=self.relu, stream=st, cu_budget=self.cu_budget)

    def check(self, tag):
        assert exact_match(self.out, self.exp, self.regime), (tag, self.what, first_mismatch(self.out, self.exp))
        if self.raw is not None:
            M, N = self.exp.shape
            assert guards_intact(self.raw, out_window(M, N, self.pad[1]), SENT16), ("write outside the C window", tag, self.what)


class TriadLaunch:
    def __init__(self, b, c, ref, blocks, what):
        self.b, self.c, self.ref, self.blocks, self.what = b, c, ref, blocks, what
        self.raw, self.a = guarded_vector(ref.numel(), *TRIAD_GUARD, "cuda")
        assert self.a.data_ptr() % 16 == 0

    def reset(self):
        self.raw.fill_(SENT32)

    def enqueue(self, st):
        from k8s_gpu_scheduler_amd.ops import loadgen
        loadgen.triad(self.a, self.b, self.c, TRIAD_S, blocks=self.blocks, stream=st)

    def check(self, tag):
        assert torch.equal(self.a, self.ref), (tag, self.what, int((self.a != self.ref).sum().item()), "elements differ")
        before = TRIAD_GUARD[0]
        assert guards_intact(self.raw, slice(before, before + self.a.numel()), SENT32), ("write outside a", tag, self.what)


class CaseLaunch:
    """One launch on the inputs of a Case of the gather or the attention module into an output of
    its own; checked by the Case's own check, which is pointed at that output for the call."""

    def __init__(self, case, rows, width, launch, what, **attrs):
        self.case, self.launch, self.what = case, launch, what
        self.raw, self.out = guarded_output(rows, width, width + GAT.C0, GAT.C0, "cuda")
        assert self.out.data_ptr() % 16 == 0
        self.attrs = attrs

    def reset(self):
        self.raw.fill_(SENT16)

    def enqueue(self, st):
        self.launch(self.out, st)

    def check(self, tag):
        c = self.case
        attrs = dict(self.attrs, raw=self.raw, out=self.out if isinstance(c, GAT.Case) else self.out.unflatten(1, (c.Hq, ATT.D)))
        saved = {k: getattr(c, k) for k in attrs}
        try:
            for k, v in attrs.items():
                setattr(c, k, v)
            c.check((tag, self.what))
        finally:
            for k, v in saved.items():
                setattr(c, k, v)


class Load:
    """A block of launches with the knob settings they are enqueued under."""

    def __init__(self, name, settings, launches):
        self.name, self.settings, self.launches = name, settings, launches

    def reset(self):
        for x in self.launches:
            x.reset()

    def enqueue(self, hip, st, times=1):
        with knobs(hip, **self.settings):
            for _ in range(times):
                for x in self.launches:
                    x.enqueue(st)

    def check(self, tag):
        for x in self.launches:
            x.check((self.name, tag))


def gemm_load(name, M, N, K, cu_budget, padded, fp8=False, regimes=REGIMES, acts=PAD_ACTS, repeats=R, **settings):
    """`repeats` launches per (regime, act) of the exact operands of test_gpu_kernels_exact; padded:
    the NaN-guarded, offset operand views and sentinel-guarded C windows of its part B."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    fn = loadgen.gemm_fp8 if fp8 else loadgen.gemm
    launches = []
    for regime in regimes:
        a, bt, bias, ref = gpu_case(M, N, K, regime, fp8)
        if padded:
            ea, eb, c0 = (80, 144, 16) if fp8 else (72, 136, 8)       # as run_exact: lda != ldb, neither is K
            a, bt = guarded_input(a, K + ea, c0=c0), guarded_input(bt, K + eb, r0=1, c0=2 * c0)
        for relu, use_bias in acts:
            exp = expected(ref, bias, relu, use_bias, regime)
            for r in range(repeats):
                what = (M, N, K, regime, "relu" if relu else "-", "bias" if use_bias else "-", cu_budget, padded, r)
                launches.append(GemmLaunch(fn, a, bt, bias if use_bias else None, relu, cu_budget, exp, regime,
                                           WIDE_C if padded else None, what))
    return Load(name, settings, launches)


def gather_load():
    """The pooled case (37 bags of 5 rows on a grid of 3 workgroups: grid-stride trips and a tail,
    through the 2-D idx form) and the long-bag case (CSR offsets) at D = 128, both regimes."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    launches = []
    for regime in GAT.REGIMES:
        p, lb = GAT.pooled_case(37, regime), GAT.long_bag_case(128, regime)

        def pooled(out, st, c=p):
            loadgen.embedding_bag(c.table, c.idx.view(c.B, GAT.POOL), out=out, blocks=3, stream=st, check_indices=False)

        def long_bags(out, st, c=lb):
            loadgen.embedding_bag(c.table, c.idx, c.offsets, out=out, stream=st, check_indices=False)

        for c, fn, nm in ((p, pooled, "pooled"), (lb, long_bags, "long")):
            launches += [CaseLaunch(c, c.B, c.D, fn, (nm, regime, r)) for r in range(R)]
    return Load("gather", {}, launches)


def attention_launch(c, q, table, ctx):
    from k8s_gpu_scheduler_amd.ops import loadgen

    def launch(out, st):
        loadgen.paged_decode_attention(q, c.kc, c.vc, table, ctx, out=out.unflatten(1, (c.Hq, ATT.D)), stream=st, check=False)
    return launch


def attention_load(regime, group, hkv):
    c = ATT.case(regime, group, hkv)
    return Load(f"attn-{regime}", {}, [CaseLaunch(c, c.S, c.Hq * ATT.D, attention_launch(c, c.q, c.table, c.ctx), (regime, group, hkv, r))
                                       for r in range(R)])


def triad_load(variant):
    _, _, b, c, ref = small_triad(triad_n(3))
    return Load(f"triad-v{variant}", {"triad_variant": variant}, [TriadLaunch(b, c, ref, 3, (variant, r)) for r in range(R)])


@functools.lru_cache(maxsize=None)
def stream_aggressor():
    _, _, b, c, ref = triad_buffers(STREAM_FLOATS, seed=11)
    assert 3 * 4 * STREAM_FLOATS > 256 << 20
    return Load("stream", {}, [TriadLaunch(b, c, ref, 0, "stream aggressor")])


@functools.lru_cache(maxsize=None)
def mfma_aggressor(cu_budget):
    return gemm_load("mfma", *MFMA_SHAPE, cu_budget, False, regimes=("rep",), acts=[(True, True)], repeats=1, gemm_tile=16)


@functools.lru_cache(maxsize=None)
def mixed_aggressor():
    from k8s_gpu_scheduler_amd.ops import loadgen
    g, a = GAT.pooled_case(37, "rnd"), ATT.case("pair", 4, 2)
    idx = g.idx.repeat(GATHER_REPEAT).view(g.B * GATHER_REPEAT, GAT.POOL)

    def gather(out, st):
        loadgen.embedding_bag(g.table, idx, out=out, stream=st, check_indices=False)

    q, table, ctx = a.q.repeat(ATTN_REPEAT, 1, 1), a.table.repeat(ATTN_REPEAT, 1), a.ctx.repeat(ATTN_REPEAT)
    return Load("mixed", {}, [
        CaseLaunch(g, g.B * GATHER_REPEAT, g.D, gather, "mixed aggressor: gather", B=g.B * GATHER_REPEAT,
                   exp=g.exp.repeat(GATHER_REPEAT, 1)),
        CaseLaunch(a, a.S * ATTN_REPEAT, a.Hq * ATT.D, attention_launch(a, q, table, ctx), "mixed aggressor: attention",
                   S=a.S * ATTN_REPEAT, ctxs=a.ctxs * ATTN_REPEAT, exp=a.exp.repeat(ATTN_REPEAT, 1, 1))])


def aggressor_for(kind, mode):
    if kind == "stream":
        return stream_aggressor()
    if kind == "mfma":
        return mfma_aggressor(0 if mode == "unmasked" else 32)
    return mixed_aggressor()


def budget_of(mode):
    return 0 if mode == "unmasked" else 32


PLAIN_DRAWS = 8


def runs_beside(hip, sv, sa):
    """True iff a trivial kernel on sv, enqueued behind the start event of 16 HBM triad passes on
    sa, ends before they do.  Two plain streams that the runtime put on one hardware queue (it
    has 4 by default) run one after the other instead."""
    load, scratch = stream_aggressor(), torch.zeros(256, device="cuda")
    load.reset()
    torch.cuda.synchronize()

    def passes(a0):
        a0.record(sa)
        load.enqueue(hip, sa, 16)

    def trivial():
        with torch.cuda.stream(sv):
            scratch.fill_(1.0)

    _, (_, ta1, _, tv1) = enqueue_both(passes, trivial, sv, sa)
    return tv1 < ta1


@contextlib.contextmanager
def streams_for(hip, mode):
    """(victim stream, aggressor stream, gate stream): three non-default streams, the masked ones
    closed afterwards.  A masked stream has a hardware queue of its own; plain streams share the
    runtime's few, so the victim's is drawn again (from torch's pool: nothing is created or kept)
    until it demonstrably runs beside the aggressor's."""
    from k8s_gpu_scheduler_amd.ops.cumask import MaskedStream
    from k8s_gpu_scheduler_amd.plugins.gpu.devices import cu_slice_mask
    masked = []
    try:
        if mode == "unmasked":
            sa = torch.cuda.Stream()
            for _ in range(PLAIN_DRAWS):
                sv = torch.cuda.Stream()
                if runs_beside(hip, sv, sa):
                    break
            else:
                pytest.fail(f"no overlap: none of {PLAIN_DRAWS} plain streams ran beside the aggressor's (one hardware queue?)")
        else:
            masked.append(MaskedStream(cu_slice_mask(0, 1)))
            masked.append(MaskedStream(cu_slice_mask(1 if mode == "disjoint" else 0, 1)))
            sv, sa = masked[0].stream, masked[1].stream
        yield sv, sa, torch.cuda.Stream()
    finally:
        torch.cuda.synchronize()
        for m in masked:
            m.close()


def run_alone(hip, load, st, times=1):
    """Warm-up run with a check, then a timed one of `times` passes: per pass, (host seconds from
    the first enqueue to the sync, host seconds of the enqueueing, device seconds between events
    around the block)."""
    load.reset()
    torch.cuda.synchronize()
    load.enqueue(hip, st)
    torch.cuda.synchronize()
    load.check("alone")
    load.reset()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(st)
    load.enqueue(hip, st, times)
    e1.record(st)
    t1 = time.perf_counter()
    st.synchronize()
    t2 = time.perf_counter()
    return (t2 - t0) / times, (t1 - t0) / times, e0.elapsed_time(e1) * 1e-3 / times


class Sizing:
    """The times measured alone: the victim block (host clock, first enqueue to sync), one
    aggressor pass (events), one gate pass (events, over a run of 8) and the host's enqueue times."""

    def __init__(self, hip, victim, aggressor, sv, sa, sg):
        self.t_victim, self.t_victim_enqueue, _ = run_alone(hip, victim, sv)
        _, self.t_pass_enqueue, self.t_pass = run_alone(hip, aggressor, sa)
        _, self.t_gate_enqueue, self.t_gate = run_alone(hip, stream_aggressor(), sg, times=8)
        self.n = aggressor_passes(self.t_victim, self.t_pass)
        self.host = self.n * self.t_pass_enqueue + self.t_victim_enqueue         # a first estimate, for the rehearsal

    def gate(self, host_seconds):
        return gate_passes(host_seconds + GATE_SLACK_S, self.t_gate, self.t_gate_enqueue)

    def resize(self, times, host_seconds):
        """After a rehearsal with self.n passes: the same rule fed with what the rehearsal showed
        where that asks for more -- the victim's co-run time if longer than alone (a saturating
        stream aggressor starves big workgroups: x 6 on shared CUs), the co-run time per pass if
        shorter (queued passes run back to back; alone, a short pass is bound by its enqueue)."""
        ta0, ta1, tv0, tv1 = times
        n = aggressor_passes(max(self.t_victim, (tv1 - tv0) * 1e-3), min(self.t_pass, (ta1 - ta0) * 1e-3 / self.n))
        self.host, self.n = host_seconds * max(1.0, n / self.n), max(n, self.n)


def enqueue_both(enqueue_aggressor, enqueue_victim, sv, sa):
    """The aggressor first, then the victim behind the aggressor's start event; one sync.  Returns
    (host seconds of the enqueueing, (aggressor start, end, victim start, end) in ms after one
    clock event)."""
    clock, a0, a1, v0, v1 = (torch.cuda.Event(enable_timing=True) for _ in range(5))
    clock.record(torch.cuda.current_stream())
    t0 = time.perf_counter()
    enqueue_aggressor(a0)
    a1.record(sa)
    sv.wait_event(a0)
    v0.record(sv)
    enqueue_victim()
    v1.record(sv)
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return host, tuple(clock.elapsed_time(e) for e in (a0, a1, v0, v1))


def assert_overlap(what, z, times):
    """Prints the slowdowns; fails as "no overlap" unless the victim ran inside the aggressor."""
    ta0, ta1, tv0, tv1 = times
    print(f"corun {what}: {z.n} passes, victim {z.t_victim * 1e3:.3f} ms alone (host) -> {tv1 - tv0:.3f} ms co-run (events), "
          f"slowdown {(tv1 - tv0) / (z.t_victim * 1e3):.2f}; aggressor pass {z.t_pass * 1e3:.4f} ms alone -> "
          f"{(ta1 - ta0) / z.n:.4f} ms co-run, slowdown {(ta1 - ta0) / (z.n * z.t_pass * 1e3):.2f}; "
          f"aggressor [{ta0:.3f}, {ta1:.3f}] victim [{tv0:.3f}, {tv1:.3f}] ms")
    assert victim_inside(ta0, ta1, tv0, tv1), (
        f"no overlap ({what}): the victim ran [{tv0:.3f}, {tv1:.3f}] ms, the aggressor's {z.n} passes [{ta0:.3f}, {ta1:.3f}] ms "
        f"(alone: victim {z.t_victim * 1e3:.3f} ms, pass {z.t_pass * 1e3:.4f} ms)")


def corun(hip, victim, aggressor, mode):
    what = f"{victim.name} | {aggressor.name} | {mode}"
    with streams_for(hip, mode) as (sv, sa, sg):
        z = Sizing(hip, victim, aggressor, sv, sa, sg)

        def attempt():
            n, n_gate, gate = z.n, z.gate(z.host), torch.cuda.Event()
            victim.reset()
            aggressor.reset()
            torch.cuda.synchronize()

            def enqueue_aggressor(a0):
                stream_aggressor().enqueue(hip, sg, n_gate)
                gate.record(sg)
                sa.wait_event(gate)
                a0.record(sa)
                aggressor.enqueue(hip, sa, n)

            return enqueue_both(enqueue_aggressor, lambda: victim.enqueue(hip, sv), sv, sa)

        host, times = attempt()               # the rehearsal: nothing is asserted on it
        z.resize(times, host)
        _, times = attempt()
        assert_overlap(what, z, times)
        victim.check(("co-run", aggressor.name, mode))
        aggressor.check(("co-run aggressor", victim.name, mode))


# ------------------------------------------------------------------------------------------------
# 1. every kernel as the victim
# ------------------------------------------------------------------------------------------------
def _ids(cases):
    return [pytest.param(*c, id="-".join(str(x) for x in c)) for c in cases]


def forced_tile_cases():
    cases = []
    for tile in FORCED_TILES:
        for K in FORCED_KS:
            cases += [(tile, 0, K, a, m) for a, m in (ALL_PAIRS if tile in WIDE_VICTIM_TILES else BASE_PAIRS)]
    cases += [(9, 0, 320, a, m) for a, m in BASE_PAIRS]
    cases += [(14, 1, K, a, m) for K in FORCED_KS for a, m in BASE_PAIRS]           # tile 14 with set_w4_prio(1)
    return [pytest.param(*c, id=f"tile{c[0]}{'prio' if c[1] else ''}-K{c[2]}-{c[3]}-{c[4]}") for c in cases]


@pytest.mark.parametrize("tile,prio,K,aggressor,mode", forced_tile_cases())
def test_forced_tile_corun(hip, tile, prio, K, aggressor, mode):
    """2 x 3 blocks of the forced tile (every wave role, m0 and n0 != 0); at a 32-CU share with
    padded, guarded operands under a mask, on the whole chip without."""
    M, N, cu = 2 * TILE_BM[tile], 3 * TILE_BN[tile], budget_of(mode)
    settings = dict(gemm_tile=tile, w4_prio=1) if prio else dict(gemm_tile=tile)
    with knobs(hip, **settings):
        assert hip.pick_gemm_tile(M, N, cu) == tile
    corun(hip, gemm_load(f"tile{tile}{'prio' if prio else ''}-{M}x{N}x{K}", M, N, K, cu, mode != "unmasked", **settings),
          aggressor_for(aggressor, mode), mode)


@pytest.mark.parametrize("aggressor,mode", _ids(BASE_PAIRS))
@pytest.mark.parametrize("K", FORCED_KS)
def test_policy10_tile14_corun(hip, K, aggressor, mode):
    """The 4-wave kernel as the default picker launches it at a 4-CU share."""
    with knobs(hip, gemm_policy=10):
        assert hip.pick_gemm_tile(512, 512, 4) == 14
    corun(hip, gemm_load(f"policy10-512x512x{K}", 512, 512, K, 4, mode != "unmasked", gemm_policy=10),
          aggressor_for(aggressor, mode), mode)


@pytest.mark.parametrize("aggressor,mode", _ids(ALL_PAIRS))
@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("M,N,cu_budget,blocks", [pytest.param(128, 192, 0, 6, id="fp8-64x64-128x192"),
                                                  pytest.param(256, 256, 4, 4, id="fp8-128x128-256x256")])
def test_fp8_corun(hip, M, N, cu_budget, blocks, K, aggressor, mode):
    assert hip.gemm_workgroups(M, N, K, cu_budget, True) == blocks
    corun(hip, gemm_load(f"fp8-{M}x{N}x{K}", M, N, K, cu_budget, mode != "unmasked", fp8=True), aggressor_for(aggressor, mode), mode)


@pytest.mark.parametrize("aggressor,mode", _ids(ALL_PAIRS))
def test_split_k_corun(hip, aggressor, mode):
    """fp32 partials in a workspace from the caching allocator, then the reduce kernel."""
    M, N, K = 256, 256, 2048
    with knobs(hip, split_k=-1):
        assert hip.pick_split_k(M, N, K) > 1
    corun(hip, gemm_load(f"splitk-{M}x{N}x{K}", M, N, K, 0, mode != "unmasked", split_k=-1), aggressor_for(aggressor, mode), mode)


@pytest.mark.parametrize("aggressor,mode", _ids(BASE_PAIRS))
def test_policy9_row_slices_corun(hip, aggressor, mode):
    M, N, K = 1024, 512, 256
    with knobs(hip, gemm_policy=9):
        assert hip.pick_gemm_tile(M, N, 4) == 10 and hip.gemm_workgroups(M, N, K, 4) > 4
    corun(hip, gemm_load(f"policy9-{M}x{N}x{K}", M, N, K, 4, mode != "unmasked", gemm_policy=9), aggressor_for(aggressor, mode), mode)


@pytest.mark.parametrize("aggressor,mode", _ids(BASE_PAIRS))
def test_gather_corun(hip, aggressor, mode):
    corun(hip, gather_load(), aggressor_for(aggressor, mode), mode)


@pytest.mark.parametrize("aggressor,mode", _ids(BASE_PAIRS))
@pytest.mark.parametrize("regime,group,hkv", [("pair", 4, 2), ("uniform", 8, 1)])
def test_decode_attention_corun(hip, regime, group, hkv, aggressor, mode):
    corun(hip, attention_load(regime, group, hkv), aggressor_for(aggressor, mode), mode)


@pytest.mark.parametrize("aggressor,mode", _ids(BASE_PAIRS))
@pytest.mark.parametrize("variant", [3, 6, 10])
def test_triad_corun(hip, variant, aggressor, mode):
    """Three grid-stride trips and a ragged fourth of 3 blocks, inside guarded buffers."""
    corun(hip, triad_load(variant), aggressor_for(aggressor, mode), mode)


def test_graph_replay_corun(hip):
    """The bench's mode: the tile-14 policy-10 victim and the stream aggressor, each captured once
    (linearly, on its own stream) and replayed concurrently three times."""
    mode, K = "unmasked", 320
    victim, aggressor = gemm_load(f"graph-policy10-512x512x{K}", 512, 512, K, 4, False, gemm_policy=10), stream_aggressor()
    with knobs(hip, gemm_policy=10):
        assert hip.pick_gemm_tile(512, 512, 4) == 14
    with streams_for(hip, mode) as (sv, sa, sg):
        z = Sizing(hip, victim, aggressor, sv, sa, sg)
        ga, gv = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(ga, stream=sa):           # one pass; a 48 us pass outlasts the enqueueing of its replay
            aggressor.enqueue(hip, sa)
        with torch.cuda.graph(gv, stream=sv):           # the whole victim block
            victim.enqueue(hip, sv)

        def replay_aggressor(a0):
            a0.record(sa)
            with torch.cuda.stream(sa):
                for _ in range(z.n):
                    ga.replay()

        def replay_victim():
            with torch.cuda.stream(sv):
                gv.replay()

        def attempt():
            victim.reset()
            aggressor.reset()
            torch.cuda.synchronize()
            return enqueue_both(replay_aggressor, replay_victim, sv, sa)

        try:
            host, times = attempt()           # the rehearsal, as in corun
            z.resize(times, host)
            for k in range(3):
                _, times = attempt()
                assert_overlap(f"{victim.name} | stream | graph replay {k}", z, times)
                victim.check(("graph replay", k))
                aggressor.check(("graph replay aggressor", k))
        finally:
            torch.cuda.synchronize()
            del ga, gv


# ------------------------------------------------------------------------------------------------
# 2. the executor's co-run path against an independent reference
# ------------------------------------------------------------------------------------------------
def fill_outputs(bufs):
    from k8s_gpu_scheduler_amd.parallel.executor import op_output
    for o, t in bufs.ops:
        out = op_output(o, t)
        if out.dtype == torch.bfloat16:
            out.view(torch.int16).fill_(SENT16)
        else:
            out.fill_(NAN)


def check_pod_outputs(bufs, what):
    """Every op's output of one pod against a reference computed without the kernels; returns the
    largest GEMM error / bound ratio."""
    from k8s_gpu_scheduler_amd.parallel.executor import op_output
    worst = 0.0
    for i, (o, t) in enumerate(bufs.ops):
        out, tag = op_output(o, t), (what, i, o.kind)
        if o.kind == "gather":
            _, table, idx, offsets = t
            ref = table.double().index_select(0, idx.long()).view(o.M, o.K, o.N).sum(1)
            assert torch.equal(ref.float().double(), ref)                                  # exact in fp32, in any order
            assert torch.equal(out, ref.float().to(torch.bfloat16)), tag
        elif o.kind == "triad":
            want = torch.tensor(1.0) + torch.tensor(1.0001)                                 # one fp32 rounding, fused or not
            assert torch.equal(out, torch.full_like(out, want.item())), tag
        elif o.kind == "attn":
            _, q, kc, vc, table, ctx = t
            ref = ATT.reference(q, kc, vc, table, ctx)
            err, vmax = (out.double() - ref).abs().max().item(), float(vc.abs().max())
            print(f"executor co-run {tag}: attention max|out - ref| = {err:.5f} (bound {ATT.RANDOM_BOUND * vmax:.5f})")
            assert err <= ATT.RANDOM_BOUND * vmax, (tag, err)                               # NaN fails too
        else:
            a, bt, bias, c = t
            ref, bound = gemm_bound(a.float(), bt.float(), bias)
            err = (c.double() - ref).abs()
            assert bool((err <= bound).all()), (tag, int((~(err <= bound)).sum().item()), "elements outside the bound")
            ratio = (err / bound.clamp_min(1e-300)).max().item()
            print(f"executor co-run {tag}: largest GEMM error / bound = {ratio:.4f}")
            worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("use_graphs", [False, True], ids=["eager", "graphs"])
def test_executor_corun_against_independent_reference(monkeypatch, use_graphs):
    """Four pods on units (0,2) .. (6,2), masked and unmasked alternating, then two on (0,4) and
    (4,4) that wait on the device for the streams of the first four."""
    from k8s_gpu_scheduler_amd.models import workloads as W
    from k8s_gpu_scheduler_amd.parallel.executor import DeviceExecutor, PodRun
    for w in tiny_workloads():
        monkeypatch.setitem(W.EXTRA, w.name, w)
    names = ("t_mix", "t_idx")
    ex = DeviceExecutor(0)
    ex.use_graphs = use_graphs
    try:
        e1 = [PodRun(i, names[i % 2], 2 * i, 2, 24, masked=i % 2 == 0) for i in range(4)]
        e2 = [PodRun(4, names[1], 0, 4, 4, masked=True), PodRun(5, names[0], 4, 4, 4, masked=False)]
        ex.warm(e1 + e2)
        for r in e1 + e2:
            fill_outputs(ex.buffers(W.get(r.workload), r.first_unit, r.n_units))
        torch.cuda.synchronize()
        ex.launch_epoch(e1)
        ex.launch_epoch(e2)
        ex.wait_all()
        torch.cuda.synchronize()
        assert all(r.end.query() for r in e1 + e2)
        for r in e2:      # the device-side order: a pod starts after the previous occupants of its units ended
            for p in e1:
                if p.first_unit < r.first_unit + r.n_units and r.first_unit < p.first_unit + p.n_units:
                    assert ex.clock.elapsed_time(r.start) >= ex.clock.elapsed_time(p.end), (r.pod_id, p.pod_id)
        worst = max(check_pod_outputs(ex.buffers(W.get(r.workload), r.first_unit, r.n_units), (r.pod_id, r.workload, use_graphs))
                    for r in e1 + e2)
        print(f"executor co-run, graphs={use_graphs}: largest GEMM error / bound over all pods = {worst:.4f}")
    finally:
        ex.close()
