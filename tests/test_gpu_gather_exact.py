"""Exact-arithmetic, guarded-buffer tests of the embedding-bag gather (run with `-m gpu` on an
MI355X), in the style of test_gpu_kernels_exact.py, whose guard helpers and sentinels are used.

Two value regimes make the fp32 bag sums exact, hence independent of the summation order; the
comparison with a float64 reference (index_select + a per-bag sum) is `torch.equal`:

  rep   table integers in [-4, 4], bags of at most 64 rows (129 in the long-bag case): |ref| <= 256
        (asserted on the reference alone), so bf16 holds every expected value exactly.
  rnd   table values k / 8 with |k| <= 64 (each one a bf16), bags of at most 64 (129) rows: sums are
        multiples of 1/8 below 512, exact in fp32; most outputs need the bf16 rounding and many
        are ties, which pins round-to-nearest-even (a tie is asserted on the reference alone).

Every launch runs in guarded buffers: the table is a view with ld = D + 8 at column offset 8 of an
allocation that is NaN everywhere else -- including the table rows no index names -- so a wrong
row or a read past D poisons the output; the output is a window with ld = D + 8 of a SENT16-filled
allocation whose guard cells are compared bitwise afterwards; idx and offsets start one element
into SENT32-filled int32 allocations (4-byte, not 8-byte aligned; SENT32 is no valid row).
"""
import functools
import json
import subprocess
import sys

import pytest
import torch

from test_gpu_kernels_exact import NAN, SENT16, SENT32, guarded_input, guarded_output, guards_intact, out_window

pytestmark = pytest.mark.gpu

REGIMES = ("rep", "rnd")
REP_CAP = 256
MAX_BAG = 64
C0 = 8                     # column offset of the table and output windows; ld = D + C0


@pytest.fixture(scope="module")
def hip():
    from k8s_gpu_scheduler_amd import _native
    return _native.hip(required=True)


# ------------------------------------------------------------------------------------------------
# operands and reference
# ------------------------------------------------------------------------------------------------
def table_values(R, D, regime, g):
    if regime == "rep":
        return torch.randint(-4, 5, (R, D), generator=g).float()
    return torch.randint(-64, 65, (R, D), generator=g).float() / 8


def reference(values, idx, offsets):
    """float64 [B, D]: index_select, then one sum per bag (an empty bag sums to zero)."""
    rows = values.double().index_select(0, idx.long())
    o = offsets.tolist()
    return torch.stack([rows[o[b]:o[b + 1]].sum(0) for b in range(len(o) - 1)])


def expected(ref, regime, need_tie=False):
    """rep: float32 (every value an integer of magnitude <= 256); rnd: the bf16 nearest-even
    rounding of the exact value."""
    if regime == "rep":
        cap = ref.abs().max().item() if ref.numel() else 0
        assert cap <= REP_CAP, f"representable regime: max|ref| = {cap} > {REP_CAP}"
        return ref.float()
    assert ref.abs().max().item() < 512 and torch.equal(ref * 8, (ref * 8).round())
    f = ref.float()
    assert torch.equal(f.double(), ref)
    if need_tie:      # exactly half-way between two bf16: the 16 dropped bits are 0x8000
        assert bool(((f.view(torch.int32) & 0xFFFF) == 0x8000).any()), "no tie in the reference"
    return f.to(torch.bfloat16)


def guarded_ints(t, after=3):
    """(raw, view): the int32 vector t as raw[1:1+n] of a SENT32-filled allocation."""
    raw = torch.full((1 + t.numel() + after,), SENT32, dtype=torch.int32, device="cuda")
    raw[1:1 + t.numel()] = t.cuda()
    view = raw[1:1 + t.numel()]
    assert view.data_ptr() % 8 == 4
    return raw, view


def guarded_table(values, idx):
    """The bf16 table window; the rows no index names are NaN like everything around it."""
    t = values.to(torch.bfloat16)
    assert torch.equal(t.float(), values)                           # the operands are exact
    view = guarded_input(t.cuda(), values.shape[1] + C0, c0=C0)
    unnamed = torch.ones(values.shape[0], dtype=torch.bool)
    unnamed[idx.long()] = False
    view[unnamed.cuda()] = NAN
    assert view.data_ptr() % 16 == 0 and view.stride(0) == values.shape[1] + C0
    return view


class Case:
    def __init__(self, values, idx, offsets, regime, need_tie=False, max_bag=MAX_BAG):
        assert int(offsets.diff().max()) <= max_bag
        self.B, self.D, self.R, self.regime = offsets.numel() - 1, values.shape[1], values.shape[0], regime
        self.exp = expected(reference(values, idx, offsets), regime, need_tie).cuda()
        self.table = guarded_table(values, idx)
        self.idx_raw, self.idx = guarded_ints(idx)
        self.off_raw, self.offsets = guarded_ints(offsets)
        self.raw, self.out = guarded_output(self.B, self.D, self.D + C0, C0, "cuda")
        assert self.out.data_ptr() % 16 == 0

    def resentinel(self):
        self.raw.fill_(SENT16)

    def check(self, what):
        torch.cuda.synchronize()
        out, exp = self.out, self.exp
        same = torch.equal(out.float(), exp) if self.regime == "rep" else torch.equal(out, exp)
        if not same:
            bad = (out.float() != exp.float()).nonzero()
            i, j = bad[0].tolist()
            raise AssertionError((what, f"{len(bad)} elements differ, first at [{i}, {j}]: "
                                        f"got {out[i, j].item()}, expected {exp[i, j].item()}"))
        assert guards_intact(self.raw, out_window(self.B, self.D, C0), SENT16), ("write outside the window", what)

    def untouched(self):
        torch.cuda.synchronize()
        return guards_intact(self.raw, (slice(0, 0), slice(0, 0)), SENT16)


# ------------------------------------------------------------------------------------------------
# 1. bag length boundaries
# ------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 64, 0]
R1 = 257


@functools.lru_cache(maxsize=None)
def boundary_case(D, regime):
    g = torch.Generator().manual_seed(D * 7 + (1 if regime == "rnd" else 0))
    offsets = torch.tensor([0] + LENGTHS, dtype=torch.int32).cumsum(0).to(torch.int32)
    idx = torch.randint(R1, (int(offsets[-1]),), generator=g, dtype=torch.int32)
    o = offsets.tolist()
    idx[o[1]] = 0                               # bag 1 = [0]
    idx[o[2]:o[3]] = R1 - 1                     # bag 2 = [R-1, R-1]: the last row, repeated in one bag
    idx[o[3]] = 0                               # bag 3 shares row 0 with bag 1
    idx[o[11] + 63] = R1 - 1                    # the last row of the longest bag
    return Case(table_values(R1, D, regime, g), idx, offsets, regime, need_tie=regime == "rnd")


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("D", [64, 128, 256, 512, 1024, 2048])
def test_bag_length_boundaries(hip, D, regime):
    """Remainders of the 4 steps in flight and (D <= 256) of the 8 / 4 / 2 rows per wave-instruction, empty
    bags (exactly +0.0, not the sentinel), rows 0 and R - 1, repeated and shared rows."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    c = boundary_case(D, regime)
    assert c.B == 13 and hip.embedding_bag_workgroups(c.B, 0) == 4
    c.resentinel()
    loadgen.embedding_bag(c.table, c.idx, c.offsets, out=c.out)
    c.check((D, regime))
    bits = c.out.view(torch.int16)
    assert not bits[0].any() and not bits[12].any()                 # +0.0: bit pattern 0


LONG_LENGTHS = [31, 32, 33, 65, 127, 128, 129]
LONG_MAX_BAG = 129
FRONT = 5                  # idx entries in front of offsets[0] in the offset-start case


@functools.lru_cache(maxsize=None)
def long_bag_case(D, regime):
    g = torch.Generator().manual_seed(D * 11 + (3 if regime == "rnd" else 2))
    offsets = torch.tensor([0] + LONG_LENGTHS, dtype=torch.int32).cumsum(0).to(torch.int32)
    idx = torch.randint(R1, (int(offsets[-1]),), generator=g, dtype=torch.int32)
    idx[-1] = R1 - 1                            # the last row closes the longest bag
    return Case(table_values(R1, D, regime, g), idx, offsets, regime, need_tie=regime == "rnd", max_bag=LONG_MAX_BAG)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("D", [64, 128, 256, 512, 1024, 2048])
def test_long_bags(hip, D, regime):
    """Bags of 31 .. 129 rows: more than two full trips of 4 steps at every D (at D = 64 a trip is
    32 rows, at D >= 512 four), each with a ragged tail of every kind around the trip lengths."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    c = long_bag_case(D, regime)
    assert c.B == 7 and max(LONG_LENGTHS) > 2 * 4 * max(1, 512 // D)
    c.resentinel()
    loadgen.embedding_bag(c.table, c.idx, c.offsets, out=c.out)
    c.check((D, regime, "long"))


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("D", [64, 256, 1024])
def test_offsets_start_past_zero(hip, D, regime):
    """offsets[0] = 5: the five idx entries in front of the first bag hold SENT32 (no valid row);
    neither the kernel nor the index check may read them as indices."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    c = boundary_case(D, regime)
    front = torch.full((FRONT,), SENT32, dtype=torch.int32)
    _, idx = guarded_ints(torch.cat([front, c.idx.cpu()]))
    _, offsets = guarded_ints(c.offsets.cpu() + FRONT)
    assert int(offsets[0]) == FRONT and int(offsets[-1]) == idx.numel() and int(idx[FRONT - 1]) == SENT32
    for check in (True, False):
        c.resentinel()
        loadgen.embedding_bag(c.table, idx, offsets, out=c.out, check_indices=check)
        c.check((D, regime, "offsets[0] = 5", check))
    bad = idx.clone()
    bad[FRONT] = SENT32                         # the first entry that is an index
    c.resentinel()
    with pytest.raises(ValueError):
        loadgen.embedding_bag(c.table, bad, offsets, out=c.out)
    assert c.untouched()


# ------------------------------------------------------------------------------------------------
# 2. workgroup tail and grid-stride trips (fixed pooling through the 2-D idx form)
# ------------------------------------------------------------------------------------------------
POOL = 5


@functools.lru_cache(maxsize=None)
def pooled_case(B, regime):
    g = torch.Generator().manual_seed(B * 13 + (1 if regime == "rnd" else 0))
    idx = torch.randint(R1, (B * POOL,), generator=g, dtype=torch.int32)
    offsets = (torch.arange(B + 1) * POOL).to(torch.int32)
    return Case(table_values(R1, 128, regime, g), idx, offsets, regime)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("B,blocks", [(1, 0), (3, 0), (4, 0), (5, 0), (9, 0), (37, 1), (37, 2), (37, 3)])
def test_workgroup_tail_and_grid_stride(hip, B, blocks, regime):
    from k8s_gpu_scheduler_amd.ops import loadgen
    c = pooled_case(B, regime)
    assert hip.embedding_bag_workgroups(B, blocks) == (blocks or -(-B // 4))
    c.resentinel()
    loadgen.embedding_bag(c.table, c.idx.view(B, POOL), out=c.out, blocks=blocks)
    c.check((B, blocks, regime))


# ------------------------------------------------------------------------------------------------
# 3. check_indices stops bad indices and offsets on the host
# ------------------------------------------------------------------------------------------------
def _bad_index(c, v):
    idx = c.idx.clone()
    idx[7] = v
    return idx, c.offsets


def _decreasing(c):
    off = c.offsets.clone()
    off[3], off[4] = c.offsets[4], c.offsets[3]
    return c.idx, off


def _past_end(c):
    off = c.offsets.clone()
    off[-1] = c.idx.numel() + 1
    return c.idx, off


@pytest.mark.parametrize("breakage", ["index-R", "index-minus-1", "offsets-decreasing", "offsets-past-L"])
def test_check_indices_raises_and_launches_nothing(breakage):
    from k8s_gpu_scheduler_amd.ops import loadgen
    c = boundary_case(128, "rep")
    idx, off = {"index-R": lambda: _bad_index(c, c.R), "index-minus-1": lambda: _bad_index(c, -1),
                "offsets-decreasing": lambda: _decreasing(c), "offsets-past-L": lambda: _past_end(c)}[breakage]()
    c.resentinel()
    with pytest.raises(ValueError):
        loadgen.embedding_bag(c.table, idx, off, out=c.out)
    assert c.untouched()


# ------------------------------------------------------------------------------------------------
# 4. row addresses beyond 4 GiB
# ------------------------------------------------------------------------------------------------
def test_rows_beyond_4_gib():
    """idx * ld_table * 2 passes 2^32 for the table's last rows: bags mix rows of both ends of a
    4 GiB + 64-row table that is initialised only there."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    D, edge = 128, 64
    free, _ = torch.cuda.mem_get_info()
    if free < 8 << 30:
        pytest.skip(f"needs 8 GiB of free device memory ({free >> 30} GiB free)")
    R = (1 << 32) // (2 * D) + edge
    g = torch.Generator().manual_seed(4)
    vals = table_values(2 * edge, D, "rep", g)                        # rows 0..63, then the last 64
    lengths = [8, 1, 64, 0, 5, 2, 33]
    offsets = torch.tensor([0] + lengths, dtype=torch.int32).cumsum(0).to(torch.int32)
    local = torch.randint(2 * edge, (int(offsets[-1]),), generator=g, dtype=torch.int32)
    local[:4] = torch.tensor([0, 2 * edge - 1, edge - 1, edge])       # both ends inside one bag
    idx = torch.where(local < edge, local, local + (R - 2 * edge))
    assert int(idx.max()) == R - 1 and int(idx.max()) * D * 2 >= 1 << 32
    exp = expected(reference(vals, local, offsets), "rep").cuda()
    table = torch.empty((R, D), dtype=torch.bfloat16, device="cuda")
    table[:edge] = vals[:edge].to(torch.bfloat16).cuda()
    table[R - edge:] = vals[edge:].to(torch.bfloat16).cuda()
    _, idx_v = guarded_ints(idx)
    _, off_v = guarded_ints(offsets)
    raw, out = guarded_output(len(lengths), D, D + C0, C0, "cuda")
    try:
        loadgen.embedding_bag(table, idx_v, off_v, out=out)
        torch.cuda.synchronize()
        assert torch.equal(out.float(), exp), int((out.float() != exp).sum().item())
        assert guards_intact(raw, out_window(len(lengths), D, C0), SENT16)
    finally:
        del table
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------
# 5. side stream and graph replay
# ------------------------------------------------------------------------------------------------
def test_side_stream_and_graph_replay():
    from k8s_gpu_scheduler_amd.ops import loadgen
    c = boundary_case(128, "rnd")
    s = torch.cuda.Stream()
    c.resentinel()
    torch.cuda.synchronize()
    loadgen.embedding_bag(c.table, c.idx, c.offsets, out=c.out, stream=s)
    s.synchronize()
    c.check("side stream")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        loadgen.embedding_bag(c.table, c.idx, c.offsets, out=c.out, stream=s, check_indices=False)
    for k in range(2):
        c.resentinel()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        s.synchronize()
        c.check(("replay", k))


# ------------------------------------------------------------------------------------------------
# 6. the grid rule
# ------------------------------------------------------------------------------------------------
def test_workgroups_match_the_python_rule(hip):
    from k8s_gpu_scheduler_amd.models import workloads as W
    for B in (1, 4, 5, 53248):
        assert hip.embedding_bag_workgroups(B, 0) == W.default_gather_workgroups(B)


# ------------------------------------------------------------------------------------------------
# 7. pod path
# ------------------------------------------------------------------------------------------------
def test_podrun_dlrm():
    p = subprocess.run([sys.executable, "-m", "k8s_gpu_scheduler_amd.ops.podrun", "--workload", "dlrm_2048",
                        "--iters", "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    assert res["workload"] == "dlrm_2048" and res["iters"] == 2 and res["throughput"] > 0


def _bf16_ordinal(t):
    """bf16 -> an integer that steps by one from each bf16 to the next (-0 and +0 coincide)."""
    bits = t.view(torch.int16).int()
    return torch.where(bits < 0, -(bits & 0x7FFF), bits)


def test_executor_dlrm_buffers_and_gather_output():
    """The executor's operands are reproducible, and one iteration's gather output is the per-bag
    sum torch computes in fp32, within 1 bf16 ulp (plumbing; the arithmetic is pinned above)."""
    from k8s_gpu_scheduler_amd.models import workloads as W
    from k8s_gpu_scheduler_amd.parallel.executor import _Buffers, enqueue_ops
    dev = torch.device("cuda", 0)
    w = W.get("dlrm_2048")
    a, b = _Buffers(w, dev), _Buffers(w, dev)
    (o, (out, table, idx, offsets)), (_, (_, table_b, idx_b, offsets_b)) = a.ops[0], b.ops[0]
    assert o.kind == "gather" and table.shape == (o.rows, o.N) and idx.numel() == o.M * o.K
    assert torch.equal(idx, idx_b) and torch.equal(offsets, offsets_b)
    assert torch.equal(table.view(torch.int16), table_b.view(torch.int16))
    assert int(idx.min()) >= 0 and int(idx.max()) < o.rows and int(idx.max()) >= o.rows // 2
    del b, table_b, idx_b, offsets_b
    out.view(torch.int16).fill_(SENT16)
    enqueue_ops(a, 1, torch.cuda.current_stream(), 0)
    torch.cuda.synchronize()
    ref = table.index_select(0, idx.long()).float().view(o.M, o.K, o.N).sum(1).to(torch.bfloat16)
    d = (_bf16_ordinal(out) - _bf16_ordinal(ref)).abs().max().item()
    assert d <= 1, f"gather output differs from the fp32 torch sum by {d} bf16 ulp"
    del a
    torch.cuda.empty_cache()
