"""Bit-exact, guarded-buffer tests of the stream triad's workgroup shapes and its clamped grid (run with
`-m gpu` on an MI355X).

stream_triad launches min(blocks, ceil(n4 / (THREADS * U))) workgroups of THREADS threads, each moving
THREADS * U float4 per trip.  Variant 3 is the 256-thread 4x kernel, variants 5 and 7 the 1024-thread 2x and
3x kernels, so one workgroup tile is T = THREADS * U * 4 floats: 4096, 8192 and 12288.  The sizes are the
smallest at which the indexing by blockDim.x, the clamp and the tail predicates can go wrong:

  n = 4                  one float4: a single lane of a single workgroup works
  n = T - 4, T, T + 4    the last lane of a tile idle, a tile exactly, one float4 into a second tile (the
                         clamp gives 1, 1 and 2 workgroups under the default grid)
  n = 3T + 4, default    the clamp gives 4 workgroups, the last with one live lane
  n = 5T + 4, blocks 2   three trips per workgroup, the last trip of one of them predicated off but for a lane
  n = 5T + 4, blocks 1   six trips of one workgroup
  an output that starts 16 bytes into its allocation

Operands are integers in [-1024, 1024] and s = 0.5, so b + s * c is exact in fp32 whether or not the
multiply and the add are fused, and the comparison is bitwise.  The output is a window of a sentinel-filled
allocation with at least one workgroup tile of canaries on either side (4 floats in front in the last case,
which is what it is about); each input is the tail of its own allocation behind NaNs, so that it ends where
its allocation ends and a read in front of it would show in the result."""
import functools

import pytest
import torch

from test_gpu_kernels_exact import NAN, SENT32, guards_intact, knobs

pytestmark = pytest.mark.gpu

S = 0.5
TILE = {3: 256 * 4 * 4, 5: 1024 * 2 * 4, 7: 1024 * 3 * 4}          # floats per workgroup and trip
VARIANTS = sorted(TILE)


@pytest.fixture(scope="module")
def hip():
    from k8s_gpu_scheduler_amd import _native
    return _native.hip(required=True)


@pytest.fixture(autouse=True)
def default_knobs(hip):
    try:
        yield
    finally:
        hip.reset_knobs()


@functools.lru_cache(maxsize=None)
def operands(n):
    """(b, c, ref): b and c the last n floats of allocations that hold NaN in front of them."""
    g = torch.Generator(device="cuda").manual_seed(n)
    ins = []
    for _ in range(2):
        big = torch.full((64 + n,), NAN, device="cuda")
        big[64:] = torch.randint(-1024, 1025, (n,), device="cuda", generator=g).float()
        ins.append(big[64:])
    ref = ins[0] + S * ins[1]
    assert all(t.data_ptr() % 16 == 0 for t in ins) and not torch.isnan(ref).any()
    return ins[0], ins[1], ref


def run(hip, variant, n, blocks, front=None):
    from k8s_gpu_scheduler_amd.ops import loadgen
    tile = TILE[variant]
    front = tile if front is None else front
    b, c, ref = operands(n)
    raw = torch.full((front + n + tile,), SENT32, dtype=torch.int32, device="cuda")
    a = raw.view(torch.float32)[front:front + n]
    assert a.data_ptr() % 16 == 0 and a.data_ptr() - raw.data_ptr() == 4 * front
    with knobs(hip, triad_variant=variant):
        loadgen.triad(a, b, c, S, blocks=blocks)
    what = (variant, n, blocks, front)
    assert torch.equal(a, ref), (what, int((a != ref).sum().item()), "elements differ")
    assert guards_intact(raw, slice(front, front + n), SENT32), ("write outside a", what)


@pytest.mark.parametrize("variant", VARIANTS)
def test_one_float4(hip, variant):
    run(hip, variant, 4, 0)


@pytest.mark.parametrize("off", [-4, 0, 4])
@pytest.mark.parametrize("variant", VARIANTS)
def test_around_one_tile(hip, variant, off):
    run(hip, variant, TILE[variant] + off, 0)


@pytest.mark.parametrize("variant", VARIANTS)
def test_default_grid_clamped_to_four_tiles(hip, variant):
    run(hip, variant, 3 * TILE[variant] + 4, 0)


@pytest.mark.parametrize("blocks", [2, 1])
@pytest.mark.parametrize("variant", VARIANTS)
def test_several_trips_and_predicated_tail(hip, variant, blocks):
    run(hip, variant, 5 * TILE[variant] + 4, blocks)


@pytest.mark.parametrize("variant", VARIANTS)
def test_output_16_bytes_into_its_allocation(hip, variant):
    run(hip, variant, TILE[variant] + 4, 0, front=4)


@pytest.mark.parametrize("variant", VARIANTS)
def test_alignment_and_multiple_of_4_errors(hip, variant):
    """Raised by the native launcher before anything is launched, as before; the output keeps its sentinel."""
    n = 64
    raw = torch.full((n + 8,), SENT32, dtype=torch.int32, device="cuda")
    a = raw.view(torch.float32)
    b, c = torch.zeros(n + 8, device="cuda"), torch.zeros(n + 8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    with knobs(hip, triad_variant=variant):
        with pytest.raises(RuntimeError, match="multiple of 4"):
            hip.stream_triad(a.data_ptr(), b.data_ptr(), c.data_ptr(), S, n + 2, 0, st)
        for k, name in enumerate("abc"):
            ptrs = [t.data_ptr() + (4 if i == k else 0) for i, t in enumerate((a, b, c))]
            with pytest.raises(RuntimeError, match=name + " must be 16-byte aligned"):
                hip.stream_triad(*ptrs, S, n, 0, st)
    torch.cuda.synchronize()
    assert bool((raw == SENT32).all().item())
