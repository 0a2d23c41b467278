"""quantize_mx on the GPU, bit for bit against the rule's CPU reference (ops.loadgen.quantize_mx_reference, itself
pinned in tests/test_mx_cpu.py): elements and scale bytes, both formats -- all 65,536 bf16 patterns, crafted blocks
(amax at and just below every power of two, ties, saturation, signed zeros, underflow beside a huge amax, non-finite
blocks), row and block counts that are no multiple of the lane groups, guarded windows with odd row strides (the
byte-store path) and aligned ones (the 8-byte / 4-byte store path), and graph replays."""
import functools

import pytest
import torch

from k8s_gpu_scheduler_amd.ops import loadgen

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
FORMATS = ("fp8", "fp4")
SENT8 = 0x5A


def all_patterns() -> torch.Tensor:
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF).view(64, 1024)


def crafted() -> torch.Tensor:
    """[R, 64] bf16: two blocks per row.  Powers of two and the pattern just below each as the amax, the tie values of
    both formats under several block scales, saturating values, signed zeros, an underflow beside a huge amax, Inf and
    NaN blocks beside finite ones."""
    rows = []
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 1.0625, 1.1875, 17.0, 19.0, 2.0 ** -10, 3 * 2.0 ** -10, 6.5, 7.0, 7.5,
            464.0, 480.0, 496.0, 400.0, -0.0, 0.0, -0.25, -(2.0 ** -10), 2.0 ** -6 - 2.0 ** -11, 2.0 ** -20]
    for e in range(-126, 128):
        r = torch.zeros(64, dtype=torch.float64)
        r[3] = 2.0 ** e
        r[4] = -(2.0 ** e) * 0.75
        r[32 + 7] = 2.0 ** e
        rb = r.to(BF)
        rb.view(torch.int16)[32 + 7] -= 1                               # just below 2^e
        rows.append(rb)
    for shift in (-100, -40, -1, 0, 3, 60, 110):
        for amax in (4.0, 256.0):
            r = torch.zeros(64, dtype=torch.float64)
            r[:len(ties)] = torch.tensor(ties, dtype=torch.float64)
            r[31] = amax
            r[32:32 + len(ties)] = -torch.tensor(ties, dtype=torch.float64)
            r[63] = -amax
            rows.append((r * 2.0 ** shift).to(BF))
    special = torch.zeros(6, 64, dtype=torch.float64)
    special[0, :5] = torch.tensor([2.0 ** 120, 1.0, -1.0, 2.0 ** -126, -(2.0 ** -133)])
    special[0, 40] = 2.0 ** -130                                        # a subnormal amax
    special[1, 2], special[1, 35] = float("inf"), 1.0
    special[2, 2], special[2, 63] = 1.0, float("-inf")
    special[3, 0], special[3, 32] = float("nan"), float("nan")
    special[4] = -0.0
    special[5, 1::2] = 2.0 ** -133
    rows += list(special.to(BF))
    return torch.stack(rows)


@functools.lru_cache(maxsize=None)
def case(name: str, fmt: str):
    """(x on the GPU, reference q bytes, reference scales), built once."""
    if name == "patterns":
        x = all_patterns()
    elif name == "crafted":
        x = crafted()
    else:
        T, D = (int(v) for v in name.split("x"))
        g = torch.Generator().manual_seed(T * 100003 + D)
        x = (torch.randn(T, D, generator=g) * torch.exp2(torch.randint(-12, 12, (T, D // 32), generator=g)
                                                          .repeat_interleave(32, dim=1).float())).to(BF)
    q, s = loadgen.quantize_mx_reference(x, fmt)
    return x.cuda(), q.view(torch.uint8), s


def check(q, s, qr, sr, what):
    q, s = q.view(torch.uint8).cpu(), s.cpu()
    bad_s = (s != sr).nonzero()
    assert len(bad_s) == 0, f"{what}: {len(bad_s)} scale bytes differ, first at {bad_s[0].tolist()}: " \
                            f"{int(s[tuple(bad_s[0])])} vs {int(sr[tuple(bad_s[0])])}"
    bad = (q != qr).nonzero()
    assert len(bad) == 0, f"{what}: {len(bad)} element bytes differ, first at {bad[0].tolist()}: " \
                          f"{int(q[tuple(bad[0])]):#x} vs {int(qr[tuple(bad[0])]):#x}"


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", ["patterns", "crafted"])
def test_patterns_and_crafted_blocks_exact(name, fmt):
    x, qr, sr = case(name, fmt)
    q, s = loadgen.quantize_mx(x, fmt)
    assert q.dtype == loadgen.mx_element_dtype(fmt) and s.dtype == torch.uint8
    check(q, s, qr, sr, f"{name} {fmt}")
    if name == "patterns":
        assert int((s == 255).sum()) == 8 and int((s == 0).sum()) == {"fp4": 24, "fp8": 72}[fmt]


SHAPES = [f"{T}x{D}" for T in (1, 5, 67) for D in (32, 96, 160, 4096)]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", SHAPES)
def test_shapes_exact(name, fmt):
    x, qr, sr = case(name, fmt)
    q, s = loadgen.quantize_mx(x, fmt)
    check(q, s, qr, sr, f"{name} {fmt}")


# (q row padding, q column offset, scale row padding, scale column offset): odd strides and offsets take the byte
# stores, multiples of 8 the one-store-per-lane path
WINDOWS = [pytest.param(4, 3, 2, 1, id="odd-strides"), pytest.param(16, 8, 1, 0, id="aligned-q")]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("qpad,qc0,spad,sc0", WINDOWS)
@pytest.mark.parametrize("name", ["crafted", "5x96", "67x160"])
def test_guarded_windows(name, fmt, qpad, qc0, spad, sc0):
    x, qr, sr = case(name, fmt)
    T, D = x.shape
    # x: a window of a NaN-filled allocation (16-byte aligned rows: column offset and stride multiples of 8)
    big = torch.full((T + 5, D + 24), float("nan"), dtype=BF, device="cuda")
    big[2:2 + T, 8:8 + D] = x
    xw = big[2:2 + T, 8:8 + D]
    qcols, scols = qr.shape[1], sr.shape[1]
    odd = qpad % 8 != 0
    qld, sld = qcols + qpad + qc0, scols + spad + sc0
    if odd:                                                             # literally odd row strides
        qld, sld = qld | 1, sld | 1
    qraw = torch.full((T + 4, qld), SENT8, dtype=torch.uint8, device="cuda")
    sraw = torch.full((T + 4, sld), SENT8, dtype=torch.uint8, device="cuda")
    qw = qraw[1:1 + T, qc0:qc0 + qcols].view(loadgen.mx_element_dtype(fmt))
    sw = sraw[1:1 + T, sc0:sc0 + scols]
    if odd and T > 1:
        assert qw.stride(0) % 2 == 1 and sw.stride(0) % 2 == 1
    q, s = loadgen.quantize_mx(xw, fmt, out=qw, scales=sw)
    assert q is qw and s is sw
    torch.cuda.synchronize()
    want_q = torch.full_like(qraw, SENT8).cpu()
    want_q[1:1 + T, qc0:qc0 + qcols] = qr
    want_s = torch.full_like(sraw, SENT8).cpu()
    want_s[1:1 + T, sc0:sc0 + scols] = sr
    assert torch.equal(qraw.cpu(), want_q), f"{name} {fmt}: q window or its guard cells differ"
    assert torch.equal(sraw.cpu(), want_s), f"{name} {fmt}: scale window or its guard cells differ"
    assert torch.isnan(big[:2]).all() and torch.isnan(big[:, :8]).all()


@pytest.mark.parametrize("fmt", FORMATS)
def test_graph_replays_give_the_same_bytes(fmt):
    x, qr, sr = case("67x4096", fmt)
    q = torch.zeros(qr.shape, dtype=torch.uint8, device="cuda").view(loadgen.mx_element_dtype(fmt))
    s = torch.zeros(sr.shape, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        loadgen.quantize_mx(x, fmt, out=q, scales=s, stream=st)          # warm-up outside the capture
        st.synchronize()
        with torch.cuda.graph(graph, stream=st):
            loadgen.quantize_mx(x, fmt, out=q, scales=s, stream=st)
    for i in range(3):
        q.view(torch.uint8).fill_(0xEE)
        s.fill_(0xEE)
        graph.replay()
        torch.cuda.synchronize()
        check(q, s, qr, sr, f"replay {i} {fmt}")


def test_empty_launches_nothing():
    x = torch.zeros(0, 64, dtype=BF, device="cuda")
    q, s = loadgen.quantize_mx(x, "fp4")
    assert tuple(q.shape) == (0, 32) and tuple(s.shape) == (0, 2)
