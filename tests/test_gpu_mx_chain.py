"""quantize_mx feeding gemm_mx on the GPU, both activation formats, at 64 x 128 x 256 and 128 x 192 x 384: the quantised
bytes are the CPU reference's, the product is within the true-regime bound of the reference chain (float64 product of
the dequantised reference operands; bound as in tests/test_gpu_gemm_mx_exact.py), and the chain replayed three times
from one captured graph gives identical bytes.  Then one pass of llm_mx_block_decode_256 through the executor, twice:
every op's output finite and equal between the passes."""
import functools

import pytest
import torch

from k8s_gpu_scheduler_amd.ops import loadgen

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SHAPES = [(64, 128, 256), (128, 192, 384)]


@functools.lru_cache(maxsize=None)
def chain_case(M, N, K, fmt):
    g = torch.Generator().manual_seed(M * 31 + N * 7 + K)
    x = torch.randn(M, K, generator=g).to(BF)
    w = (torch.randn(N, K, generator=g) * 0.05).to(BF)
    xq, xs = loadgen.quantize_mx_reference(x, fmt)
    wq, ws = loadgen.quantize_mx_reference(w, "fp4")
    a, b = loadgen.dequantize_mx_reference(xq, xs, fmt), loadgen.dequantize_mx_reference(wq, ws, "fp4")
    return x.cuda(), w.cuda(), (xq.view(torch.uint8), xs, wq, ws), a @ b.t(), a.abs() @ b.abs().t()


@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_quantise_then_multiply(M, N, K, fmt):
    x, w, (xq_r, xs_r, wq_r, ws_r), ref, mag = chain_case(M, N, K, fmt)
    wq, ws = loadgen.quantize_mx(w, "fp4")                               # the weights, once
    xq = torch.empty(M, loadgen.mx_row_bytes(fmt, K), dtype=loadgen.mx_element_dtype(fmt), device="cuda")
    xs = torch.empty(M, K // 32, dtype=torch.uint8, device="cuda")
    out = torch.empty(M, N, dtype=BF, device="cuda")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())

    def chain():
        loadgen.quantize_mx(x, fmt, out=xq, scales=xs, stream=st)
        loadgen.gemm_mx(xq, xs, wq, ws, fmt, out=out, stream=st)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        chain()
        st.synchronize()
        assert torch.equal(xq.view(torch.uint8).cpu(), xq_r) and torch.equal(xs.cpu(), xs_r)
        assert torch.equal(wq.cpu(), wq_r) and torch.equal(ws.cpu(), ws_r)
        got = out.double().cpu()
        bound = 2.0 ** -8 * ref.abs() + (1 + 2.0 ** -8) * K * 2.0 ** -23 * mag
        ratio = ((got - ref).abs() / bound).max().item()
        print(f"mx chain {fmt} {M}x{N}x{K}: max error / bound = {ratio:.4f}")
        assert ratio <= 1.0
        first = out.view(torch.int16).clone()
        with torch.cuda.graph(graph, stream=st):
            chain()
    for i in range(3):
        xq.view(torch.uint8).fill_(0x11)
        xs.fill_(0x11)
        out.view(torch.int16).fill_(0x1111)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), first), f"replay {i}"
        assert torch.equal(xq.view(torch.uint8).cpu(), xq_r) and torch.equal(xs.cpu(), xs_r), f"replay {i}"


def test_llm_mx_block_decode_through_the_executor_twice():
    from k8s_gpu_scheduler_amd.models import workloads as W
    from k8s_gpu_scheduler_amd.parallel.executor import _Buffers, enqueue_ops, op_output
    w = W.get("llm_mx_block_decode_256")
    bufs = _Buffers(w, torch.device("cuda", 0))
    passes = []
    for _ in range(2):
        for o, t in bufs.ops:
            out = op_output(o, t)
            out.view(torch.uint8 if out.element_size() == 1 else torch.int16).fill_(0x11)
        enqueue_ops(bufs, 1, torch.cuda.current_stream(), 0)
        torch.cuda.synchronize()
        passes.append([op_output(o, t).clone() for o, t in bufs.ops])
    kinds = [o.kind for o, _ in bufs.ops]
    assert kinds.count("quant_mx") == 4 and kinds.count("gemm_mx") == 4
    for (o, _), first, second in zip(bufs.ops, *passes):
        bits = torch.uint8 if first.element_size() == 1 else torch.int16
        assert torch.equal(first.view(bits), second.view(bits)), o
        if first.dtype == BF:
            assert torch.isfinite(first.float()).all(), o
        if o.kind == "quant_mx":                                         # randn: no non-finite block
            assert int((t_scales(bufs, o) == 255).sum()) == 0
    del bufs, passes
    torch.cuda.empty_cache()


def t_scales(bufs, op):
    return next(t[1] for o, t in bufs.ops if o is op)
