"""The MoE MLP end to end -- loadgen.moe_mlp = moe_route -> moe_gemm (gathered) -> swiglu -> moe_gemm (in place) ->
moe_combine (run with `-m gpu` on an MI355X).

The check is STAGE-WISE: each stage's GPU output is compared with that stage's reference applied to the GPU's actual
output of the stage before, so no error of one stage is charged to the next and every bound is the stage's own:

  route    ids and the four layout arrays bitwise (loadgen.moe_topk_reference, moe_align_reference); the weights
           within the bound of test_gpu_moe_route_exact.py;
  gemm     the valid rows within the true-regime bound of test_gpu_moe_gemm_exact.py -- 2^-8 |ref| + (1 + 2^-8) K 2^-23
           sum |a_i w_i| against the float64 product of the rows the GPU read --, the pad rows of used tiles 0x0000;
  swiglu   |act - ref| <= (2^-8 + 2^-16) |ref| on every row, the bound of test_gpu_swiglu_exact.py (|g| <= 8 asserted);
  combine  bitwise against the fp32 fma emulation of test_gpu_moe_combine_exact.py.

Cases: T = 70, D = 128, F = 64, k = 2 over FOUR live experts, and T = 256, E = 128, k = 8 with D = 128, F = 64.  The
router's interface wants E a multiple of 8 in [8, 256], so the four-expert case gives the router 8 logit columns of
which the last four are -Inf: with k = 2 <= 4 they are never selected, 140 slots fall on 4 experts (35 each on
average, every tile more than half full), and experts 4 .. 7 own no tile.  The second case is the decode workload's
routing shape: 2,048 slots over 128 experts, 158 tiles of which about 128 are used.

moe_mlp is then bitwise equal to the five separate calls, also replayed twice from a captured graph; the pod path
(podrun --workload llm_moe_decode_256 in a fresh child process) exits 0; and the executor's gathered moe_gemm output
on 8 picked rows is within the true-regime bound of the float64 reference.
"""
import json
import subprocess
import sys

import pytest
import torch

from test_gpu_moe_combine_exact import chain
from test_gpu_moe_route_exact import weight_bound
from test_gpu_swiglu_exact import TRUE_BOUND as SWIGLU_BOUND, reference as swiglu_reference
from test_moe_cpu import check_layout

pytestmark = pytest.mark.gpu

# MEASURED on an MI355X (printed by the tests):
MEASURED = """
  error / bound per stage: four_experts (4 of 10 tiles used): route weights 0.2743, up 0.9607, down 0.9872;
  decode_routing (128 of 158 tiles used): route weights 0.2000, up 0.9786, down 0.9879; the combine and every
  moe_mlp / graph-replay comparison bit-exact.  The executor's moe_gemm, 8 picked rows: 0.5761.
  The module: 4 tests in 5 s, 3 s of them the podrun process.
"""

BF, I32 = torch.bfloat16, torch.int32
INF = float("inf")
CASES = {"four_experts": (70, 8, 2, 128, 64, 4), "decode_routing": (256, 128, 8, 128, 64, 128)}    # T, E, k, D, F, live


@pytest.fixture(scope="module")
def L():
    from k8s_gpu_scheduler_amd import _native
    from k8s_gpu_scheduler_amd.ops import loadgen
    _native.hip(required=True)
    return loadgen


def operands(name):
    T, E, k, D, F, live = CASES[name]
    g = torch.Generator().manual_seed(len(name))
    x = torch.randn(T, D, generator=g).to(BF)
    lg = torch.randn(T, E, generator=g)
    lg[:, live:] = -INF
    w13 = (torch.randn(E, 2 * F, D, generator=g) / 16).to(BF)
    w2 = (torch.randn(E, D, F, generator=g) / 8).to(BF)
    return x, lg.to(BF), w13, w2


def gemm_stage(a, w, s, t, n_slots, gather_div, got, what):
    """One moe_gemm stage on the CPU: got (the GPU's output) against the float64 product of the rows of `a` (the
    GPU's input) it names.  Returns max error / bound."""
    E, N, K = w.shape
    valid = s < n_slots
    e_row = t.long().repeat_interleave(64)
    src = (s // gather_div if gather_div else torch.arange(len(s), dtype=I32)).long()
    worst = 0.0
    for e in range(E):
        rows = (valid & (e_row == e)).nonzero().flatten()
        if not len(rows):
            continue
        ar, we = a[src[rows]].double(), w[e].double()
        ref, mag = ar @ we.T, ar.abs() @ we.abs().T
        bound = 2.0 ** -8 * ref.abs() + (1 + 2.0 ** -8) * K * 2.0 ** -23 * mag
        worst = max(worst, ((got[rows].double() - ref).abs() / bound).max().item())
    assert worst <= 1.0, (what, worst)
    pads = (e_row >= 0) & ~valid
    assert bool((got[pads].view(torch.int16) == 0).all()), what
    return worst


def five_calls(L, x, lg, w13, w2, k):
    n, F = x.shape[0] * k, w2.shape[2]
    ids, tw, s, t, off, p = L.moe_route(lg, k)
    h13 = torch.zeros(len(s), 2 * F, dtype=BF, device="cuda")
    L.moe_gemm(x, w13, s, t, n, gather_div=k, out=h13)
    act = L.swiglu(h13)
    y = torch.zeros(len(s), x.shape[1], dtype=BF, device="cuda")
    L.moe_gemm(act, w2, s, t, n, gather_div=0, out=y)
    out = L.moe_combine(y, p, tw)
    torch.cuda.synchronize()
    return ids, tw, s, t, off, p, h13, act, y, out


@pytest.mark.parametrize("name", list(CASES))
def test_stage_wise_and_moe_mlp_bitwise(L, name):
    T, E, k, D, F, live = CASES[name]
    host = operands(name)
    x, lg, w13, w2 = (v.cuda() for v in host)
    ids, tw, s, t, off, p, h13, act, y, out = (v.cpu() for v in five_calls(L, x, lg, w13, w2, k))
    n = T * k
    # route
    ref_ids, _ = L.moe_topk_reference(host[1], k)
    assert torch.equal(ids, ref_ids) and int(ids.max()) < live
    for a, b in zip((s, t, off, p), L.moe_align_reference(ids, E)):
        assert torch.equal(a, b)
    check_layout(ids, E, s, t, off, p)
    l_sel = host[1].double().gather(1, ids.long())
    e = torch.exp2((l_sel - l_sel[:, :1]) * 1.4426950408889634)
    ref_w = e / e.sum(dim=1, keepdim=True)
    r_route = ((tw.double() - ref_w).abs() / (weight_bound(l_sel, k) * ref_w)).max().item()
    assert r_route <= 1.0
    # gemm, gathered: from x
    r_up = gemm_stage(host[0], host[2], s, t, n, k, h13, "up")
    # swiglu: from the GPU's h13, every row
    assert float(h13[:, :F].float().abs().max()) <= 8
    ref_act = swiglu_reference(h13)
    assert bool(((act.double() - ref_act).abs() <= SWIGLU_BOUND * ref_act.abs()).all())
    # gemm, in place: from the GPU's act
    r_down = gemm_stage(act, host[3], s, t, n, 0, y, "down")
    # combine: from the GPU's y and weights, bitwise
    assert torch.equal(out.view(torch.int16), chain(y, p, tw, fp32=True).view(torch.int16))
    print(f"moe chain {name}: error / bound: route weights {r_route:.4f}, up {r_up:.4f}, down {r_down:.4f}; "
          f"{int((t >= 0).sum())} of {len(t)} tiles used")
    # moe_mlp: the same bits, eagerly and replayed from a graph
    eager = L.moe_mlp(x, lg, w13, w2, k)
    torch.cuda.synchronize()
    assert torch.equal(eager.cpu().view(torch.int16), out.view(torch.int16))
    ws = L.moe_workspace(T, E, k, D, F, x.device)
    out_g = torch.empty(T, D, dtype=BF, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        L.moe_mlp(x, lg, w13, w2, k, workspace=ws, out=out_g, stream=st)
    for r in range(2):
        if r == 0:
            out_g.fill_(float("nan"))                                                  # the second replay writes over the first
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            g.replay()
        st.synchronize()
        assert torch.equal(out_g.cpu().view(torch.int16), out.view(torch.int16)), r


def test_podrun_llm_moe_decode():
    p = subprocess.run([sys.executable, "-m", "k8s_gpu_scheduler_amd.ops.podrun", "--workload", "llm_moe_decode_256",
                        "--iters", "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    assert res["workload"] == "llm_moe_decode_256" and res["iters"] == 2 and res["throughput"] > 0


def test_the_executors_moe_gemm_on_8_picked_rows(L):
    """One iteration of llm_moe_decode_256's gathered moe_gemm (its own op alone: 0.8 GiB of operands, not the
    workload's 1.3) through _Buffers + enqueue_ops; 8 valid rows spread over the layout against float64."""
    from k8s_gpu_scheduler_amd.models import workloads as W
    from k8s_gpu_scheduler_amd.parallel.executor import _Buffers, enqueue_ops
    w = W.get("llm_moe_decode_256")
    o = w.ops[3]
    assert o.kind == "moe_gemm" and o.gather
    bufs = _Buffers(W.Workload("llm_moe_decode_256", w.family, w.framework, w.batch, (o,), 0.0), torch.device("cuda", 0))
    out, a, wt, s, t = bufs.ops[0][1]
    enqueue_ops(bufs, 1, torch.cuda.current_stream(), 0)
    torch.cuda.synchronize()
    s_h, t_h = s.cpu(), t.cpu()
    n = o.M * o.q
    rows = (s_h < n).nonzero().flatten()
    picked = rows[torch.linspace(0, len(rows) - 1, 8).long()]
    worst = 0.0
    for i in picked.tolist():
        e, src = int(t_h[i // 64]), int(s_h[i]) // o.q
        ar, we = a[src].double().cpu(), wt[e].double().cpu()
        ref, mag = we @ ar, we.abs() @ ar.abs()
        bound = 2.0 ** -8 * ref.abs() + (1 + 2.0 ** -8) * o.K * 2.0 ** -23 * mag
        worst = max(worst, ((out[i].double().cpu() - ref).abs() / bound).max().item())
    print(f"executor moe_gemm, 8 picked rows: max error / bound = {worst:.4f}")
    assert worst <= 1.0
    del bufs
    torch.cuda.empty_cache()
