"""Time per launch of the mixture-of-experts kernels on the MI355X at the shapes of llm_moe_decode_256 and
llm_moe_prefill_2048 (128 experts, top-8, hidden 2048, expert width 768), with the stream triad, a torch loop over
the experts and the dense GEMM as the yardsticks -- all in one process.

Per workload: `moe_route`, the gathered `moe_gemm` to 2 x 768, the in-place `moe_gemm` to 2048 and `moe_combine`, on the
operands the executor builds (parallel.executor.OP_KINDS: randn logits routed on the CPU, weights that repeat a
pattern of four experts at 128 distinct addresses).  The expert GEMMs' yardstick at decode sizes is the stream triad
over a working set of 1 GiB: `weights_vs_triad` is (bytes of the weights of the experts that own a tile) / time as a
fraction of the triad's bytes/s.  Beside each expert GEMM the same product as a torch loop over the experts that own
rows -- torch.index_select of the expert's rows, then torch.matmul with its weight matrix, per expert, the index
vectors made beforehand -- and, for the prefill shape, loadgen.gemm on a DENSE problem of equal useful flops
(16,384 rows times one weight matrix).

The method is that of tools/sample_rate.py: every figure is the time of a CHAIN of back-to-back launches on one
stream between two events, divided by the chain's length (--chain, default 20; 10 for the triad and the torch
loops), the chain captured once into a graph and replayed, a warm-up chain first, then the median of --chains
chains.  Every shape's operands are far larger than the Infinity Cache (0.4 to 0.8 GB of weights), so a chain on the
same operands streams them again from HBM.  No pass/fail threshold.

    python tools/moe_rate.py [--chains 10] [--chain 20] [--out profiles/r15_moe/rates.json]
                             [--kernel-resources "moe_gemm_128:vgprs=..,lds=..;..."]

--kernel-resources is recorded as given: registers, LDS and scratch as the compiler's resource-usage remarks state
them (hipcc -Rpass-analysis=kernel-resource-usage).  README.md beside the output gets the table between its
`<!-- table -->` markers; the rest of an existing README.md is kept.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from k8s_gpu_scheduler_amd import _native  # noqa: E402
from k8s_gpu_scheduler_amd.models import workloads as W  # noqa: E402
from k8s_gpu_scheduler_amd.ops import loadgen  # noqa: E402
from k8s_gpu_scheduler_amd.parallel import executor  # noqa: E402
from tools.norm_act_rate import BIG_CHAIN, MARK0, MARK1, chain_us, summary  # noqa: E402

TRIAD_FLOATS = 88 << 20                  # per array: 3 x 352 MiB, a working set of 1 GiB
NOT_MEASURED = ("skewed routing (a few hot experts: many tiles of one expert, many unused tiles)",
                "co-run groups with the MoE kernels", "other block tiles, stage counts and workgroup orders of moe_gemm",
                "a multi-workgroup align step", "top-k other than 8 and expert counts other than 128")


def table(res):
    rows = ["| workload | op | shape | workgroups (used) | per launch | TFLOP/s | expert weights | weights / time | of the triad's | torch loop | dense gemm |",
            "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["ops"]:
        wt = f"{r['weight_bytes'] / 1e6:.0f} MB | {r['weight_gbps'] / 1e3:.2f} TB/s | {r['weights_vs_triad']:.3f}" if "weight_bytes" in r else " | | "
        loop = f"{r['torch_loop_us']} us ({r['torch_loop_method']}; x{r['torch_over_moe']:.1f})" if "torch_loop_us" in r else ""
        dense = f"{r['dense_us']} us (x{r['dense_over_moe']:.2f})" if "dense_us" in r else ""
        used = f" ({r['used_workgroups']:,})" if "used_workgroups" in r else ""
        rows.append(f"| `{r['workload']}` | `{r['kind']}` | {r['shape']} | {r['workgroups']:,}{used} | {r['median_us']} us | "
                    f"{r['flops'] / r['median_us'] / 1e6:.1f} | {wt} | {loop} | {dense} |")
    t = res["triad"]
    rows.append(f"| | stream triad | 3 x 352 MiB | | {t['median_us']} us | | {t['bytes'] / 1e6:.0f} MB | {t['gbps'] / 1e3:.2f} TB/s | 1 | | |")
    return "\n".join(rows)


def write_readme(path, res):
    body = f"{MARK0}\n{table(res)}\n{MARK1}"
    text = open(path).read() if os.path.exists(path) else ""
    if MARK0 in text and MARK1 in text:
        text = text[:text.index(MARK0)] + body + text[text.index(MARK1) + len(MARK1):]
    else:
        text = ("# r15: mixture-of-experts route, grouped GEMM and combine\n\n`rates.json` is the output of\n\n    " + res["command"]
                + "\n\non one MI355X (tools/moe_rate.py tells the method: chains of back-to-back launches between two events,\n"
                "each chain a replayed graph, time per launch, the median of the chains).  `weights / time` is the bytes of the\n"
                "weights of the experts that own a tile over the launch time; the torch loop is `index_select` + `matmul` per\n"
                "expert, the dense gemm `loadgen.gemm` on as many rows as there are slots.\n\n" + body
                + "\n\nNot measured: " + "; ".join(res["not_measured"]) + ".\n")
    with open(path, "w") as f:
        f.write(text)


def timed(fn, chain, chains):
    """(per-launch times, method): a replayed graph, or the eager chain where torch cannot capture fn."""
    try:
        return chain_us(fn, chain, chains), "replayed graph"
    except RuntimeError as e:
        print("not captured:", str(e).splitlines()[0], flush=True)
        torch.cuda.synchronize()
        return chain_us(fn, chain, chains, eager=True), "eager chain"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--chains", type=int, default=10)
    ap.add_argument("--chain", type=int, default=20)
    ap.add_argument("--out", default="profiles/r15_moe/rates.json")
    ap.add_argument("--kernel-resources", default="", help="kernel:name=value,...;kernel:... from the compiler's remarks")
    a = ap.parse_args(argv)
    if a.chains < 5 or a.chain < BIG_CHAIN:
        ap.error(f"--chains must be at least 5 and --chain at least {BIG_CHAIN}")
    if not torch.cuda.is_available():
        raise SystemExit("moe_rate needs a GPU")
    h = _native.hip(required=True)
    dev = torch.device("cuda", 0)
    res = {"command": f"{os.path.basename(sys.executable)} {sys.argv[0]} --chains {a.chains} --chain {a.chain}",
           "device": torch.cuda.get_device_name(0), "ops": [], "not_measured": list(NOT_MEASURED)}
    if a.kernel_resources:
        res["kernel_resources"] = {k: {n: int(v) for n, v in (nv.split("=") for nv in rest.split(","))}
                                   for k, rest in (kr.split(":") for kr in a.kernel_resources.split(";"))}

    x, y, z = (torch.ones(TRIAD_FLOATS, dtype=torch.float32, device=dev) for _ in range(3))
    triad = summary(chain_us(lambda: loadgen.triad(x, y, z, 1.0001), BIG_CHAIN, a.chains),
                    W.Op("triad", n_floats=TRIAD_FLOATS).bytes, BIG_CHAIN)
    res["triad"] = triad
    print("triad", triad, flush=True)
    del x, y, z
    torch.cuda.empty_cache()

    for w in W.LLM_MOE.values():
        for o in w.ops:
            if o.kind not in ("moe_route", "moe_gemm", "moe_combine"):
                continue
            make, launch, _ = executor.OP_KINDS[o.kind]
            t = make(o, torch.Generator().manual_seed(15), dev)
            r = dict(summary(chain_us(lambda: launch(o, t, None, 0, 0), a.chain, a.chains), o.bytes, a.chain),
                     workload=w.name, kind=o.kind + (" (gathered)" if o.gather else ""), flops=o.flops,
                     workgroups=o.workgroups(0), shape=f"T {o.M}, N {o.N}, K {o.K}")
            if o.kind == "moe_gemm":
                out, amat, wt, s, te = t
                n = o.M * o.q
                tiles_used = int((te >= 0).sum())
                experts = te[te >= 0].unique()
                r["used_workgroups"] = tiles_used * (o.workgroups(0) // len(te))
                r["weight_bytes"] = 2 * len(experts) * o.N * o.K
                r["weight_gbps"] = round(r["weight_bytes"] / (r["median_us"] * 1e-6) / 1e9, 1)
                r["weights_vs_triad"] = round(r["weight_gbps"] / triad["gbps"], 4)
                # the torch loop: per expert, index_select of its rows and a matmul with its matrix
                valid = s < n
                e_row = te.long().repeat_interleave(64)
                src = (s // o.q if o.gather else torch.arange(len(s), dtype=torch.int32, device=dev)).long()
                idx = [src[valid & (e_row == e)] for e in experts.tolist()]

                def loop():
                    return [torch.matmul(torch.index_select(amat, 0, i), wt[e].T) for e, i in zip(experts.tolist(), idx)]
                us, method = timed(loop, BIG_CHAIN, a.chains)
                lp = summary(us, o.bytes, BIG_CHAIN)
                r.update(torch_loop_us=lp["median_us"], torch_loop_method=method,
                         torch_over_moe=round(lp["median_us"] / r["median_us"], 2))
                if o.M == 2048:                            # the dense problem of equal useful flops
                    da = torch.randn(n, o.K, device=dev).to(torch.bfloat16)
                    dc = torch.empty(n, o.N, dtype=torch.bfloat16, device=dev)
                    d = summary(chain_us(lambda: loadgen.gemm(da, wt[0], out=dc), a.chain, a.chains),
                                W.Op("gemm", n, o.N, o.K).bytes, a.chain)
                    r.update(dense_us=d["median_us"], dense_over_moe=round(d["median_us"] / r["median_us"], 3),
                             dense_workgroups=h.gemm_workgroups(n, o.N, o.K, 0, False, False))
                    del da, dc
                del out, amat, wt, s, te, idx
            res["ops"].append(r)
            print(o.kind, r, flush=True)
            torch.cuda.synchronize()
            del t
            torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    write_readme(os.path.join(os.path.dirname(os.path.abspath(a.out)), "README.md"), res)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
