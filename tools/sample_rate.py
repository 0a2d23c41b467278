"""Time per launch and achieved bytes/s of the top-k / top-p token sampler on the MI355X, with the stream triad and
a torch pipeline as the yardsticks.

Shapes at Llama-3's vocabulary of 128,256 and the executor's parameters (temperature 0.8, top_k 50, top_p 0.9,
logits bf16(1.5 * randn)): 8 rows (llm_head_decode_8: 8 workgroups on 256 CUs), 256 rows (llm_head_decode_256:
one workgroup per CU, 64 MB, served from the Infinity Cache) and 4,096 rows (1 GiB: past the 256 MiB Infinity
Cache, the one that can be read as a bandwidth); 256 greedy rows (top_k 1); and the selection's fallback on 256
"staircase" rows whose top 64 values lie 3 binades apart from one another, so that the window walk crosses the
whole middle of the key space.  As the floor of a launch the kernel at its smallest shape, greedy (1 x 8, top_k 1:
one histogram window); beside it the same 8 logits sampled (k = 8 = V: the candidates lie on both sides of zero,
so the walk crosses half the key space -- a shape no vocabulary has).  In the same process the stream triad over
a working set of 1 GiB (3 x 352 MiB), and on the same logits the pipeline torch.topk(logits, 50) -> softmax of the
50 values / temperature -> cumsum, the reference a sampler written with torch ops would start from (it does not
even cut or pick).

As in tools/norm_act_rate.py every figure is the time of a CHAIN of back-to-back launches on one stream between
two events, divided by the chain's length (--chain, default 50; 10 for the 1 GiB shapes, the triad and the torch
pipeline): a warm-up chain first, then the median of --chains (default 20) chains.  The chain is captured once
into a HIP graph and replayed, so the host enqueues nothing per launch.  The launches of a chain run on the
same operands: a shape that fits in the Infinity Cache is served from it.  Bytes are Op.bytes of
models.workloads.  No pass/fail threshold.

    python tools/sample_rate.py [--chains 20] [--chain 50] [--out profiles/r14_sample/rates.json]
                                [--kernel-resources "sample_topk:vgprs=..,lds=.."]

--kernel-resources is recorded as given: the kernel's registers and occupancy as the compiler's resource-usage
remarks state them (hipcc -Rpass-analysis=kernel-resource-usage).  README.md beside the output gets the table
between its `<!-- table -->` markers; the rest of an existing README.md is kept.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from k8s_gpu_scheduler_amd import _native  # noqa: E402
from k8s_gpu_scheduler_amd.models import workloads as W  # noqa: E402
from k8s_gpu_scheduler_amd.ops import loadgen  # noqa: E402
from tools.norm_act_rate import BIG_CHAIN, MARK0, MARK1, chain_us, summary  # noqa: E402

V = 128256
TOP_K, TEMPERATURE, TOP_P = 50, 0.8, 0.9
# (name, rows, vocabulary, top_k, what the rows hold, past the Infinity Cache)
SHAPES = (("floor", 1, 8, 1, "randn", False), ("smallest_sampled", 1, 8, TOP_K, "randn", False),
          ("llm_head_decode_8", 8, V, TOP_K, "randn", False),
          ("llm_head_decode_256", 256, V, TOP_K, "randn", False), ("large", 4096, V, TOP_K, "randn", True),
          ("greedy_256", 256, V, 1, "randn", False), ("staircase_256", 256, V, 64, "staircase", False))
TORCH_ROWS = (8, 256, 4096)
TRIAD_FLOATS = 88 << 20                  # per array: 3 x 352 MiB, a working set of 1 GiB
NOT_MEASURED = ("other workgroup sizes and chunk counts per thread", "a split-row launch for few rows",
                "window sequences other than 16 / 64 / 128 / 256 codes and, before it, 16 / 64 / 256", "co-run groups with the sampler",
                "logits that are not normally distributed (a trained model's)")


def staircase(rows, g):
    """Rows whose 64 largest values are 2^6, 2^3 .. 2^-87 and -2^-87 .. -2^6 at random places over a crowd near
    -1000: every one of them in a histogram window of its own."""
    steps = torch.tensor([2.0 ** (6 - 3 * i) for i in range(32)] + [-(2.0 ** (-87 + 3 * i)) for i in range(32)], device="cuda")
    x = (-1000 - 50 * torch.rand(rows, V, device="cuda", generator=g)).to(torch.bfloat16)
    where = torch.rand(rows, V, device="cuda", generator=g).argsort(-1)[:, :64]
    x.scatter_(1, where, steps.to(torch.bfloat16)[None, :].expand(rows, -1))
    return x


def table(res):
    rows = ["| what | rows x vocabulary | workgroups | per launch | bytes | bytes/s | of the triad's | of the torch pipeline's time |",
            "|---|---|---|---|---|---|---|---|"]
    for r in res["ops"]:
        vs = f"1 / {r['torch_over_sample']:.1f}" if "torch_over_sample" in r else ""
        rows.append(f"| `sample` `{r['shape']}` | {r['rows']:,} x {r['cols']:,} | {r['workgroups']:,} | {r['median_us']} us "
                    f"| {r['bytes'] / 1e6:.2f} MB | {r['gbps'] / 1e3:.3f} TB/s | {r['vs_triad']:.3f} | {vs} |")
    for r in res["torch"]:
        rows.append(f"| torch topk + softmax + cumsum ({r['method']}) | {r['rows']:,} x {V:,} | | {r['median_us']} us | "
                    f"{r['bytes'] / 1e6:.2f} MB | {r['gbps'] / 1e3:.3f} TB/s | | 1 |")
    t = res["triad"]
    rows.append(f"| stream triad | 3 x 352 MiB | | {t['median_us']} us | {t['bytes'] / 1e6:.0f} MB | {t['gbps'] / 1e3:.2f} TB/s | 1 | |")
    return "\n".join(rows)


def write_readme(path, res):
    body = f"{MARK0}\n{table(res)}\n{MARK1}"
    text = open(path).read() if os.path.exists(path) else ""
    if MARK0 in text and MARK1 in text:
        text = text[:text.index(MARK0)] + body + text[text.index(MARK1) + len(MARK1):]
    else:
        text = ("# r14: top-k / top-p token sampling\n\n`rates.json` is the output of\n\n    " + res["command"]
                + "\n\non one MI355X (tools/sample_rate.py tells the method: chains of back-to-back launches between two\n"
                "events, each chain a replayed graph, time per launch, the median of the chains; bytes are `Op.bytes` of\n"
                "`models/workloads.py`).\n\n" + body + "\n\nNot measured: " + "; ".join(res["not_measured"]) + ".\n")
    with open(path, "w") as f:
        f.write(text)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--chains", type=int, default=20)
    ap.add_argument("--chain", type=int, default=50)
    ap.add_argument("--out", default="profiles/r14_sample/rates.json")
    ap.add_argument("--kernel-resources", default="", help="kernel:name=value,... from the compiler's remarks")
    a = ap.parse_args(argv)
    if a.chains < 10 or a.chain < BIG_CHAIN:
        ap.error(f"--chains must be at least 10 and --chain at least {BIG_CHAIN}")
    if not torch.cuda.is_available():
        raise SystemExit("sample_rate needs a GPU")
    h = _native.hip(required=True)
    g = torch.Generator(device="cuda").manual_seed(14)
    res = {"command": f"{os.path.basename(sys.executable)} {sys.argv[0]} --chains {a.chains} --chain {a.chain}",
           "device": torch.cuda.get_device_name(0), "parameters": {"temperature": TEMPERATURE, "top_k": TOP_K, "top_p": TOP_P},
           "ops": [], "torch": [], "not_measured": list(NOT_MEASURED)}
    if a.kernel_resources:
        res["kernel_resources"] = {k: {n: int(v) for n, v in (nv.split("=") for nv in rest.split(","))}
                                   for k, rest in (kr.split(":") for kr in a.kernel_resources.split(";"))}

    x, y, z = (torch.ones(TRIAD_FLOATS, dtype=torch.float32, device="cuda") for _ in range(3))
    triad = summary(chain_us(lambda: loadgen.triad(x, y, z, 1.0001), BIG_CHAIN, a.chains),
                    W.Op("triad", n_floats=TRIAD_FLOATS).bytes, BIG_CHAIN)
    res["triad"] = triad
    print("triad", triad, flush=True)
    del x, y, z
    torch.cuda.empty_cache()

    torch_us = {}
    for name, S, v, k, fill, big in SHAPES:
        op = W.Op("sample", S, v, k)
        chain = BIG_CHAIN if big else a.chain
        if fill == "staircase":
            logits = staircase(S, g)
        else:
            logits = (1.5 * torch.randn(S, v, device="cuda", generator=g)).to(torch.bfloat16)
        u = torch.rand(S, device="cuda", generator=g)
        t = torch.full((S,), TEMPERATURE, device="cuda")
        tk = torch.full((S,), k, dtype=torch.int32, device="cuda")
        tp = torch.full((S,), TOP_P, device="cuda")
        out = torch.empty(S, dtype=torch.int32, device="cuda")
        loadgen.sample_tokens(logits, u, t, tk, tp, out=out)                            # once with the device-side check
        fn = lambda: loadgen.sample_tokens(logits, u, t, tk, tp, out=out, check=False)  # noqa: E731
        r = dict(summary(chain_us(fn, chain, a.chains), op.bytes, chain), shape=name, rows=S, cols=v, top_k=k, fill=fill,
                 flops=op.flops, workgroups=h.sample_workgroups(S))
        r["vs_triad"] = round(r["gbps"] / triad["gbps"], 4)
        if name == "floor":
            r["eager_median_us"] = round(statistics.median(chain_us(fn, chain, a.chains, eager=True)), 2)
        if fill == "randn" and v == V and k == TOP_K and S in TORCH_ROWS:
            def pipeline():
                vals, idx = torch.topk(logits, TOP_K, dim=-1)
                return torch.softmax(vals.float() / TEMPERATURE, dim=-1).cumsum(-1), idx
            try:
                us, method = chain_us(pipeline, BIG_CHAIN, a.chains), "replayed graph"
            except RuntimeError as e:                       # a torch op that cannot be captured: the eager chain, said so
                print("torch pipeline not captured:", str(e).splitlines()[0], flush=True)
                torch.cuda.synchronize()
                us, method = chain_us(pipeline, BIG_CHAIN, a.chains, eager=True), "eager chain"
            tr = dict(summary(us, op.bytes, BIG_CHAIN), rows=S, method=method)
            res["torch"].append(tr)
            torch_us[S] = tr["median_us"]
            r["torch_over_sample"] = round(tr["median_us"] / r["median_us"], 2)
            print("torch", tr, flush=True)
        res["ops"].append(r)
        print("sample", r, flush=True)
        torch.cuda.synchronize()
        del logits, u, t, tk, tp, out
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
