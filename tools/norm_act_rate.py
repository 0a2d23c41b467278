"""Achieved bytes/s of the residual add + RMSNorm and of SwiGLU on the MI355X, with the stream triad as the yardstick.

Shapes: the four ops of the llm_block_decode_256 and llm_block_prefill_2048 workloads (add_rmsnorm 256 x 4096
and 2048 x 4096, swiglu 256 x 14336 and 2048 x 14336), add_rmsnorm at 8192 x 8192 (0.5 GiB moved) and swiglu at
8192 x 14336 (0.66 GiB) -- these two exceed the 256 MiB Infinity Cache and are the ones that can be read as a
bandwidth -- and, as the floor of a launch, each kernel at its smallest shape (1 x 8).  In the same process the
stream triad over 3 x 96 MiB.

profiles/r11_rope_append found that two events around ONE small launch cost about 21 us whatever the kernel
does.  So every figure here is the time of a CHAIN of back-to-back launches on one stream between two events,
divided by the chain's length (--chain, default 50; 10 for the shapes past the Infinity Cache and the triad): a
warm-up chain first, then the median of --chains (default 20) chains.  The chain is captured once into a HIP
graph and replayed, so the host enqueues nothing per launch; for the two floor shapes the same chain is also
enqueued eagerly from Python (`eager_median_us`): that figure is the host's cost of one call of the wrapper,
which an eager chain of small launches cannot go below.  The launches of a chain run on the same operands: a
shape that fits in the Infinity Cache is served from it.  Bytes are Op.bytes of models.workloads.  A shape is
marked latency-dominated when its time per launch is under three times its kernel's floor.  No pass/fail
threshold.

    python tools/norm_act_rate.py [--chains 20] [--chain 50] [--out profiles/r12_norm_act/rates.json]
                                  [--kernel-resources "add_rmsnorm:vgprs=..,lds=..;swiglu:vgprs=.."]

--kernel-resources is recorded as given: each kernel's registers and occupancy as the compiler's resource-usage
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

# (kind, name, rows, row length, past the Infinity Cache)
SHAPES = (("add_rmsnorm", "floor", 1, 8, False), ("add_rmsnorm", "llm_block_decode_256", 256, 4096, False),
          ("add_rmsnorm", "llm_block_prefill_2048", 2048, 4096, False), ("add_rmsnorm", "large", 8192, 8192, True),
          ("swiglu", "floor", 1, 8, False), ("swiglu", "llm_block_decode_256", 256, 14336, False),
          ("swiglu", "llm_block_prefill_2048", 2048, 14336, False), ("swiglu", "large", 8192, 14336, True))
TRIAD_FLOATS = 24 << 20
BIG_CHAIN = 10
MARK0, MARK1 = "<!-- table -->", "<!-- /table -->"


def chain_us(fn, chain, chains, eager=False):
    """Per-launch device times (us) of `chains` chains of `chain` back-to-back launches on one stream, after one
    untimed chain.  The chain is captured once into a HIP graph and replayed between the two events: the host
    then enqueues nothing per launch.  eager=True enqueues every launch from Python instead -- the figure is
    then the larger of the device's time and the host's cost of a call of the wrapper."""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    g = None
    if not eager:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(chain):
                fn()
    out = []
    with torch.cuda.stream(s):
        for k in range(chains + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if g is not None:
                g.replay()
            else:
                for _ in range(chain):
                    fn()
            e1.record()
            torch.cuda.synchronize()
            if k:                        # the first chain is the warm-up
                out.append(e0.elapsed_time(e1) * 1e3 / chain)
    return out


def summary(us, nbytes, chain):
    med = statistics.median(us)
    return {"median_us": round(med, 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2), "chains": len(us),
            "chain": chain, "bytes": nbytes, "gbps": round(nbytes / (med * 1e-6) / 1e9, 1)}


def table(res):
    rows = ["| kernel | shape | rows x row length | workgroups | per launch | bytes | bytes/s | of the triad's | latency-dominated |",
            "|---|---|---|---|---|---|---|---|---|"]
    for r in res["ops"]:
        rows.append(f"| `{r['kind']}` | `{r['shape']}` | {r['rows']:,} x {r['cols']:,} | {r['workgroups']:,} | {r['median_us']} us "
                    f"| {r['bytes'] / 1e6:.1f} MB | {r['gbps'] / 1e3:.2f} TB/s | {r['vs_triad']:.3f} | "
                    f"{'yes' if r['latency_dominated'] else 'no'} |")
    t = res["triad"]
    rows.append(f"| stream triad | 3 x 96 MiB | | 8,192 | {t['median_us']} us | {t['bytes'] / 1e6:.0f} MB | {t['gbps'] / 1e3:.2f} TB/s | 1 | |")
    return "\n".join(rows)


def write_readme(path, res):
    body = f"{MARK0}\n{table(res)}\n{MARK1}"
    text = open(path).read() if os.path.exists(path) else ""
    if MARK0 in text and MARK1 in text:
        text = text[:text.index(MARK0)] + body + text[text.index(MARK1) + len(MARK1):]
    else:
        text = ("# r12: residual add + RMSNorm and SwiGLU\n\n`rates.json` is the output of\n\n    " + res["command"]
                + "\n\non one MI355X (tools/norm_act_rate.py tells the method: chains of back-to-back launches between two\n"
                "events, each chain a replayed graph, time per launch, the median of the chains; bytes are `Op.bytes` of `models/workloads.py`).\n\n"
                + body + "\n")
    with open(path, "w") as f:
        f.write(text)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--chains", type=int, default=20)
    ap.add_argument("--chain", type=int, default=50)
    ap.add_argument("--out", default="profiles/r12_norm_act/rates.json")
    ap.add_argument("--kernel-resources", default="", help="kernel:name=value,...;kernel:... from the compiler's remarks")
    a = ap.parse_args(argv)
    if a.chains < 10 or a.chain < BIG_CHAIN:
        ap.error(f"--chains must be at least 10 and --chain at least {BIG_CHAIN}")
    if not torch.cuda.is_available():
        raise SystemExit("norm_act_rate needs a GPU")
    h = _native.hip(required=True)
    g = torch.Generator(device="cuda").manual_seed(12)
    # the command as it bears on the measurement: where the result is written is left out
    res = {"command": f"{os.path.basename(sys.executable)} {sys.argv[0]} --chains {a.chains} --chain {a.chain}",
           "device": torch.cuda.get_device_name(0), "ops": []}
    if a.kernel_resources:
        res["kernel_resources"] = {k: {n: int(v) for n, v in (nv.split("=") for nv in rest.split(","))}
                                   for k, rest in (kr.split(":") for kr in a.kernel_resources.split(";"))}

    x, y, z = (torch.ones(TRIAD_FLOATS, dtype=torch.float32, device="cuda") for _ in range(3))
    triad = summary(chain_us(lambda: loadgen.triad(x, y, z, 1.0001), BIG_CHAIN, a.chains),
                    W.Op("triad", n_floats=TRIAD_FLOATS).bytes, BIG_CHAIN)
    res["triad"] = triad
    print("triad", triad, flush=True)
    del x, y, z

    floor = {}
    for kind, name, T, n, big in SHAPES:
        op = W.Op(kind, T, n)
        chain = BIG_CHAIN if big else a.chain
        if kind == "add_rmsnorm":
            xs = torch.randn(T, n, device="cuda", generator=g).to(torch.bfloat16)
            rs = torch.randn(T, n, device="cuda", generator=g).to(torch.bfloat16)
            wt = (1 + 0.1 * torch.randn(n, device="cuda", generator=g)).to(torch.bfloat16)
            yo, ro = torch.empty_like(xs), torch.empty_like(xs)
            fn = lambda: loadgen.add_rmsnorm(xs, wt, rs, out=yo, residual_out=ro)          # noqa: E731
            wgs = h.add_rmsnorm_workgroups(T)
        else:
            gu = torch.randn(T, 2 * n, device="cuda", generator=g).to(torch.bfloat16)
            out = torch.empty(T, n, dtype=torch.bfloat16, device="cuda")
            fn = lambda: loadgen.swiglu(gu, out=out)                                        # noqa: E731
            wgs = h.swiglu_workgroups(T, n)
        r = dict(summary(chain_us(fn, chain, a.chains), op.bytes, chain), kind=kind, shape=name, rows=T, cols=n,
                 flops=op.flops, workgroups=wgs)
        if name == "floor":
            floor[kind] = r["median_us"]
            r["eager_median_us"] = round(statistics.median(chain_us(fn, chain, a.chains, eager=True)), 2)
        r["vs_triad"] = round(r["gbps"] / triad["gbps"], 4)
        r["latency_dominated"] = r["median_us"] < 3 * floor[kind]
        res["ops"].append(r)
        print(kind, r, flush=True)
        torch.cuda.synchronize()
        if kind == "add_rmsnorm":
            del xs, rs, wt, yo, ro
        else:
            del gu, out
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
