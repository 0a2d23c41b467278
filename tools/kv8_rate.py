"""Time per launch of the FP8 paged-KV kernels on the MI355X beside their bf16 siblings -- decode attention, split-KV
decode attention and rope_append over float8_e4m3fn caches (native/hip/decode_attn_kv8.hip, rope_append.hip)
against the same shapes over bf16 caches -- and the stream triad over a working set of 1 GiB, all in one process.

Shapes: the llm_decode_256 attention (256 sequences x 1,024 tokens, 32 query heads over 8 KV heads), the same at 4,096
tokens, 8 sequences x 32,768 tokens unsplit and with 4 and 8 splits, 32 sequences x 1,024 tokens (a bf16 cache of
128 MiB, inside the 256 MiB Infinity Cache), and the two append shapes of profiles/r11_rope_append (256 decode tokens;
two 1,024-token chunks).  The operands are the executor's (its seeded cache patterns, a shuffled block table).

The method is that of tools/mx_rate.py: every figure is the time of a CHAIN of back-to-back launches on one stream
between two events, divided by the chain's length, the chain captured once into a graph and replayed, a warm-up chain
first.  bf16 and FP8 ALTERNATE: --rounds rounds (default 3) of --chains chains each, bf16 then FP8, and the median
over all of a kind's chains.  `bytes` is Op.bytes of models/workloads.py.  No pass/fail threshold.

    python tools/kv8_rate.py [--chains 5] [--rounds 3] [--chain 20] [--out profiles/r17_kv8/rates.json]
                             [--kernel-resources "paged_decode_kv8_kernel:vgprs=..,lds=..,scratch=..;..."]

--kernel-resources is recorded as given: registers, LDS and scratch as the compiler's resource-usage remarks state them
(hipcc -Rpass-analysis=kernel-resource-usage).  README.md beside the output gets the table between its
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
# (label, the bf16 Op); the FP8 Op is the same with kind + "_kv8"
SHAPES = (
    ("llm_decode_256", W.Op("attn", 256, 32, 1024, rows=8)),
    ("256 x 4,096", W.Op("attn", 256, 32, 4096, rows=8)),
    ("8 x 32,768 unsplit", W.Op("attn", 8, 32, 32768, rows=8)),
    ("8 x 32,768, 4 splits", W.Op("attn_split", 8, 32, 32768, rows=8, splits=4)),
    ("8 x 32,768, 8 splits", W.Op("attn_split", 8, 32, 32768, rows=8, splits=8)),
    ("32 x 1,024 (Infinity Cache)", W.Op("attn", 32, 32, 1024, rows=8)),
    ("append, 256 decode tokens", W.Op("rope_append", 256, 32, 1024, rows=8, q=1)),
    ("append, two 1,024-token chunks", W.Op("rope_append", 2, 32, 4096, rows=8, q=1024)),
)
NOT_MEASURED = ("co-run groups with the FP8 kernels", "v_cvt_pk_fp8_f32 in the writer", "16-byte V loads (a token map that gives "
                "a lane 16 consecutive tokens)", "FP8 q / P on the fp8 MFMAs", "chunked-prefill attention over the FP8 cache")


def kv8(o):
    return W.Op(o.kind + "_kv8", o.M, o.N, o.K, rows=o.rows, q=o.q, splits=o.splits)


def launcher(o, dev):
    """The executor's operands and launch of the op, as a closure on the current stream."""
    make, launch, _ = executor.OP_KINDS[o.kind]
    t = make(o, torch.Generator().manual_seed(17), dev)
    return lambda: launch(o, t, None, 0, 0)


def table(res):
    rows = ["| shape | workgroups | bf16 | FP8 | FP8 / bf16 time | bf16 bytes/s (of the triad's) | FP8 bytes/s (of the triad's) |",
            "|---|---|---|---|---|---|---|"]
    for r in res["shapes"]:
        b, f = r["bf16"], r["fp8"]
        rows.append(f"| {r['label']} | {r['workgroups']:,} | {b['median_us']} us, {b['bytes'] / 1e6:.1f} MB | {f['median_us']} us, "
                    f"{f['bytes'] / 1e6:.1f} MB | {r['time_ratio']:.3f} | {b['gbps'] / 1e3:.2f} TB/s ({b['vs_triad']:.2f}) | "
                    f"{f['gbps'] / 1e3:.2f} TB/s ({f['vs_triad']:.2f}) |")
    t = res["triad"]
    rows.append(f"| stream triad, 3 x 352 MiB | | {t['median_us']} us, {t['bytes'] / 1e6:.0f} MB | | | {t['gbps'] / 1e3:.2f} TB/s (1) | |")
    return "\n".join(rows)


def write_readme(path, res):
    body = f"{MARK0}\n{table(res)}\n{MARK1}"
    text = open(path).read() if os.path.exists(path) else ""
    if MARK0 in text and MARK1 in text:
        text = text[:text.index(MARK0)] + body + text[text.index(MARK1) + len(MARK1):]
    else:
        text = ("# r17: FP8 paged-KV cache -- append writer and decode attention\n\n`rates.json` is the output of\n\n    " + res["command"]
                + "\n\non one MI355X (tools/kv8_rate.py tells the method: chains of back-to-back launches between two events,\n"
                "each chain a replayed graph, bf16 and FP8 alternating, time per launch, the median of the chains; the\n"
                "executor's operands; bytes are `Op.bytes` of `models/workloads.py`).\n\n" + body
                + "\n\nNot measured: " + "; ".join(res["not_measured"]) + ".\n")
    with open(path, "w") as f:
        f.write(text)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--chains", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chain", type=int, default=20)
    ap.add_argument("--out", default="profiles/r17_kv8/rates.json")
    ap.add_argument("--kernel-resources", default="", help="kernel:name=value,...;kernel:... from the compiler's remarks")
    a = ap.parse_args(argv)
    if a.chains < 3 or a.rounds < 1 or a.chain < BIG_CHAIN:
        ap.error(f"--chains must be at least 3, --rounds at least 1 and --chain at least {BIG_CHAIN}")
    if not torch.cuda.is_available():
        raise SystemExit("kv8_rate needs a GPU")
    _native.hip(required=True)
    dev = torch.device("cuda", 0)
    res = {"command": f"{os.path.basename(sys.executable)} {sys.argv[0]} --chains {a.chains} --rounds {a.rounds} --chain {a.chain}",
           "device": torch.cuda.get_device_name(0), "shapes": [], "not_measured": list(NOT_MEASURED)}
    if a.kernel_resources:
        res["kernel_resources"] = {k: {n: int(v) for n, v in (nv.split("=") for nv in rest.split(","))}
                                   for k, rest in (kr.split(":") for kr in a.kernel_resources.split(";"))}

    x, y, z = (torch.ones(TRIAD_FLOATS, dtype=torch.float32, device=dev) for _ in range(3))
    triad = summary(chain_us(lambda: loadgen.triad(x, y, z, 1.0001), BIG_CHAIN, a.chains * a.rounds),
                    W.Op("triad", n_floats=TRIAD_FLOATS).bytes, BIG_CHAIN)
    res["triad"] = triad
    print("triad", triad, flush=True)
    del x, y, z
    torch.cuda.empty_cache()

    for label, o in SHAPES:
        o8 = kv8(o)
        chain = BIG_CHAIN if o.bytes > 5e8 else a.chain                   # launches past ~100 us: the shorter chain
        fb, f8 = launcher(o, dev), launcher(o8, dev)
        us = {"bf16": [], "fp8": []}
        for _ in range(a.rounds):                                         # alternating
            us["bf16"] += chain_us(fb, chain, a.chains)
            us["fp8"] += chain_us(f8, chain, a.chains)
        row = {"label": label, "kind": o.kind, "S": o.M, "Hq": o.N, "ctx": o.K, "Hkv": o.rows, "q": o.q, "splits": o.splits,
               "workgroups": o.workgroups(0), "bf16": summary(us["bf16"], o.bytes, chain), "fp8": summary(us["fp8"], o8.bytes, chain)}
        for k in ("bf16", "fp8"):
            row[k]["vs_triad"] = round(row[k]["gbps"] / triad["gbps"], 4)
        row["time_ratio"] = round(row["fp8"]["median_us"] / row["bf16"]["median_us"], 4)
        res["shapes"].append(row)
        print(label, row, flush=True)
        del fb, f8
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
