"""Time per launch of the chunked-prefill attention over an FP8 paged-KV cache (native/hip/prefill_attn_kv8.hip)
beside the bf16 kernel (prefill_attn.hip) on the same shapes, in one process, on the MI355X.

Shapes: the attention of llm_kv8_layer_prefill_2048 (2 x 1,024-token chunks on 4,096 tokens: the caches in the
Infinity Cache, the compute-bound case), that of llm_kv8_chunk_prefill_64 (64 x 32-token chunks on 8,192 tokens: a
bf16 cache of 2 GiB streamed from HBM), the decode shape through the prefill kernels (256 x 1-token chunks on 1,024
tokens; reported beside attn_kv8's time from profiles/r17_kv8/rates.json where that file is there) and a long context
(8 x 512-token chunks on 32,768 tokens).  32 query heads over 8 KV heads; the operands are the executor's.

The method is tools/kv8_rate.py's, whose helpers are imported: every figure is the time of a CHAIN of back-to-back
launches on one stream between two events, divided by the chain's length, the chain captured once into a graph and
replayed, a warm-up chain first.  bf16 and FP8 ALTERNATE: --rounds rounds (default 3) of --chains chains each, bf16
then FP8, and the median over all of a kind's chains.  flops and bytes are Op.flops / Op.bytes of models/workloads.py.
No pass/fail threshold.

    python tools/prefill_kv8_rate.py [--chains 5] [--rounds 3] [--chain 20] [--out profiles/r18_prefill_kv8/rates.json]
                                     [--kernel-resources "paged_prefill_kv8_kernel:vgprs=..,lds=..,scratch=..;..."]
                                     [--decode-profile a-copy-of-profiles/r17_kv8/rates.json]

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
from tools.kv8_rate import BIG_CHAIN, MARK0, MARK1, chain_us, kv8, launcher, summary  # noqa: E402

# (label, the bf16 Op); the FP8 Op is the same with kind + "_kv8"
SHAPES = (
    ("2 x 1,024 on 4,096 (llm_kv8_layer_prefill_2048)", W.Op("prefill", 2, 32, 4096, rows=8, q=1024)),
    ("64 x 32 on 8,192 (llm_kv8_chunk_prefill_64)", W.Op("prefill", 64, 32, 8192, rows=8, q=32)),
    ("256 x 1 on 1,024 (the decode shape)", W.Op("prefill", 256, 32, 1024, rows=8, q=1)),
    ("8 x 512 on 32,768", W.Op("prefill", 8, 32, 32768, rows=8, q=512)),
)
DECODE_PROFILE, DECODE_LABEL = os.path.join("profiles", "r17_kv8", "rates.json"), "llm_decode_256"
NOT_MEASURED = ("co-run groups with the FP8 prefill", "the two-instruction conversion (v_cvt_pk_f32_fp8 + v_cvt_pk_bf16_f32) in this "
                "kernel", "FP8 q / P on the fp8 MFMAs", "a split-KV prefill")


def decode_reference(path):
    """attn_kv8's and attn's medians for the decode shape from the r17 profile, or None."""
    try:
        with open(path) as f:
            row = next(r for r in json.load(f)["shapes"] if r["label"] == DECODE_LABEL)
        return {"source": DECODE_PROFILE, "attn_us": row["bf16"]["median_us"], "attn_kv8_us": row["fp8"]["median_us"]}
    except (OSError, KeyError, StopIteration, ValueError):
        return None


def table(res):
    rows = ["| shape | workgroups | bf16 | FP8 | FP8 / bf16 time | bf16 flops/s | FP8 flops/s | bf16 bytes/s | FP8 bytes/s |",
            "|---|---|---|---|---|---|---|---|---|"]
    for r in res["shapes"]:
        b, f = r["bf16"], r["fp8"]
        rows.append(f"| {r['label']} | {r['workgroups']:,} | {b['median_us']} us, {b['bytes'] / 1e6:.1f} MB | {f['median_us']} us, "
                    f"{f['bytes'] / 1e6:.1f} MB | {r['time_ratio']:.3f} | {b['tflops']:.0f} TFLOP/s | {f['tflops']:.0f} TFLOP/s | "
                    f"{b['gbps'] / 1e3:.2f} TB/s | {f['gbps'] / 1e3:.2f} TB/s |")
    d = res.get("decode_reference")
    if d:
        rows.append(f"| the decode kernels on the decode shape ({d['source']}) | 2,048 | {d['attn_us']} us | {d['attn_kv8_us']} us | "
                    f"{d['attn_kv8_us'] / d['attn_us']:.3f} | | | | |")
    return "\n".join(rows)


def write_readme(path, res):
    body = f"{MARK0}\n{table(res)}\n{MARK1}"
    text = open(path).read() if os.path.exists(path) else ""
    if MARK0 in text and MARK1 in text:
        text = text[:text.index(MARK0)] + body + text[text.index(MARK1) + len(MARK1):]
    else:
        text = ("# r18: chunked-prefill attention over the FP8 paged-KV cache\n\n`rates.json` is the output of\n\n    " + res["command"]
                + "\n\non one MI355X (tools/prefill_kv8_rate.py tells the method: chains of back-to-back launches between two\n"
                "events, each chain a replayed graph, bf16 and FP8 alternating, time per launch, the median of the chains; the\n"
                "executor's operands; flops and bytes are `Op.flops` / `Op.bytes` of `models/workloads.py`).\n\n" + body
                + "\n\nNot measured: " + "; ".join(res["not_measured"]) + ".\n")
    with open(path, "w") as f:
        f.write(text)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--chains", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chain", type=int, default=20)
    ap.add_argument("--out", default="profiles/r18_prefill_kv8/rates.json")
    ap.add_argument("--decode-profile", default=None, help=f"a copy of {DECODE_PROFILE} (default: that file)")
    ap.add_argument("--kernel-resources", default="", help="kernel:name=value,...;kernel:... from the compiler's remarks")
    a = ap.parse_args(argv)
    if a.chains < 3 or a.rounds < 1 or a.chain < BIG_CHAIN:
        ap.error(f"--chains must be at least 3, --rounds at least 1 and --chain at least {BIG_CHAIN}")
    if not torch.cuda.is_available():
        raise SystemExit("prefill_kv8_rate needs a GPU")
    _native.hip(required=True)
    dev = torch.device("cuda", 0)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {"command": f"{os.path.basename(sys.executable)} {sys.argv[0]} --chains {a.chains} --rounds {a.rounds} --chain {a.chain}",
           "device": torch.cuda.get_device_name(0), "shapes": [], "not_measured": list(NOT_MEASURED)}
    if a.kernel_resources:
        res["kernel_resources"] = {k: {n: int(v) for n, v in (nv.split("=") for nv in rest.split(","))}
                                   for k, rest in (kr.split(":") for kr in a.kernel_resources.split(";"))}
    d = decode_reference(a.decode_profile or os.path.join(root, DECODE_PROFILE))
    if d:
        res["decode_reference"] = d

    for label, o in SHAPES:
        o8 = kv8(o)
        chain = BIG_CHAIN if o.flops > 2e11 else a.chain                  # launches past ~200 us: the shorter chain
        fb, f8 = launcher(o, dev), launcher(o8, dev)
        us = {"bf16": [], "fp8": []}
        for _ in range(a.rounds):                                         # alternating
            us["bf16"] += chain_us(fb, chain, a.chains)
            us["fp8"] += chain_us(f8, chain, a.chains)
        row = {"label": label, "kind": o.kind, "S": o.M, "Hq": o.N, "ctx": o.K, "Hkv": o.rows, "q": o.q,
               "workgroups": o.workgroups(0), "flops": o.flops, "bf16": summary(us["bf16"], o.bytes, chain),
               "fp8": summary(us["fp8"], o8.bytes, chain)}
        for k in ("bf16", "fp8"):
            row[k]["tflops"] = round(o.flops / (row[k]["median_us"] * 1e-6) / 1e12, 1)
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
