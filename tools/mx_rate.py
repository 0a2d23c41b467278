"""Time per launch of the MX kernels on the MI355X -- `gemm_mx` with fp8 and with fp4 activations beside `gemm` (bf16)
and `gemm_fp8` (unit scales), and `quantize_mx` in both formats beside the stream triad -- all in one process, on
random operands (zero-filled ones read high).

GEMMs: 4096^3 and 8192^3, then the four projection shapes (QKV 6144 x 4096, output 4096 x 4096, gate / up 28672 x 4096,
down 4096 x 14336) at the rows of llm_mx_block_decode_256 (256) and llm_mx_block_prefill_2048 (2048).  bf16 and fp8
operands are uniform in [-1, 1) (the weights times 0.05, times 16 for fp8, as the executor makes them); MX operands are
the executor's (random element bytes without the fp8 NaN codes, scale bytes from [120, 127]).  For the decode rows
`weights / time` is the bytes of the weight matrix (elements and scales) over the launch time, as a fraction of the
stream triad's bytes/s over a working set of 1 GiB.  Quantiser: 256 x 4096, 2048 x 14336, 8192 x 8192.

The method is that of tools/moe_rate.py: every figure is the time of a CHAIN of back-to-back launches on one stream
between two events, divided by the chain's length (--chain, default 20; 10 for the triad and launches past 300 us),
the chain captured once into a graph and replayed, a warm-up chain first, then the median of --chains chains.  No
pass/fail threshold.

    python tools/mx_rate.py [--chains 10] [--chain 20] [--out profiles/r16_mx/rates.json]
                            [--kernel-resources "gemm_mx_128_fp4:vgprs=..,lds=..;..."]

--kernel-resources is recorded as given: registers, LDS, scratch and waves per SIMD as the compiler's resource-usage
remarks state them (hipcc -Rpass-analysis=kernel-resource-usage).  README.md beside the output gets the tables between
its `<!-- table -->` markers; the rest of an existing README.md is kept.
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
SQUARES = (4096, 8192)
PROJECTIONS = ((6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336))          # (N, K) of _llm_block's GEMMs
QUANT_SHAPES = ((256, 4096), (2048, 14336), (8192, 8192))
KINDS = ("gemm", "gemm_fp8", "gemm_mx fp8", "gemm_mx fp4")
NOT_MEASURED = ("co-run groups with the MX kernels", "other block tiles, a 256-deep fp4 K tile, more LDS stages",
                "skinny M (below 64 rows)", "scales through LDS or as one dword per row and K tile")


def gemm_case(kind, M, N, K, g, dev):
    """(launch, Op) of one GEMM kind at M x N x K on fresh random operands."""
    c = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
    if kind in ("gemm", "gemm_fp8"):
        a = (torch.rand(M, K, device=dev, generator=g) * 2 - 1).to(torch.bfloat16)
        bt = ((torch.rand(N, K, device=dev, generator=g) * 2 - 1) * 0.05).to(torch.bfloat16)
        if kind == "gemm":
            return (lambda: loadgen.gemm(a, bt, out=c)), W.Op("gemm", M, N, K, relu=False)
        a8, b8 = a.to(loadgen.FP8), (bt * 16).to(loadgen.FP8)
        return (lambda: loadgen.gemm_fp8(a8, b8, out=c)), W.Op("gemm8", M, N, K, relu=False)
    fmt = kind.split()[1]
    cpu = torch.Generator().manual_seed(16)
    a_q, a_s = executor._mx_random(M, K, fmt, cpu, dev)
    w_q, w_s = executor._mx_random(N, K, "fp4", cpu, dev)
    return (lambda: loadgen.gemm_mx(a_q, a_s, w_q, w_s, fmt, out=c)), W.Op("gemm_mx", M, N, K, relu=False, fmt=fmt)


def gemm_table(res):
    rows = ["| shape (M x N x K) | " + " | ".join(f"`{k}`" for k in KINDS) + " | fp8 / bf16 | mx fp8 / fp8 | mx fp4 / fp8 | mx fp4 / mx fp8 |",
            "|---|" + "---|" * (len(KINDS) + 4)]
    for s in res["gemms"]:
        r = s["kinds"]
        cells = [f"{r[k]['median_us']} us, {r[k]['tflops']:.0f} TF" + (f", weights {r[k]['weights_vs_triad']:.2f} of the triad" if "weights_vs_triad" in r[k] else "")
                 for k in KINDS]
        t = {k: r[k]["median_us"] for k in KINDS}
        rows.append(f"| {s['label']} {s['M']} x {s['N']} x {s['K']} | " + " | ".join(cells)
                    + f" | {t['gemm'] / t['gemm_fp8']:.2f}x | {t['gemm_fp8'] / t['gemm_mx fp8']:.2f}x | {t['gemm_fp8'] / t['gemm_mx fp4']:.2f}x "
                      f"| {t['gemm_mx fp8'] / t['gemm_mx fp4']:.2f}x |")
    return "\n".join(rows)


def quant_table(res):
    rows = ["| kernel | rows x row length | workgroups | per launch | bytes | bytes/s | of the triad's |", "|---|---|---|---|---|---|---|"]
    for r in res["quantize"]:
        rows.append(f"| `quantize_mx {r['fmt']}` | {r['rows']:,} x {r['cols']:,} | {r['workgroups']:,} | {r['median_us']} us | "
                    f"{r['bytes'] / 1e6:.1f} MB | {r['gbps'] / 1e3:.2f} TB/s | {r['vs_triad']:.3f} |")
    t = res["triad"]
    rows.append(f"| stream triad | 3 x 352 MiB | | {t['median_us']} us | {t['bytes'] / 1e6:.0f} MB | {t['gbps'] / 1e3:.2f} TB/s | 1 |")
    return "\n".join(rows)


def write_readme(path, res):
    body = f"{MARK0}\n{gemm_table(res)}\n\n{quant_table(res)}\n{MARK1}"
    text = open(path).read() if os.path.exists(path) else ""
    if MARK0 in text and MARK1 in text:
        text = text[:text.index(MARK0)] + body + text[text.index(MARK1) + len(MARK1):]
    else:
        text = ("# r16: MX quantiser and MXFP4-weight GEMM\n\n`rates.json` is the output of\n\n    " + res["command"]
                + "\n\non one MI355X (tools/mx_rate.py tells the method: chains of back-to-back launches between two events,\n"
                "each chain a replayed graph, time per launch, the median of the chains; random operands).  TF is 2 M N K\n"
                "over the launch time; `weights` is the weight matrix's bytes over the launch time as a fraction of the\n"
                "stream triad's bytes/s.\n\n" + body + "\n\nNot measured: " + "; ".join(res["not_measured"]) + ".\n")
    with open(path, "w") as f:
        f.write(text)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--chains", type=int, default=10)
    ap.add_argument("--chain", type=int, default=20)
    ap.add_argument("--out", default="profiles/r16_mx/rates.json")
    ap.add_argument("--kernel-resources", default="", help="kernel:name=value,...;kernel:... from the compiler's remarks")
    a = ap.parse_args(argv)
    if a.chains < 5 or a.chain < BIG_CHAIN:
        ap.error(f"--chains must be at least 5 and --chain at least {BIG_CHAIN}")
    if not torch.cuda.is_available():
        raise SystemExit("mx_rate needs a GPU")
    h = _native.hip(required=True)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cuda").manual_seed(16)
    res = {"command": f"{os.path.basename(sys.executable)} {sys.argv[0]} --chains {a.chains} --chain {a.chain}",
           "device": torch.cuda.get_device_name(0), "gemms": [], "quantize": [], "not_measured": list(NOT_MEASURED)}
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

    shapes = [("square", s, s, s) for s in SQUARES]
    shapes += [(w.name, w.batch, N, K) for w in W.LLM_MX.values() for N, K in PROJECTIONS]
    for label, M, N, K in shapes:
        row = {"label": label, "M": M, "N": N, "K": K, "kinds": {}}
        for kind in KINDS:
            launch, o = gemm_case(kind, M, N, K, g, dev)
            chain = BIG_CHAIN if o.flops > 3e11 else a.chain                # launches past ~300 us: the shorter chain
            r = dict(summary(chain_us(launch, chain, a.chains), o.bytes, chain), flops=o.flops, workgroups=o.workgroups(0))
            r["tflops"] = round(o.flops / r["median_us"] / 1e6, 1)
            if M == 256:                                                  # weight-bound: the weight matrix's bytes / time
                wb = {"gemm": 2.0, "gemm_fp8": 1.0}.get(kind, 0.5 + 1.0 / W.MX_BLOCK) * N * K
                r.update(weight_bytes=wb, weight_gbps=round(wb / (r["median_us"] * 1e-6) / 1e9, 1))
                r["weights_vs_triad"] = round(r["weight_gbps"] / triad["gbps"], 4)
            row["kinds"][kind] = r
            print(label, M, N, K, kind, r, flush=True)
            del launch
            torch.cuda.empty_cache()
        res["gemms"].append(row)

    for fmt in loadgen.MX_FORMATS:
        for T, D in QUANT_SHAPES:
            o = W.Op("quant_mx", T, D, fmt=fmt)
            xin = torch.randn(T, D, device=dev, generator=g).to(torch.bfloat16)
            q = torch.empty(T, loadgen.mx_row_bytes(fmt, D), dtype=loadgen.mx_element_dtype(fmt), device=dev)
            s = torch.empty(T, D // loadgen.MX_BLOCK, dtype=torch.uint8, device=dev)
            r = dict(summary(chain_us(lambda: loadgen.quantize_mx(xin, fmt, out=q, scales=s), a.chain, a.chains), o.bytes, a.chain),
                     fmt=fmt, rows=T, cols=D, workgroups=h.quantize_mx_workgroups(T, D))
            r["vs_triad"] = round(r["gbps"] / triad["gbps"], 4)
            res["quantize"].append(r)
            print("quantize_mx", r, flush=True)
            del xin, q, s
            torch.cuda.empty_cache()

    big = next(s for s in res["gemms"] if s["M"] == 8192)["kinds"]
    res["fp4_beats_fp8_at_8192"] = big["gemm_mx fp4"]["median_us"] < big["gemm_fp8"]["median_us"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    write_readme(os.path.join(os.path.dirname(os.path.abspath(a.out)), "README.md"), res)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
