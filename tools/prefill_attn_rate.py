"""Achieved FLOP/s of the paged-KV prefill attention on the MI355X, with torch's SDPA and the project's
bf16 GEMM as yardsticks.

Three shapes over 8 KV heads, each at query-head groups of 1 and 4: the prefill op of the
llm_prefill_2048 workload (2 sequences, a 1,024-token chunk on 4,096 tokens of context); 8 sequences
of 512 tokens with no prefix; 16 sequences with a 128-token chunk on 4,096 tokens (short chunks on a
long context).  The paged cache holds exactly the sequences' blocks, dealt out by a random
permutation.  q, K and V are random (a softmax on zeros would run faster than one on data).  In the
same process, on contiguous K / V of the same logical shapes [S, H, tokens, 128] (the KV heads
repeated per group outside the timed region), torch.nn.functional.scaled_dot_product_attention with
a causal mask -- `is_causal=True` where the chunk is the whole context, else a boolean mask aligned
to the last token, since is_causal aligns to the first -- and the bf16 GEMM at 4096^3 as the MFMA
yardstick.  HIP events around every launch, a warm-up of 3, the median of --launches launches; flops
are Op.flops of models.workloads (4 * 128 per query, head and token at or below the query: SDPA is
credited with the same causal count, whatever it computes).  No pass/fail threshold.

    python tools/prefill_attn_rate.py [--launches 20] [--out profiles/r09_prefill_attn/rates.json]
                                      [--kernel-resources vgprs=212,agprs=0,lds=0,waves_per_simd=2]

--kernel-resources is recorded as given: the kernel's registers and occupancy as the compiler's
resource-usage remarks state them (hipcc -Rpass-analysis=kernel-resource-usage).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from k8s_gpu_scheduler_amd import _native  # noqa: E402
from k8s_gpu_scheduler_amd.models import workloads as W  # noqa: E402
from k8s_gpu_scheduler_amd.ops import loadgen  # noqa: E402

HKV = 8
D, T = W.ATTN_HEAD_DIM, W.ATTN_BLOCK_TOKENS
SHAPES = (("llm_prefill_2048", 2, 1024, 4096), ("no_prefix", 8, 512, 512), ("short_chunks", 16, 128, 4096))   # (S, q, ctx)
GROUPS = (1, 4)


def launch_ms(fn, launches, warm=3):
    """Per-launch device times (ms) of `launches` launches after `warm` untimed ones."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for e0, e1 in evs:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in evs]


def summary(ms, flops):
    med = statistics.median(ms)
    return {"median_us": round(med * 1e3, 2), "min_us": round(min(ms) * 1e3, 2), "max_us": round(max(ms) * 1e3, 2),
            "launches": len(ms), "flops": flops, "tflops": round(flops / (med * 1e-3) / 1e12, 2)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default="profiles/r09_prefill_attn/rates.json")
    ap.add_argument("--kernel-resources", default="", help="name=value,... from the compiler's resource-usage remarks")
    a = ap.parse_args(argv)
    if a.launches < 10:
        ap.error("--launches must be at least 10")
    if not torch.cuda.is_available():
        raise SystemExit("prefill_attn_rate needs a GPU")
    h = _native.hip(required=True)
    g = torch.Generator(device="cuda").manual_seed(9)
    # the command as it bears on the measurement: where the result is written is left out
    res = {"command": f"{os.path.basename(sys.executable)} {sys.argv[0]} --launches {a.launches}",
           "device": torch.cuda.get_device_name(0), "kv_heads": HKV, "prefill": []}
    if a.kernel_resources:
        res["kernel_resources"] = {k: int(v) for k, v in (kv.split("=") for kv in a.kernel_resources.split(","))}

    n = 4096
    x = (torch.rand(n, n, device="cuda", generator=g) * 2 - 1).to(torch.bfloat16)
    y = ((torch.rand(n, n, device="cuda", generator=g) * 2 - 1) * 0.05).to(torch.bfloat16)
    z = torch.empty(n, n, dtype=torch.bfloat16, device="cuda")
    gemm = summary(launch_ms(lambda: loadgen.gemm(x, y, out=z), a.launches), loadgen.gemm_flops(n, n, n))
    res["gemm_4096"] = gemm
    print("gemm 4096^3", gemm, flush=True)
    del x, y, z

    for name, S, qn, ctx in SHAPES:
        per_seq = ctx // T
        nb = S * per_seq
        kc = torch.randn(nb, HKV, T, D, device="cuda", generator=g).to(torch.bfloat16)
        vc = (torch.rand(nb, HKV, D, T, device="cuda", generator=g) * 2 - 1).to(torch.bfloat16)
        table = torch.randperm(nb, device="cuda", generator=g).to(torch.int32).view(S, per_seq)
        ctx_lens = torch.full((S,), ctx, dtype=torch.int32, device="cuda")
        q_start = torch.arange(S + 1, dtype=torch.int32, device="cuda") * qn
        # the same tokens, contiguous: [S, HKV, ctx, D]
        kd = kc[table.long()].permute(0, 2, 1, 3, 4).reshape(S, HKV, ctx, D)
        vd = vc[table.long()].permute(0, 2, 1, 4, 3).reshape(S, HKV, ctx, D)
        for group in GROUPS:
            hq = group * HKV
            op = W.Op("prefill", S, hq, ctx, rows=HKV, q=qn)
            q = torch.randn(S * qn, hq, D, device="cuda", generator=g).to(torch.bfloat16)
            out = torch.empty_like(q)
            loadgen.paged_prefill_attention(q, kc, vc, table, ctx_lens, q_start, out=out)      # checks the operands once
            ms = launch_ms(lambda: loadgen.paged_prefill_attention(q, kc, vc, table, ctx_lens, q_start, max_q_len=qn,
                                                                   out=out, check=False), a.launches)
            r = dict(summary(ms, op.flops), shape=name, sequences=S, chunk=qn, ctx=ctx, group=group,
                     cache_mib=(kc.numel() + vc.numel()) * 2 >> 20, workgroups=h.paged_prefill_workgroups(S, hq, HKV, qn))
            r["vs_gemm"] = round(r["tflops"] / gemm["tflops"], 3)
            # SDPA on the contiguous copy
            qd = q.view(S, qn, hq, D).transpose(1, 2)
            ke, ve = kd.repeat_interleave(group, 1), vd.repeat_interleave(group, 1)
            if qn == ctx:
                kw, r["sdpa_mask"] = dict(is_causal=True), "is_causal"
            else:
                pos = ctx - qn + torch.arange(qn, device="cuda")
                kw = dict(attn_mask=torch.arange(ctx, device="cuda")[None, :] <= pos[:, None])
                r["sdpa_mask"] = "boolean, aligned to the last token"
            ref = F.scaled_dot_product_attention(qd, ke, ve, **kw)
            r["max_abs_diff_vs_sdpa"] = round((ref.transpose(1, 2).reshape(S * qn, hq, D).float() - out.float()).abs().max().item(), 5)
            sd = summary(launch_ms(lambda: F.scaled_dot_product_attention(qd, ke, ve, **kw), a.launches), op.flops)
            r["sdpa_tflops"], r["sdpa_median_us"] = sd["tflops"], sd["median_us"]
            r["vs_sdpa"] = round(r["tflops"] / sd["tflops"], 3)
            res["prefill"].append(r)
            print("prefill", r, flush=True)
            del q, out, qd, ke, ve, ref, kw
        del kc, vc, kd, vd, table

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
