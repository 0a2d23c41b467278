"""Achieved bytes/s of the RoPE + paged-KV append on the MI355X, with the stream triad as the yardstick.

Three shapes, 32 query heads over 8 KV heads (groups of 4): the rope_append op of the
llm_layer_decode_256 workload (256 sequences, one new token each on 1,024 tokens of context -- slot 31
of each sequence's last block), the op of llm_layer_prefill_2048 (2 sequences, a 1,024-token chunk on
4,096 tokens) and a mid shape (16 sequences, a 128-token chunk on 4,096 tokens).  The paged cache holds
exactly the sequences' blocks, dealt out by a random permutation; qkv is random, cos_sin is
rope_table(ctx).  In the same process the stream triad over 3 x 96 MiB (more than the Infinity Cache).
HIP events around every launch, a warm-up of 3, the median of --launches launches; bytes are Op.bytes
of models.workloads (qkv read, q_out, K and V written, a cos / sin row per token, the int operands).
The append is small and latency-dominated: microseconds are the figure to read, bytes/s against the
triad's says how far from a streaming kernel it is.  No pass/fail threshold.

    python tools/rope_append_rate.py [--launches 20] [--out profiles/r11_rope_append/rates.json]
                                     [--kernel-resources vgprs=..,agprs=..,lds=..,waves_per_simd=..]

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

from k8s_gpu_scheduler_amd import _native  # noqa: E402
from k8s_gpu_scheduler_amd.models import workloads as W  # noqa: E402
from k8s_gpu_scheduler_amd.ops import loadgen  # noqa: E402

HQ, HKV = 32, 8
D, T = W.ATTN_HEAD_DIM, W.ATTN_BLOCK_TOKENS
SHAPES = (("llm_layer_decode_256", 256, 1, 1024), ("llm_layer_prefill_2048", 2, 1024, 4096),
          ("mid_chunks", 16, 128, 4096))                                                     # (S, q, ctx)
TRIAD_FLOATS = 24 << 20


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


def summary(ms, nbytes):
    med = statistics.median(ms)
    return {"median_us": round(med * 1e3, 2), "min_us": round(min(ms) * 1e3, 2), "max_us": round(max(ms) * 1e3, 2),
            "launches": len(ms), "bytes": nbytes, "gbps": round(nbytes / (med * 1e-3) / 1e9, 1)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default="profiles/r11_rope_append/rates.json")
    ap.add_argument("--kernel-resources", default="", help="name=value,... from the compiler's resource-usage remarks")
    a = ap.parse_args(argv)
    if a.launches < 10:
        ap.error("--launches must be at least 10")
    if not torch.cuda.is_available():
        raise SystemExit("rope_append_rate needs a GPU")
    h = _native.hip(required=True)
    g = torch.Generator(device="cuda").manual_seed(11)
    # the command as it bears on the measurement: where the result is written is left out
    res = {"command": f"{os.path.basename(sys.executable)} {sys.argv[0]} --launches {a.launches}",
           "device": torch.cuda.get_device_name(0), "query_heads": HQ, "kv_heads": HKV, "rope_append": []}
    if a.kernel_resources:
        res["kernel_resources"] = {k: int(v) for k, v in (kv.split("=") for kv in a.kernel_resources.split(","))}

    x, y, z = (torch.ones(TRIAD_FLOATS, dtype=torch.float32, device="cuda") for _ in range(3))
    triad = summary(launch_ms(lambda: loadgen.triad(x, y, z, 1.0001), a.launches), W.Op("triad", n_floats=TRIAD_FLOATS).bytes)
    res["triad"] = triad
    print("triad", triad, flush=True)
    del x, y, z

    for name, S, qn, ctx in SHAPES:
        op = W.Op("rope_append", S, HQ, ctx, rows=HKV, q=qn)
        per_seq = ctx // T
        nb = S * per_seq
        qkv = torch.randn(S * qn, HQ + 2 * HKV, D, device="cuda", generator=g).to(torch.bfloat16)
        cos_sin = loadgen.rope_table(ctx).cuda()
        kc = torch.zeros(nb, HKV, T, D, dtype=torch.bfloat16, device="cuda")
        vc = torch.zeros(nb, HKV, D, T, dtype=torch.bfloat16, device="cuda")
        table = torch.randperm(nb, device="cuda", generator=g).to(torch.int32).view(S, per_seq)
        ctx_lens = torch.full((S,), ctx, dtype=torch.int32, device="cuda")
        q_start = torch.arange(S + 1, dtype=torch.int32, device="cuda") * qn
        q_out = torch.empty(S * qn, HQ, D, dtype=torch.bfloat16, device="cuda")
        loadgen.rope_append(qkv, cos_sin, kc, vc, table, ctx_lens, q_start, q_out=q_out)      # checks the operands once
        ms = launch_ms(lambda: loadgen.rope_append(qkv, cos_sin, kc, vc, table, ctx_lens, q_start, max_q_len=qn,
                                                   q_out=q_out, check=False), a.launches)
        r = dict(summary(ms, op.bytes), shape=name, sequences=S, chunk=qn, ctx=ctx, flops=op.flops,
                 cache_mib=(kc.numel() + vc.numel()) * 2 >> 20, workgroups=h.rope_append_workgroups(S, HKV, qn))
        r["vs_triad"] = round(r["gbps"] / triad["gbps"], 4)
        res["rope_append"].append(r)
        print("rope_append", r, flush=True)
        del qkv, cos_sin, kc, vc, table, q_out

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
