"""Achieved bytes/s of the paged-KV decode attention on the MI355X, with the stream triad as yardstick.

For contexts of 512, 1,024 and 4,096 tokens, query-head groups of 1 and 8 over 8 KV heads, from a
1 GiB KV cache (four times the Infinity Cache: slabs from HBM) and a 64 MiB one (slabs from the
Infinity Cache / L2): at least 256 sequences (2,048 workgroups) and at least as many KV bytes per
launch as the cache holds, the block tables being random permutations of the cache's blocks laid
end to end, so a launch reads every block equally often.  q, K and V are random (a softmax on zeros
would run faster than one on data).  HIP events around every launch, a warm-up, the median of
--launches launches; bytes are Op.bytes of models.workloads (K and V read + q + out + block table
+ ctx_lens).  The triad on a 1 GiB working set is timed the same way in the same process.  No
pass/fail threshold.

    python tools/decode_attn_rate.py [--launches 20] [--out profiles/r08_decode_attn/rates.json]
                                     [--kernel-resources vgprs=124,agprs=0,waves_per_simd=4]

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

HKV = 8
MIN_SEQS = 256
D, T = W.ATTN_HEAD_DIM, W.ATTN_BLOCK_TOKENS


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
            "launches": len(ms), "bytes": nbytes, "tbps": round(nbytes / (med * 1e-3) / 1e12, 3)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default="profiles/r08_decode_attn/rates.json")
    ap.add_argument("--kernel-resources", default="", help="name=value,... from the compiler's resource-usage remarks")
    a = ap.parse_args(argv)
    if a.launches < 10:
        ap.error("--launches must be at least 10")
    if not torch.cuda.is_available():
        raise SystemExit("decode_attn_rate needs a GPU")
    h = _native.hip(required=True)
    g = torch.Generator(device="cuda").manual_seed(8)
    # the command as it bears on the measurement: where the result is written is left out
    res = {"command": f"{os.path.basename(sys.executable)} {sys.argv[0]} --launches {a.launches}",
           "device": torch.cuda.get_device_name(0), "kv_heads": HKV, "attn": []}
    if a.kernel_resources:
        res["kernel_resources"] = {k: int(v) for k, v in (kv.split("=") for kv in a.kernel_resources.split(","))}

    n = (1 << 30) // 12 // 4 * 4                               # three fp32 arrays, 1 GiB together
    x, y, z = (torch.rand(n, device="cuda", generator=g) for _ in range(3))
    triad = summary(launch_ms(lambda: loadgen.triad(x, y, z, 1.0001), a.launches), 12 * n)
    res["triad_1gib"] = triad
    print("triad 1 GiB", triad, flush=True)
    del x, y, z

    slab = T * D * 2                                           # bytes of one (block, KV head) of K or of V
    for cache_bytes in (1 << 30, 64 << 20):
        nb = cache_bytes // (2 * HKV * slab)
        kc = torch.randn(nb, HKV, T, D, device="cuda", generator=g, dtype=torch.float32).to(torch.bfloat16)
        vc = (torch.rand(nb, HKV, D, T, device="cuda", generator=g) * 2 - 1).to(torch.bfloat16)
        for ctx in (512, 1024, 4096):
            per_seq = ctx // T
            S = max(MIN_SEQS, nb // per_seq)
            reps = -(-S * per_seq // nb)
            table = torch.cat([torch.randperm(nb, device="cuda", generator=g) for _ in range(reps)])[:S * per_seq]
            table = table.to(torch.int32).view(S, per_seq).contiguous()
            ctx_lens = torch.full((S,), ctx, dtype=torch.int32, device="cuda")
            for group in (1, 8):
                hq = group * HKV
                op = W.Op("attn", S, hq, ctx, rows=HKV)
                q = torch.randn(S, hq, D, device="cuda", generator=g).to(torch.bfloat16)
                out = torch.empty(S, hq, D, dtype=torch.bfloat16, device="cuda")
                loadgen.paged_decode_attention(q, kc, vc, table, ctx_lens, out=out)          # checks the table once
                ms = launch_ms(lambda: loadgen.paged_decode_attention(q, kc, vc, table, ctx_lens, out=out, check=False),
                               a.launches)
                r = dict(summary(ms, int(op.bytes)), ctx=ctx, group=group, cache_mib=cache_bytes >> 20, blocks=nb,
                         sequences=S, workgroups=h.paged_decode_workgroups(S, HKV), vs_triad=0.0)
                r["vs_triad"] = round(r["tbps"] / triad["tbps"], 3)
                res["attn"].append(r)
                print("attn", r, flush=True)
                del q, out
            del table, ctx_lens
        del kc, vc

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
