"""Split-KV against unsplit paged-KV decode attention on the MI355X for a few long sequences.

For 1, 8 and 32 sequences of 32,768 tokens and 8 sequences of 4,096, query-head groups of 1 and 4
over 8 KV heads, and kv_splits in (1, 2, 4, 8, 16, 32): the device time of
loadgen.paged_decode_attention -- one launch for kv_splits = 1, the split and merge pair otherwise,
the workspace passed in.  q, K and V are random; the cache is 1 GiB (8,192 blocks) and the block
tables are random permutations of its blocks laid end to end, so 8 sequences of 32,768 tokens name
every block once, 32 name each four times, and the two small shapes name 1,024 blocks (128 MiB,
which fits the Infinity Cache: `touched_mib` says what a launch reads).  HIP events around every
launch (pair), a warm-up, the median of --launches launches; bytes are Op.bytes of models.workloads
("attn" for kv_splits = 1, "attn_split" -- the workspace written and read once on top -- otherwise).

The unsplit launch is measured again beside every split count (kv_splits = 1, then the count, per
shape) and the whole sweep runs --passes times, so every shape has passes x 5 unsplit medians: their
spread is what a split count has to beat.  The triad on a 1 GiB working set is timed the same way
in the same process.  No pass/fail threshold.

    python tools/decode_split_rate.py [--launches 20] [--passes 2] [--out profiles/r10_decode_split/rates.json]
                                      [--kernel-resources split_vgprs=128,...]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from decode_attn_rate import launch_ms, summary  # noqa: E402
from k8s_gpu_scheduler_amd import _native  # noqa: E402
from k8s_gpu_scheduler_amd.models import workloads as W  # noqa: E402
from k8s_gpu_scheduler_amd.ops import loadgen  # noqa: E402

HKV = 8
D, T = W.ATTN_HEAD_DIM, W.ATTN_BLOCK_TOKENS
SHAPES = ((1, 32768), (8, 32768), (32, 32768), (8, 4096))           # (sequences, context tokens)
GROUPS = (1, 4)
SPLITS = (2, 4, 8, 16, 32)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--out", default="profiles/r10_decode_split/rates.json")
    ap.add_argument("--kernel-resources", default="", help="name=value,... from the compiler's resource-usage remarks")
    a = ap.parse_args(argv)
    if a.launches < 20 or a.passes < 2:
        ap.error("--launches must be at least 20 and --passes at least 2")
    if not torch.cuda.is_available():
        raise SystemExit("decode_split_rate needs a GPU")
    h = _native.hip(required=True)
    g = torch.Generator(device="cuda").manual_seed(10)
    res = {"command": f"{os.path.basename(sys.executable)} {sys.argv[0]} --launches {a.launches} --passes {a.passes}",
           "device": torch.cuda.get_device_name(0), "kv_heads": HKV, "attn": [], "shapes": []}
    if a.kernel_resources:
        res["kernel_resources"] = {k: int(v) for k, v in (kv.split("=") for kv in a.kernel_resources.split(","))}

    n = (1 << 30) // 12 // 4 * 4                               # three fp32 arrays, 1 GiB together
    x, y, z = (torch.rand(n, device="cuda", generator=g) for _ in range(3))
    triad = summary(launch_ms(lambda: loadgen.triad(x, y, z, 1.0001), a.launches), 12 * n)
    res["triad_1gib"] = triad
    print("triad 1 GiB", triad, flush=True)
    del x, y, z

    slab = T * D * 2                                           # bytes of one (block, KV head) of K or of V
    nb = (1 << 30) // (2 * HKV * slab)
    kc = torch.randn(nb, HKV, T, D, device="cuda", generator=g, dtype=torch.float32).to(torch.bfloat16)
    vc = (torch.rand(nb, HKV, D, T, device="cuda", generator=g) * 2 - 1).to(torch.bfloat16)
    ws = torch.empty(loadgen.decode_split_workspace_floats(max(s for s, _ in SHAPES), max(GROUPS) * HKV, max(SPLITS)),
                     dtype=torch.float32, device="cuda")
    for ps in range(a.passes):
        for S, ctx in SHAPES:
            per_seq = ctx // T
            reps = -(-S * per_seq // nb)
            table = torch.cat([torch.randperm(nb, device="cuda", generator=g) for _ in range(reps)])[:S * per_seq]
            table = table.to(torch.int32).view(S, per_seq).contiguous()
            ctx_lens = torch.full((S,), ctx, dtype=torch.int32, device="cuda")
            for group in GROUPS:
                hq = group * HKV
                q = torch.randn(S, hq, D, device="cuda", generator=g).to(torch.bfloat16)
                out = torch.empty(S, hq, D, dtype=torch.bfloat16, device="cuda")
                loadgen.paged_decode_attention(q, kc, vc, table, ctx_lens, out=out)          # checks the table once

                def measure(k):
                    op = W.Op("attn", S, hq, ctx, rows=HKV) if k == 1 else W.Op("attn_split", S, hq, ctx, rows=HKV, splits=k)
                    ms = launch_ms(lambda: loadgen.paged_decode_attention(q, kc, vc, table, ctx_lens, out=out, check=False,
                                                                          kv_splits=k, workspace=ws), a.launches)
                    wg = h.paged_decode_workgroups(S, HKV) if k == 1 else h.paged_decode_split_workgroups(S, HKV, k)
                    r = dict(summary(ms, int(op.bytes)), sequences=S, ctx=ctx, group=group, kv_splits=k, workgroups=wg,
                             touched_mib=min(S * per_seq, nb) * 2 * HKV * slab >> 20, beside=0, vs_triad=0.0)
                    r["vs_triad"] = round(r["tbps"] / triad["tbps"], 3)
                    r["pass"] = ps
                    return r
                for k in SPLITS:
                    for kk in (1, k):                          # the unsplit launch beside every split count
                        r = measure(kk)
                        r["beside"] = k
                        res["attn"].append(r)
                        print("attn", r, flush=True)
                del q, out
            del table, ctx_lens

    # per shape: the unsplit medians' spread and every split count's medians, best first
    for S, ctx in SHAPES:
        for group in GROUPS:
            rows = [r for r in res["attn"] if (r["sequences"], r["ctx"], r["group"]) == (S, ctx, group)]
            un = sorted(r["median_us"] for r in rows if r["kv_splits"] == 1)
            per = {k: sorted(r["median_us"] for r in rows if r["kv_splits"] == k) for k in SPLITS}
            best = min(SPLITS, key=lambda k: statistics.median(per[k]))
            sh = {"sequences": S, "ctx": ctx, "group": group, "unsplit_median_us": un,
                  "unsplit_spread": round(un[-1] / un[0] - 1, 4), "split_median_us": {str(k): v for k, v in per.items()},
                  "fastest_kv_splits": best,
                  "speedup_of_fastest": round(statistics.median(un) / statistics.median(per[best]), 3),
                  "speedup_worst_case": round(un[0] / per[best][-1], 3)}
            res["shapes"].append(sh)
            print("shape", sh, flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
