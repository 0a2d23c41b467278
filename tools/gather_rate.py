"""Achieved bytes/s of the embedding-bag gather on the MI355X, with the stream triad as yardstick.

For D in {128, 512, 2048} at pooling 32, from a 1 GiB table (four times the Infinity Cache: rows
from HBM) and a 64 MiB one (rows from the Infinity Cache / L2), about 2 GiB of rows per launch:
HIP events around every launch, a warm-up, the median of --launches launches; bytes are Op.bytes
of models.workloads (rows read + indices + offsets + output).  The triad on a 1 GiB working set
is timed the same way in the same process.  No pass/fail threshold.

    python tools/gather_rate.py [--launches 20] [--out profiles/r07_gather/rates.json]
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

POOL = 32
ROW_BYTES_PER_LAUNCH = 2 << 30


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
    ap.add_argument("--out", default="profiles/r07_gather/rates.json")
    a = ap.parse_args(argv)
    if a.launches < 10:
        ap.error("--launches must be at least 10")
    if not torch.cuda.is_available():
        raise SystemExit("gather_rate needs a GPU")
    h = _native.hip(required=True)
    g = torch.Generator(device="cuda").manual_seed(7)
    res = {"command": " ".join([os.path.basename(sys.executable)] + sys.argv), "device": torch.cuda.get_device_name(0),
           "pooling": POOL, "gather": []}

    n = (1 << 30) // 12 // 4 * 4                               # three fp32 arrays, 1 GiB together
    x, y, z = (torch.rand(n, device="cuda", generator=g) for _ in range(3))
    triad = summary(launch_ms(lambda: loadgen.triad(x, y, z, 1.0001), a.launches), 12 * n)
    res["triad_1gib"] = triad
    print("triad 1 GiB", triad, flush=True)
    del x, y, z

    for table_bytes in (1 << 30, 64 << 20):
        for D in (128, 512, 2048):
            R = table_bytes // (2 * D)
            B = ROW_BYTES_PER_LAUNCH // (POOL * D * 2)
            op = W.Op("gather", B, D, POOL, rows=R)
            table = (torch.randint(-127, 128, (R, D), device="cuda", generator=g, dtype=torch.int8)
                     .to(torch.bfloat16) / 128)
            idx = torch.randint(R, (B, POOL), device="cuda", generator=g, dtype=torch.int32)
            out = torch.empty(B, D, dtype=torch.bfloat16, device="cuda")
            loadgen.embedding_bag(table, idx, out=out)          # checks the indices once
            offsets = torch.arange(B + 1, dtype=torch.int32, device="cuda") * POOL
            flat = idx.view(-1)
            ms = launch_ms(lambda: loadgen.embedding_bag(table, flat, offsets, out=out, check_indices=False),
                           a.launches)
            r = dict(summary(ms, int(op.bytes)), D=D, table_mib=table_bytes >> 20, rows=R, bags=B,
                     workgroups=h.embedding_bag_workgroups(B, 0), vs_triad=0.0)
            r["vs_triad"] = round(r["tbps"] / triad["tbps"], 3)
            res["gather"].append(r)
            print("gather", r, flush=True)
            del table, idx, out, offsets, flat

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
