"""Does a 4-wave 256 x 256 GEMM block (tile 14) find room beside a running stream triad?  (one MI355X)

A tile-14 GEMM stream of 64 blocks (2048^2, a 64-CU share's grid) beside one triad stream, per triad variant
(3 = 256-thread 4x, 5 / 7 = 1024-thread 2x / 3x; native/hip/triad.hip), interleaved over two rounds, for 3 x 256
and 3 x 64 MiB streams: `full` = both streams on the whole chip, `mask64` = the GEMM stream CU-masked to 64 CUs.
Each case is tools/contention_probe.py's: both alone, then together from a common start; it reports each side's
rate alone and co-running.  Usage: triad_wg_probe.py [OUT.json]; the default is triad_wg_probe.json in the
current directory.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
os.environ.setdefault("PROBE_GEMM", "2048")

import contention_probe as cp  # noqa: E402
import torch  # noqa: E402


def main() -> None:
    hip = cp.hip
    hip.set_gemm_tile(14)
    out = {}
    for mib in (256, 64):
        nf = mib << 18
        cp.x, cp.y, cp.z = (torch.ones(nf, device=cp.dev) for _ in range(3))
        cp.TB = 12.0 * nf
        full_g, full_t, mask_g = cp.S(), cp.S(), cp.S((0, 2))
        cp.timed([(full_g.stream, lambda s: cp.enqueue_gemm(s, 10, 64))])           # warm-up
        cp.timed([(full_t.stream, lambda s: cp.enqueue_triad(s, 4))])
        tg = cp.timed([(full_g.stream, lambda s: cp.enqueue_gemm(s, 10, 64))])[0] / 10
        tt = cp.timed([(full_t.stream, lambda s: cp.enqueue_triad(s, 4))])[0] / 4
        ng, nt = max(4, int(15 / tg)), max(2, int(15 / tt))                          # ~15 ms alone each
        for rnd in range(2):
            for v in (3, 5, 7):
                hip.set_triad_variant(v)
                out[f"{mib}MiB_full_v{v}_r{rnd}"] = cp.case(f"{mib}MiB full v{v} r{rnd}", full_g, full_t, ng, nt,
                                                            gbudget=64)
                out[f"{mib}MiB_mask64_v{v}_r{rnd}"] = cp.case(f"{mib}MiB mask64 v{v} r{rnd}", mask_g, full_t,
                                                              max(4, ng // 4), nt, gbudget=64)
    hip.reset_knobs()
    path = sys.argv[1] if len(sys.argv) > 1 else "triad_wg_probe.json"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
