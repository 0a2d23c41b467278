"""The host-side GEMM dispatch, pinned against answers recorded before the picker was refactored.

tests/data/gemm_picker_parent.json holds what pick_gemm_tile, gemm_workgroups, pick_split_k,
splitk_workspace_floats and pick_xcd_map answered over the grid below at the commit before
native/hip/loadgen.hip was split into gemm.hip + headers (host code only, no GPU).  The same
function replays the grid here, so a change of tile, grid size, split factor or tile order for any
policy, forced tile, fp8 flag or knob value shows up as a mismatch.

The JSON is produced by this file: check out the commit to record, copy this file into its tests/,
build the HIP extension there and run `python tests/test_gemm_picker_golden.py --write PATH`."""
import json
import os
import sys

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pytest

from k8s_gpu_scheduler_amd import _native
from k8s_gpu_scheduler_amd.models import workloads as W

h = _native.hip(required=False)
pytestmark = pytest.mark.skipif(h is None, reason="HIP extension not built")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "gemm_picker_parent.json")

POLICIES = list(range(14))
TILES = list(range(1, 17))
KS = [64, 128, 1024, 2560]
BUDGETS = [0, 32, 64, 128, 256]
SPLIT_KNOBS = [0, -1, 4]
BLOCK_TILES = [(64, 64), (64, 128), (128, 128), (256, 128), (256, 256)]


def shapes():
    """(M, N) of every catalog / EXTRA GEMM plus shapes around the picker's thresholds: one tile,
    sizes no tile but 64 x 64 divides, the bench's small and large co-run GEMMs, a lone GEMM that
    fills the chip and the policy-8 split-K shape."""
    mn = {(o.M, o.N) for w in list(W.CATALOG.values()) + list(W.EXTRA.values()) for o in w.ops if o.is_gemm}
    mn |= {(256, 256), (192, 320), (640, 384), (1024, 2048), (2048, 1024), (4096, 4096), (8192, 8192), (1024, 2560)}
    return sorted(mn)


def _restore():
    h.reset_knobs()


def record():
    """Every section as nested lists, outermost index first as named in the key."""
    mn = shapes()
    out = {"shapes": [list(s) for s in mn]}
    try:
        _restore()

        def workgroups(fp8, split):
            return [[[h.gemm_workgroups(M, N, K, b, fp8, split) for b in BUDGETS] for K in KS] for M, N in mn]

        tile, wg, wg_split = [], [], []
        for p in POLICIES:
            h.set_gemm_policy(p)
            tile.append([[h.pick_gemm_tile(M, N, b) for b in BUDGETS] for M, N in mn])
            wg.append(workgroups(False, False))
            wg_split.append(workgroups(False, True))
        out["pick_gemm_tile[policy][shape][budget]"] = tile
        out["gemm_workgroups[policy][shape][K][budget]"] = wg
        out["gemm_workgroups_split_workspace[policy][shape][K][budget]"] = wg_split
        h.set_gemm_policy(10)
        out["gemm_workgroups_fp8[shape][K][budget]"] = workgroups(True, False)
        forced = []
        for t in TILES:
            h.set_gemm_tile(t)
            forced.append(workgroups(False, False))
        h.set_gemm_tile(0)
        out["gemm_workgroups_forced[tile-1][shape][K][budget]"] = forced

        split = []
        for p in (8, 10):
            h.set_gemm_policy(p)
            for knob in SPLIT_KNOBS:
                h.set_split_k(knob)
                split.append([[[[h.pick_split_k(M, N, K, b), h.splitk_workspace_floats(M, N, K, b)] for b in BUDGETS]
                               for K in KS] for M, N in mn])
        out["split_k_and_workspace[policy 8,10 x knob 0,-1,4][shape][K][budget]"] = split
        _restore()

        xmap = []
        for blocks in (0, 1):
            h.set_xcd_blocks(blocks)
            for group in (1, 4, 8):
                h.set_xcd_group(group)
                xmap.append([[h.pick_xcd_map(M // bm, N // bn) for bm, bn in BLOCK_TILES] for M, N in mn])
        out["pick_xcd_map[blocks 0,1 x group 1,4,8][shape][block tile]"] = xmap
    finally:
        _restore()
    return out


def test_host_dispatch_matches_the_recorded_parent():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = record()
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key
    # the knobs are back at their defaults
    assert h.pick_gemm_tile(4096, 4096, 64) == 14 and h.pick_split_k(1024, 2560, 2560, 0) == 1
    assert h.pick_xcd_map(16, 16) == 2 | (4 << 8)


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--write":
        sys.exit("usage: python tests/test_gemm_picker_golden.py --write PATH")
    if h is None:
        sys.exit("HIP extension not built")
    with open(sys.argv[2], "w") as f:
        json.dump(record(), f, separators=(",", ":"))
        f.write("\n")
