"""The native launch plan and the knob table (host code only, no GPU).

gemm_plan(...) answers, without a GPU, which kernel instantiation, grid, block and tile order
gemm_bf16_nt launches; knobs() / knob_defaults() / reset_knobs() read and reset the launch knobs.  Every
GPU test checks results, and every selectable variant computes the same result, so this module is what
pins WHICH kernel a tile launches:

  * against tests/data/gemm_kernels_parent.json, a kernel trace (kernel name, grid, block per launch)
    recorded on an MI355X at the commit before the three launchers and their switch became one tile table;
  * against literal expectations written from that commit's code: template arguments, threads per block,
    tile order (xmap), epilogue and the order in which a tile is resolved;
  * against gemm_workgroups over the picker golden's grid.

The JSON is produced by this file.  On a machine with the GPU: check out the commit to record, copy this
file into its tests/, build the HIP extension there and run `python tests/test_gemm_plan_cpu.py --write PATH`.
That starts one kernel-trace-only rocprofv3 run of `python tests/test_gemm_plan_cpu.py --launch` (tiny
launches of every case of cases(), an xcd_probe launch of CASE_MARK blocks after each) and writes the
launches of every case.  The recorder uses only what the module offered before the plan existed."""
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if "--launch" in sys.argv:
        import torch        # noqa: F401  (before the HIP extension, so that both use the HIP runtime torch loads)

import pytest

from k8s_gpu_scheduler_amd import _native

h = _native.hip(required=False)
pytestmark = pytest.mark.skipif(h is None, reason="HIP extension not built")

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "data", "gemm_kernels_parent.json")
ACTS = [(False, False), (False, True), (True, False), (True, True)]      # (relu, bias)
CASE_MARK = 3            # blocks of the xcd_probe launch that ends a case in the trace

# The ten launch knobs: name -> (min, max, default); None = any integer, read as on / off.
KNOBS = {"gemm_tile": (0, 16, 0), "gemm_policy": (0, 13, 10), "split_k": (-1, 8, 0), "w4_probe": (0, 3, 0),
         "xcd_group": (1, 64, 4), "triad_variant": (0, 10, 6), "w4_prio": (None, None, 0),
         "wide_epilogue": (None, None, 1), "xcd_blocks": (None, None, 1), "lone_plain_order": (None, None, 1)}

# Every tile's kernel as the parent's switch and launchers spelled it ({r}, {b}: relu, bias; {w}: wide
# epilogue), threads per block, and the tiles a lone GEMM runs in the plain tile order.
PLAIN = "gemm_bf16_nt_kernel<{}, {{r}}, {{b}}, {}, {{w}}>"
TILE_KERNEL = {1: PLAIN.format("128, 128, 2, 2, 2", "2, 64, true"), 2: PLAIN.format("64, 128, 2, 2, 2", "2, 64, false"),
               3: PLAIN.format("64, 64, 2, 2, 2", "2, 64, true"), 4: PLAIN.format("256, 256, 2, 4, 1", "2, 64, true"),
               5: PLAIN.format("256, 128, 4, 2, 1", "2, 64, false"), 6: PLAIN.format("128, 128, 2, 2, 2", "2, 64, false"),
               7: PLAIN.format("64, 128, 2, 2, 2", "3, 64, false"), 8: PLAIN.format("256, 128, 4, 2, 1", "3, 64, false"),
               9: "gemm_bf16_nt_256_8ph<{r}, {b}, false, false, false, 256>",
               10: "gemm_bf16_nt_256_8ph<{r}, {b}, true, {w}, false, 256>",
               11: PLAIN.format("128, 128, 2, 2, 1", "3, 64, true"), 12: PLAIN.format("128, 128, 2, 2, 1", "4, 64, true"),
               13: "gemm_bf16_nt_256_8ph<{r}, {b}, true, {w}, false, 128>",
               14: "gemm_bf16_nt_256_w4l<{r}, {b}, 0, false, 256, 256>",
               15: "gemm_bf16_nt_256_w4l<{r}, {b}, 0, false, 128, 256>",
               16: "gemm_bf16_nt_256_w4l<{r}, {b}, 0, false, 128, 128>"}
TILE_THREADS = {1: 256, 2: 256, 3: 256, 4: 512, 5: 512, 6: 256, 7: 256, 8: 512, 9: 512, 10: 512, 11: 256, 12: 256,
                13: 512, 14: 256, 15: 256, 16: 256}
TILE_BM = {1: 128, 2: 64, 3: 64, 4: 256, 5: 256, 6: 128, 7: 64, 8: 256, 9: 256, 10: 256, 11: 128, 12: 128,
           13: 256, 14: 256, 15: 256, 16: 128}
TILE_BN = {1: 128, 2: 128, 3: 64, 4: 256, 5: 128, 6: 128, 7: 128, 8: 128, 9: 256, 10: 256, 11: 128, 12: 128,
           13: 128, 14: 256, 15: 128, 16: 128}
LONE_PLAIN_TILES = (9, 10, 13, 14, 15, 16)
WIDE_ONLY_TILES = (14, 15, 16)
SMALL_K_FALLBACK = {9: 4, 10: 4, 13: 5, 14: 4, 15: 5, 16: 1}
NARROW_C_FALLBACK = {14: 10, 15: 13, 16: 1}


def flag(x):
    return "true" if x else "false"


def tile_kernel(tile, relu, bias, wide):
    return TILE_KERNEL[tile].format(r=flag(relu), b=flag(bias), w=flag(wide))


def kernel_id(name):
    """A demangled kernel name reduced to the template name and its argument list: demanglers differ on the
    parameter types (__bf16) and on decorations after them."""
    name = name.split("(")[0].strip()
    name = name[5:] if name.startswith("void ") else name
    return re.sub(r"\s+", " ", name[4:] if name.startswith("gs::") else name)


@pytest.fixture(autouse=True)
def default_knobs():
    h.reset_knobs()
    yield
    h.reset_knobs()


def set_knobs(settings):
    for name, value in settings.items():
        getattr(h, "set_" + name)(value)


def plan(M, N, K, budget=0, relu=False, bias=False, aligned=True):
    """[(tile, kernel, grid, block, xmap, m0, m)] of the call as ops.loadgen.gemm makes it (it offers a
    workspace whenever the picker wants split-K)."""
    p = h.gemm_plan(M, N, K, budget, relu, bias, aligned, True)
    return p["split"], [(l["tile"], kernel_id(l["kernel"]), l["grid"], l["block"], l["xmap"], l["m0"], l["m"])
                        for l in p["launches"]]


# ------------------------------------------------------------------------------------------------
# the knob table
# ------------------------------------------------------------------------------------------------
def test_knob_defaults_are_the_literal_ten():
    assert h.knob_defaults() == {"gemm_tile": 0, "gemm_policy": 10, "split_k": 0, "w4_probe": 0, "w4_prio": 0,
                                 "wide_epilogue": 1, "xcd_blocks": 1, "lone_plain_order": 1, "xcd_group": 4,
                                 "triad_variant": 6}
    assert h.knobs() == h.knob_defaults() and sorted(KNOBS) == sorted(h.knobs())
    assert {k: v[2] for k, v in KNOBS.items()} == h.knob_defaults()


@pytest.mark.parametrize("name", sorted(KNOBS))
def test_setter_round_trips_and_bounds(name):
    lo, hi, default = KNOBS[name]
    setter = getattr(h, "set_" + name)
    others = {k: v for k, v in h.knobs().items() if k != name}
    if lo is None:                                   # on / off: any integer
        for value, stored in ((0, 0), (1, 1), (7, 1), (-3, 1), (0, 0)):
            setter(value)
            assert h.knobs()[name] == stored
    else:
        for value in range(lo, hi + 1):
            setter(value)
            assert h.knobs()[name] == (0 if name == "split_k" and value == 1 else value)
        keep = hi - 1
        setter(keep)
        for bad in (lo - 1, hi + 1):
            with pytest.raises(RuntimeError):
                setter(bad)
            assert h.knobs()[name] == keep           # a refused value changes nothing
    assert {k: v for k, v in h.knobs().items() if k != name} == others


def test_split_k_one_reads_back_zero():
    h.set_split_k(4)
    h.set_split_k(1)
    assert h.knobs()["split_k"] == 0


def test_reset_knobs_restores_all_ten():
    changed = {"gemm_tile": 5, "gemm_policy": 3, "split_k": -1, "w4_probe": 2, "w4_prio": 1, "wide_epilogue": 0,
               "xcd_blocks": 0, "lone_plain_order": 0, "xcd_group": 7, "triad_variant": 9}
    set_knobs(changed)
    assert h.knobs() == changed and len(changed) == 10
    h.reset_knobs()
    assert h.knobs() == h.knob_defaults()


def test_knobs_context_restores_every_knob():
    """The tests' knobs() context: whatever the block set, w4_probe included, is back at its default."""
    from test_gpu_kernels_exact import knobs
    with knobs(h, gemm_tile=14, w4_probe=2):
        assert h.knobs()["w4_probe"] == 2 and h.knobs()["gemm_tile"] == 14
        h.set_xcd_group(9)
    assert h.knobs() == h.knob_defaults()
    with pytest.raises(ZeroDivisionError):
        with knobs(h, w4_probe=3, triad_variant=2):
            1 / 0
    assert h.knobs() == h.knob_defaults()


# ------------------------------------------------------------------------------------------------
# literal rules of the launch: kernel, block, tile order, epilogue, order of resolution
# ------------------------------------------------------------------------------------------------
def whole_chip(budget):
    return budget <= 0 or budget >= 256


@pytest.mark.parametrize("xcd_blocks", [1, 0])
@pytest.mark.parametrize("lone_plain_order", [1, 0])
@pytest.mark.parametrize("budget", [0, 64, 256])
@pytest.mark.parametrize("tile", range(1, 17))
def test_forced_tile_kernel_block_order_and_epilogue(tile, budget, lone_plain_order, xcd_blocks):
    M, N, K = 2048, 2048, 128                                   # every tile divides it, two K-tiles
    set_knobs({"gemm_tile": tile, "lone_plain_order": lone_plain_order, "xcd_blocks": xcd_blocks})
    tm, tn = M // TILE_BM[tile], N // TILE_BN[tile]
    order = h.pick_xcd_map(tm, tn)
    # 8 XCDs as px x (8 / px) blocks: 2 x 4 on these grids, 4 x 2 on the 32 x 16 one (tiles 2, 7); 4 rows per group
    assert order == (0 if not xcd_blocks else (4 if (tm, tn) == (32, 16) else 2) | 4 << 8), (tm, tn)
    xmap = 0 if tile in LONE_PLAIN_TILES and lone_plain_order and whole_chip(budget) else order
    for relu, bias in ACTS:
        for aligned in (True, False):
            if tile in WIDE_ONLY_TILES and not aligned:
                with pytest.raises(RuntimeError):               # forced onto an unaligned C
                    plan(M, N, K, budget, relu, bias, aligned)
                continue
            wide = tile in WIDE_ONLY_TILES or (tile != 9 and aligned)
            assert plan(M, N, K, budget, relu, bias, aligned) == \
                (1, [(tile, tile_kernel(tile, relu, bias, wide), tm * tn, TILE_THREADS[tile], xmap, 0, M)])


def test_wide_epilogue_knob_off_is_an_unaligned_c():
    h.set_wide_epilogue(0)
    for tile in (1, 3, 10, 13):
        h.set_gemm_tile(tile)
        assert plan(1024, 1024, 128, 64)[1][0][1] == tile_kernel(tile, False, False, False)
    h.set_gemm_tile(14)
    with pytest.raises(RuntimeError):
        plan(1024, 1024, 128, 64)
    h.set_gemm_tile(0)                                          # policy 10 picks 14, which gives way to 10
    assert plan(1024, 1024, 128, 4)[1][0][:2] == (10, tile_kernel(10, False, False, False))


@pytest.mark.parametrize("tile", range(1, 17))
def test_resolution_small_k_then_divisibility(tile):
    """1. the forced tile, 2. small_k_fallback when K < 128, 3. tile 3 when the tile does not divide."""
    h.set_gemm_tile(tile)
    small = SMALL_K_FALLBACK.get(tile, tile)
    for aligned in (True, False):                               # a fallback is never wide-only: no raise
        if small == tile and tile in WIDE_ONLY_TILES:
            continue
        wide = aligned and small != 9
        assert plan(1024, 1024, 64, 64, True, False, aligned)[1] == \
            [(small, tile_kernel(small, True, False, wide), (1024 // TILE_BM[small]) * (1024 // TILE_BN[small]),
              TILE_THREADS[small], h.pick_xcd_map(1024 // TILE_BM[small], 1024 // TILE_BN[small]), 0, 1024)]
    # 192 x 320: only 64 x 64 divides it, at any K; the 4-wave tiles no longer raise on an unaligned C
    for K in (64, 128):
        assert plan(192, 320, K, 0, False, True, False)[1] == [(3, tile_kernel(3, False, True, False), 15, 256, 0, 0, 192)]
    # 384 x 384 at K = 64: tile 14 -> 4 (small K) -> 3 (256 does not divide), 16 -> 1 (divides)
    want = {14: 3, 16: 1}.get(tile)
    if want:
        assert plan(384, 384, 64, 0)[1][0][0] == want


@pytest.mark.parametrize("policy,M,N,tile", [(10, 1024, 1024, 14), (12, 512, 512, 14), (11, 512, 256, 15),
                                             (13, 256, 256, 16)])
def test_policy_four_wave_tile_gives_way_on_unaligned_c(policy, M, N, tile):
    """4. narrow_c_fallback, last: chosen by a policy (so at a share: never lone), a 4-wave tile on a C
    that is not 16-byte aligned runs its fallback's narrow kernel in the co-run tile order."""
    h.set_gemm_policy(policy)
    budget = 4
    assert h.pick_gemm_tile(M, N, budget) == tile
    grid = (M // TILE_BM[tile]) * (N // TILE_BN[tile])
    xmap = h.pick_xcd_map(M // TILE_BM[tile], N // TILE_BN[tile])
    assert plan(M, N, 128, budget, True, True, True)[1] == \
        [(tile, tile_kernel(tile, True, True, True), grid, 256, xmap, 0, M)]
    fb = NARROW_C_FALLBACK[tile]
    assert (TILE_BM[fb], TILE_BN[fb]) == (TILE_BM[tile], TILE_BN[tile])
    assert plan(M, N, 128, budget, True, True, False)[1] == \
        [(fb, tile_kernel(fb, True, True, False), grid, TILE_THREADS[fb], xmap, 0, M)]
    # below two K-tiles the small-K fallback comes first and has both epilogues
    sk = SMALL_K_FALLBACK[tile]
    assert plan(M, N, 64, budget, False, False, False)[1][0][:2] == (sk, tile_kernel(sk, False, False, False))


def test_tile14_priority_and_probe_kernels():
    h.set_gemm_tile(14)
    h.set_w4_prio(1)
    for relu, bias in ACTS:
        assert plan(512, 512, 128, 0, relu, bias)[1][0][1] == \
            f"gemm_bf16_nt_256_w4l<{flag(relu)}, {flag(bias)}, 0, true, 256, 256>"
    for probe in (1, 2, 3):                                     # a probe wins over priority, and has no epilogue flags
        h.set_w4_probe(probe)
        for relu, bias in ACTS:
            assert plan(512, 512, 128, 0, relu, bias)[1][0][1] == f"gemm_bf16_nt_256_w4l<false, false, {probe}, false, 256, 256>"
    for tile in (15, 16, 10):                                   # ... and both change tile 14 alone
        h.set_gemm_tile(tile)
        assert plan(512, 512, 128, 0, True, True)[1][0][1] == tile_kernel(tile, True, True, True)


def test_policy9_row_slices():
    """rows = max(1, cu_budget / (N / 256)) * 256 per launch once tile 10 has more tiles than the share;
    every part takes the tile order of its own rows."""
    h.set_gemm_policy(9)
    k10 = tile_kernel(10, True, False, True)

    def parts(M, N, budget):
        split, launches = plan(M, N, 128, budget, True, False)
        assert split == 1 and all(l[:2] == (10, k10) and l[3] == 512 for l in launches)
        assert [l[2] for l in launches] == [(l[6] // 256) * (N // 256) for l in launches]
        assert [l[4] for l in launches] == [h.pick_xcd_map(l[6] // 256, N // 256) for l in launches]
        return [(l[5], l[6]) for l in launches]

    assert parts(4096, 2560, 64) == [(0, 1536), (1536, 1536), (3072, 1024)]      # 64 / 10 = 6 tile rows
    assert parts(1024, 2560, 4) == [(0, 256), (256, 256), (512, 256), (768, 256)]  # 4 / 10 = 0 -> 1 tile row
    assert parts(1024, 512, 4) == [(0, 512), (512, 512)]
    assert parts(4096, 4096, 64) == [(0, 1024), (1024, 1024), (2048, 1024), (3072, 1024)]
    assert parts(2048, 2048, 64) == [(0, 2048)]                                   # 64 tiles fill the share: one launch
    assert plan(8192, 8192, 128, 0, True, False)[1] == [(10, k10, 1024, 512, 0, 0, 8192)]   # lone: never sliced
    # 1024 x 2560 at a 64-CU share has 40 tiles: too few for tile 10, the 128 x 128 tile in one launch
    assert plan(1024, 2560, 128, 64)[1] == [(1, tile_kernel(1, False, False, True), 160, 256,
                                             h.pick_xcd_map(8, 20), 0, 1024)]
    h.set_gemm_policy(1)
    assert parts(4096, 2560, 64) == [(0, 4096)]


def test_split_k_plan():
    """grid tiles x S of the split 8-phase kernel in the plain order, then splitk_reduce with
    min(ceil(M N / 4 / 256), 8192) blocks of 256."""
    split_kernel = "gemm_bf16_nt_256_8ph<false, false, true, false, true, 256>"
    h.set_split_k(-1)
    for relu, bias in ACTS:
        assert plan(256, 256, 2048, 0, relu, bias) == \
            (2, [(10, split_kernel, 2, 512, 0, 0, 256), (0, f"splitk_reduce<{flag(relu)}, {flag(bias)}>", 64, 256, 0, 0, 256)])
    assert plan(2048, 4096, 8192, 0)[1][1][2] == 8192
    assert h.gemm_plan(256, 256, 2048, 0, False, False, True, False)["split"] == 1       # no workspace, no split
    h.reset_knobs()
    h.set_gemm_policy(8)
    assert plan(1024, 2560, 2560, 64, True, True) == \
        (2, [(10, split_kernel, 80, 512, 0, 0, 1024), (0, "splitk_reduce<true, true>", 2560, 256, 0, 0, 1024)])


def test_plan_grid_equals_gemm_workgroups_over_the_picker_grid():
    import test_gemm_picker_golden as G

    def check(what):
        for M, N in G.shapes():
            for K in G.KS:
                for budget in G.BUDGETS:
                    for workspace in (False, True):
                        p = h.gemm_plan(M, N, K, budget, False, False, True, workspace)
                        blocks = sum(l["grid"] for l in p["launches"] if l["tile"])
                        assert blocks == h.gemm_workgroups(M, N, K, budget, False, workspace), (what, M, N, K, budget)
                        assert p["split"] == (h.pick_split_k(M, N, K, budget) if workspace else 1)

    for policy in G.POLICIES:
        h.set_gemm_policy(policy)
        for split_k in G.SPLIT_KNOBS if policy in (8, 10) else (0,):
            h.set_split_k(split_k)
            check(("policy", policy, split_k))
    h.reset_knobs()
    for tile in G.TILES:
        h.set_gemm_tile(tile)
        check(("tile", tile))


# ------------------------------------------------------------------------------------------------
# the kernel of every path, against the trace recorded at the parent
# ------------------------------------------------------------------------------------------------
def cases():
    """Every recorded case: the op, its arguments and the knobs set for it (all others at their defaults)."""
    out = []

    def gemm(M, N, K, budget=0, relu=False, bias=False, aligned=True, **knobs):
        out.append({"op": "gemm", "M": M, "N": N, "K": K, "budget": budget, "relu": relu, "bias": bias,
                    "aligned": aligned, "knobs": knobs})

    for tile in range(1, 17):
        for K in (64, 128):
            for aligned in (True, False):
                for relu, bias in ACTS:
                    gemm(256, 256, K, 0, relu, bias, aligned, gemm_tile=tile)
    for policy in range(14):
        for budget in (0, 64):
            for M, N in ((1024, 2048), (4096, 4096)):
                gemm(M, N, 128, budget, gemm_policy=policy)
    for relu, bias in ACTS:
        gemm(256, 256, 128, 0, relu, bias, gemm_tile=14, w4_prio=1)
    for probe in (1, 2, 3):
        gemm(256, 256, 128, 0, True, True, gemm_tile=14, w4_probe=probe)
    gemm(256, 256, 2048, 0, True, True, split_k=-1)
    gemm(1024, 2560, 2560, 64, True, False, gemm_policy=8)
    gemm(1024, 2560, 128, 64, gemm_policy=9)
    gemm(4096, 2560, 128, 64, gemm_policy=9)                    # this one is sliced: 160 tiles at a 64-CU share
    for M, N, budget in ((64, 64, 0), (2048, 4096, 64)):
        out.append({"op": "gemm_fp8", "M": M, "N": N, "K": 128, "budget": budget, "knobs": {}})
    for variant in range(11):
        out.append({"op": "triad", "n": 4096, "knobs": {"triad_variant": variant}})
    for mi in (8, 9, 32, 64):                                   # 3 x 32 MiB = 96 MiB exactly; past 96, 128, 256 MiB
        for variant in (6, 9, 10):
            out.append({"op": "triad", "n": mi << 20, "knobs": {"triad_variant": variant}})
    return out


def test_every_path_launches_the_kernel_recorded_at_the_parent():
    with open(GOLDEN) as f:
        recorded = json.load(f)
    mine = cases()
    assert [{k: v for k, v in c.items() if k not in ("launches", "raised")} for c in recorded] == mine
    seen = set()
    for c in recorded:
        if c["op"] != "gemm":
            continue
        h.reset_knobs()
        set_knobs(c["knobs"])
        args = (c["M"], c["N"], c["K"], c["budget"], c["relu"], c["bias"], c["aligned"])
        if c["raised"]:
            assert not c["launches"]
            with pytest.raises(RuntimeError):
                plan(*args)
            continue
        got = [list(l[1:4]) for l in plan(*args)[1]]
        assert got == c["launches"], (c, got)
        seen |= {l[0] for l in c["launches"]}
    # the recording reaches every kernel a tile can launch: 16 tiles x 4 acts x the epilogues each has
    for tile in range(1, 17):
        for relu, bias in ACTS:
            for wide in (True, False):
                if (wide and tile == 9) or (not wide and tile in WIDE_ONLY_TILES):
                    continue
                assert tile_kernel(tile, relu, bias, wide) in seen, (tile, relu, bias, wide)


def launch_all():
    """The program under the kernel trace: every case once on the current stream, uninitialised operands
    (only the launches matter), then the case's end mark."""
    import torch
    from k8s_gpu_scheduler_amd.ops import loadgen
    hip = _native.hip(required=True)
    defaults = (("gemm_tile", 0), ("gemm_policy", 10), ("split_k", 0), ("w4_probe", 0), ("w4_prio", 0),
                ("wide_epilogue", 1), ("xcd_blocks", 1), ("lone_plain_order", 1), ("xcd_group", 4), ("triad_variant", 6))
    mark = torch.empty(64, dtype=torch.int32, device="cuda")
    raised = []
    for c in cases():
        for name, value in defaults:
            getattr(hip, "set_" + name)(value)
        for name, value in c["knobs"].items():
            getattr(hip, "set_" + name)(value)
        if c["op"] == "triad":
            a, b, x = (torch.empty(c["n"], device="cuda") for _ in range(3))
            loadgen.triad(a, b, x, 1.5)
        else:
            M, N, K = c["M"], c["N"], c["K"]
            fp8 = c["op"] == "gemm_fp8"
            a = torch.empty(M, K, device="cuda", dtype=torch.uint8 if fp8 else torch.bfloat16)
            bt = torch.empty(N, K, device="cuda", dtype=torch.uint8 if fp8 else torch.bfloat16)
            if fp8:
                loadgen.gemm_fp8(a.view(loadgen.FP8), bt.view(loadgen.FP8), cu_budget=c["budget"])
            else:
                pad = 0 if c["aligned"] else 4
                out = torch.empty(M, N + pad, device="cuda", dtype=torch.bfloat16)[:, pad:]
                bias = torch.empty(N, device="cuda") if c["bias"] else None
                try:
                    loadgen.gemm(a, bt, out=out, bias=bias, relu=c["relu"], cu_budget=c["budget"])
                    raised.append(False)
                except RuntimeError as e:                       # a 4-wave tile forced onto an unaligned C
                    if "16-byte aligned" not in str(e):
                        raise RuntimeError(f"{c}: {e}") from e
                    raised.append(True)
        hip.xcd_probe(mark.data_ptr(), CASE_MARK, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    print("RAISED " + json.dumps(raised))


def record(path):
    """One kernel-trace-only profiler run of launch_all() in a fresh process; its launches per case."""
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable,
                            os.path.abspath(__file__), "--launch"], capture_output=True, text=True, timeout=300)
        if p.returncode != 0:
            sys.exit(f"the traced run failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        raised = json.loads([l for l in p.stdout.splitlines() if l.startswith("RAISED ")][-1][7:])
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(f, newline="") as fh:
                rows += [{k.lower(): v for k, v in r.items()} for r in csv.DictReader(fh)]
    rows.sort(key=lambda r: int(r["dispatch_id"]))
    per_case, cur = [], []
    for r in rows:
        name = kernel_id(r["kernel_name"])
        block = int(r["workgroup_size_x"])
        grid = int(r["grid_size_x"]) // block
        if "gs::" not in r["kernel_name"]:
            continue                                            # torch's own kernels
        if name == "xcd_probe_kernel" and grid == CASE_MARK:
            per_case.append(cur)
            cur = []
        else:
            cur.append([name, grid, block])
    mine = cases()
    assert len(per_case) == len(mine) and not cur, (len(per_case), len(mine), cur)
    assert len(raised) == sum(c["op"] == "gemm" for c in mine)
    raised = iter(raised)
    for c, launches in zip(mine, per_case):
        c["launches"] = launches
        if c["op"] == "gemm":
            c["raised"] = next(raised)
            assert c["raised"] == (not launches), c
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in mine) + "\n]\n")


if __name__ == "__main__":
    if sys.argv[1:] == ["--launch"]:
        launch_all()
    elif len(sys.argv) == 3 and sys.argv[1] == "--write":
        if h is None:
            sys.exit("HIP extension not built")
        record(sys.argv[2])
    else:
        sys.exit("usage: python tests/test_gemm_plan_cpu.py --write PATH")
