// Load-generator GEMMs: the MFMA-bound work a scheduled pod performs on its XCDs.
//
// The reference has no GPU code; its pods are external MLPerf-style
// inference containers whose throughput the recommender matrices describe
// (pkg/recommender/recommender/configurations_train.ods).  The MI355X build needs real,
// controllable load on the chip to measure "achieved node GPU-util %" (BASELINE.json), so
// each synthetic workload is a mix of:
//
//  * gemm_bf16_nt -- C[M,N] = act(A[M,K] . Bt[N,K]^T (+bias)), bf16 in / f32 accumulate /
//    bf16 out, on MFMA (v_mfma_f32_16x16x32_bf16).  Block tiles 64x64 .. 256x256 (4 or 8
//    waves; 64x64 or 128x64 per wave) picked per shape; both operands staged global->LDS with 16-byte
//    global_load_lds (no VGPR round trip) into a double-buffered, XOR-swizzled LDS image
//    (bank-conflict-free ds_read_b128 fragment reads); stage of tile t+1 is issued before
//    the MFMAs of tile t; XCD-aware bijective block remap + XCD-block tile order for L2 reuse.
//    Epilogue fuses bias + ReLU and stores packed bf16x4.  Lone large GEMMs use a separate
//    256x256 "8-phase" kernel (gemm_bf16_nt_256_8ph: two staggered wave groups, one
//    half-tile of glds per phase, counted vmcnt).
//  * gemm_fp8_nt -- the same GEMM with OCP e4m3fn operands on the block-scaled
//    v_mfma_scale_f32_16x16x128_f8f6f4 (unit scales): 2x the bf16 MFMA rate.
//  * stream_triad (native/hip/triad.hip) -- the HBM-bound pod phase.
//
// The one translation unit with GEMM kernels: they live in gemm_tiles.h, gemm_8ph.h and gemm_w4.h
// (over gemm_device.h); here are the knobs, the tile table and picker, the planner (plan_gemm) and the
// one launcher that runs its plan.
//
// Launch settings (the knob table GS_KNOBS of api.h, values in knobs.cpp) are process-wide values read on the launching host
// thread when a kernel is enqueued (a captured HIP graph keeps the values of its capture).  One host thread per rank
// launches every pod kernel (parallel.executor), so they are plain statics; the defaults are
// the measured winners; every selectable variant computes the same result (GPU-tested against
// fp32 PyTorch), the rest of the A/B record lives in profiles/.
#include <algorithm>
#include <array>
#include <type_traits>

#include "api.h"
#include "common.h"
#include "gemm_8ph.h"
#include "gemm_tiles.h"
#include "gemm_w4.h"

namespace gs {

// XCC id of the executing workgroup (HW_REG_XCC_ID): tests/test_gpu_native.py reads it through
// xcd_probe to check the round-robin block -> XCD dispatch the tile order relies on.
__device__ __forceinline__ int xcc_id() { return __builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xF; }

__global__ void xcd_probe_kernel(int* out) {
  if (threadIdx.x == 0) out[blockIdx.x] = xcc_id();
}

// C[m, n..n+3] = act(sum_s ws[s][m, n..n+3] + bias) as bf16 -- the split-K epilogue (float4 in,
// bf16x4 out, grid-stride over M*N/4).
template <bool RELU, bool BIAS>
__global__ void __launch_bounds__(256) splitk_reduce(const float* __restrict__ ws, int S, int M, int N,
                                                     const float* __restrict__ bias, __bf16* __restrict__ C,
                                                     int ldc) {
  const size_t mn = (size_t)M * N, n4 = mn / 4;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += (size_t)gridDim.x * blockDim.x) {
    const size_t e = q * 4;
    f32x4 v = *reinterpret_cast<const f32x4*>(ws + e);
    for (int sp = 1; sp < S; ++sp) v += *reinterpret_cast<const f32x4*>(ws + (size_t)sp * mn + e);
    const int m = (int)(e / N), n = (int)(e % N);
    if (BIAS) v += *reinterpret_cast<const f32x4*>(bias + n);
    bf16x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = act_bf16<RELU>(v[r]);
    *reinterpret_cast<bf16x4*>(C + (size_t)m * ldc + n) = o;
  }
}

void xcd_probe(uintptr_t out, int blocks, uintptr_t stream) {
  hipLaunchKernelGGL(xcd_probe_kernel, dim3(blocks), dim3(64), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<int*>(out));
  HIP_CHECK(hipGetLastError());
}

// xcd_blocks: the XCD-block tile order (tile_coords): 1 = on (px chosen per grid), 0 = the GROUP_M order
// over the whole grid (A/B knob).  xcd_group: tile rows per group inside an XCD block.
// lone_plain_order: lone 8-phase / 4-wave GEMMs (whole-chip budget) in the plain GROUP_M order (1, default)
// or the same order as co-running pods (0, A/B knob).
//
// px (XCD-block rows, 8 / px columns) minimising the strips one XCD fetches, A rows + B
// columns of its block, among the splits that divide the grid; 0 = none (legacy order).
int pick_xcd_map(int tiles_m, int tiles_n) {
  if (!knob(k_xcd_blocks) || (tiles_m * tiles_n) % kXcds) return 0;
  int best = 0, best_cost = 1 << 30;
  for (int px = 1; px <= kXcds; px *= 2) {
    const int py = kXcds / px;
    if (tiles_m % px || tiles_n % py) continue;
    const int cost = tiles_m / px + tiles_n / py;
    if (cost < best_cost) best = px, best_cost = cost;
  }
  return best ? best | (knob(k_xcd_group) << 8) : 0;
}

// Wide (LDS-staged, 16-B row stores) epilogue whenever C rows are 16-B aligned; wide_epilogue = 0
// keeps the scattered 8-B epilogue (A/B knob).
static bool wide_ok(const __bf16* Cp, int ldc) {
  return knob(k_wide_epilogue) && ldc % 8 == 0 && reinterpret_cast<uintptr_t>(Cp) % 16 == 0;
}

// gemm_tile: 0 = auto (pick_gemm_tile), 1..16 = that row of kTiles for every GEMM (A/B knob).
//
// gemm_policy.  Lone GEMMs that still get one block per CU use the 8-phase 256x256 with the
// peeled steady-state loop (tile 10; tile 9 4096^3 1306 vs 1109 TF for tile 4, 8192^3 1434 vs
// 1211, profiles/r01_gemm_big.json; peeling: +5-6 % over tile 9 on every shape,
// profiles/r02_gemm_big_peeled.json).  1 = default: co-running pods whose CU share the 256x256
// tile fills use it too -- +3.2 % pods/s in the bench once the wide epilogue and the peeled loop
// landed and every pod stream got its own HW queue (interleaved A/B, profiles/r02_gemm_share_ab.txt;
// in round 1, with the older kernels, it had been even: profiles/r01_gemm_policy_ab.txt).
// 0 = co-running pods always take the 128x128 / 2-per-CU picker.  2 = tile 4 instead of tile
// 10 for lone GEMMs.
// Default 10 since round 6: arm 1's tiles, except co-running GEMMs the 256x256 tile fills run the
// 4-wave kernel (tile 14) -- 606.3 vs 596.4 pods/s, SLOs 61.8 vs 59.0 % over 5 interleaved bench
// rounds on MI355X (600.6 vs 587.1 over 3 on another box; profiles/r06_w4corun/).
//
// split_k: split-K for lone GEMMs whose 256x256 tiles leave CUs idle: -1 = auto (up to 8 slices), 0 = off,
// 2..8 = at most that many slices.  Off by default: on the tall-K 2048x4096x8192 the split
// kernel itself runs at ~1540 TF, but the fp32 partials + reduce pass (~144 MB of traffic) put
// the whole GEMM at 1162 TF vs 1210 for the 128x128 tile and 1290 for hipBLASLt
// (profiles/r02_gemm_big_splitk.json); a fused last-arriver fixup would need cross-XCD L2
// coherence for the partials.
//
// w4_prio, w4_probe: tile 14 with whole-kernel priority, and its timing probes (plan_gemm).

// The (relu, bias, wide) instantiations of one kernel, at index relu * 4 + bias * 2 + wide.  ACT_KERNELS(k<...>)
// names the kernel once, with R, B and W where its template takes the three flags.
using ActKernels = std::array<const void*, 8>;
template <class F>
static ActKernels act_kernels(F k) {
  using Y = std::true_type;
  using N = std::false_type;
  return {k(N{}, N{}, N{}), k(N{}, N{}, Y{}), k(N{}, Y{}, N{}), k(N{}, Y{}, Y{}),
          k(Y{}, N{}, N{}), k(Y{}, N{}, Y{}), k(Y{}, Y{}, N{}), k(Y{}, Y{}, Y{})};
}
#define ACT_KERNELS(...)                                                                            \
  act_kernels([](auto r, auto b, auto w) {                                                          \
    constexpr bool R = decltype(r)::value, B = decltype(b)::value, W = decltype(w)::value;          \
    return (void)W, reinterpret_cast<const void*>(&__VA_ARGS__);                                    \
  })

// The tile table, the whole description of a tile: block tile, threads per block, the tile that runs
// instead when the kernel's own limits rule it out (0 = no such limit): small_k_fallback below two K-tiles
// (K < 128: the 8-phase and 4-wave prologues stage two), narrow_c_fallback when C rows are not 16-B aligned
// and the tile has only the wide epilogue; the epilogues it has; whether a lone GEMM takes the plain tile
// order (plan_gemm); its kernels.  Any tile that does not divide the shape falls back to 3.
// models/workloads.py keeps a HIP-free copy of the rows the default policy uses.
enum Epilogues { NARROW, BOTH, WIDE };
struct TileInfo {
  int bm, bn, threads, small_k_fallback, narrow_c_fallback;
  Epilogues epi;
  bool lone_plain;
  ActKernels kernel;
};
// gemm_bf16_nt_kernel<BM, BN, WGM, WGN, OCC, R, B, STAGES, KT, HOIST, W>, gemm_bf16_nt_256_8ph<R, B, PEEL, W, SPLIT, BN>,
// gemm_bf16_nt_256_w4l<R, B, PROBE, PRIO, BN, BM>
static const TileInfo kTiles[17] = {
    {},  //  0 = auto
    //  1: 4 waves, 2 stages, 2 / CU, hoisted reads -- the small-GEMM winner (below)
    {128, 128, 256, 0, 0, BOTH, false, ACT_KERNELS(gemm_bf16_nt_kernel<128, 128, 2, 2, 2, R, B, 2, 64, true, W>)},
    //  2: 4 waves, 2 / CU, per-k-step reads (hoisting is mixed here)
    {64, 128, 256, 0, 0, BOTH, false, ACT_KERNELS(gemm_bf16_nt_kernel<64, 128, 2, 2, 2, R, B, 2, BK, false, W>)},
    //  3: 4 waves, 2 / CU, hoisted; always divides (the callers check % 64)
    {64, 64, 256, 0, 0, BOTH, false, ACT_KERNELS(gemm_bf16_nt_kernel<64, 64, 2, 2, 2, R, B, 2, 64, true, W>)},
    //  4: 8 waves of 128x64, 1 / CU, hoisted
    {256, 256, 512, 0, 0, BOTH, false, ACT_KERNELS(gemm_bf16_nt_kernel<256, 256, 2, 4, 1, R, B, 2, 64, true, W>)},
    //  5: 8 waves of 64x64, 1 / CU
    {256, 128, 512, 0, 0, BOTH, false, ACT_KERNELS(gemm_bf16_nt_kernel<256, 128, 4, 2, 1, R, B, 2, BK, false, W>)},
    //  6: tile 1 without hoisted reads (A/B reference)
    {128, 128, 256, 0, 0, BOTH, false, ACT_KERNELS(gemm_bf16_nt_kernel<128, 128, 2, 2, 2, R, B, 2, BK, false, W>)},
    //  7: tile 2 with 3 stages (2 / CU)
    {64, 128, 256, 0, 0, BOTH, false, ACT_KERNELS(gemm_bf16_nt_kernel<64, 128, 2, 2, 2, R, B, 3, BK, false, W>)},
    //  8: tile 5 with 3 stages
    {256, 128, 512, 0, 0, BOTH, false, ACT_KERNELS(gemm_bf16_nt_kernel<256, 128, 4, 2, 1, R, B, 3, BK, false, W>)},
    //  9: 8-phase (gemm_bf16_nt_256_8ph), the original loop; the 8-B epilogue only
    {256, 256, 512, 4, 0, NARROW, true, ACT_KERNELS(gemm_bf16_nt_256_8ph<R, B, false, W, false, 256>)},
    // 10: 8-phase, steady-state K loop peeled (constant vmcnt) + wide LDS-staged epilogue
    {256, 256, 512, 4, 0, BOTH, true, ACT_KERNELS(gemm_bf16_nt_256_8ph<R, B, true, W, false, 256>)},
    // 11: tile 1 with 3 LDS stages (counted vmcnt, glds issued 2 K-tiles ahead), 1 / CU
    {128, 128, 256, 0, 0, BOTH, false, ACT_KERNELS(gemm_bf16_nt_kernel<128, 128, 2, 2, 1, R, B, 3, 64, true, W>)},
    // 12: tile 1 with 4 LDS stages (3 K-tiles ahead), 1 / CU
    {128, 128, 256, 0, 0, BOTH, false, ACT_KERNELS(gemm_bf16_nt_kernel<128, 128, 2, 2, 1, R, B, 4, 64, true, W>)},
    // 13: tile 10's schedule on a 256 x 128 block tile
    {256, 128, 512, 5, 0, BOTH, true, ACT_KERNELS(gemm_bf16_nt_256_8ph<R, B, true, W, false, 128>)},
    // 14: 4 waves of 128x128 (gemm_bf16_nt_256_w4l); the co-run default (policy 10)
    {256, 256, 256, 4, 10, WIDE, true, ACT_KERNELS(gemm_bf16_nt_256_w4l<R, B, 0, false, 256, 256>)},
    // 15: the same kernel, wave tile 128x64 (policy 11)
    {256, 128, 256, 5, 13, WIDE, true, ACT_KERNELS(gemm_bf16_nt_256_w4l<R, B, 0, false, 128, 256>)},
    // 16: the same kernel, wave tile 64x64, 80 KiB ring, 2 / CU (policy 13)
    {128, 128, 256, 1, 1, WIDE, true, ACT_KERNELS(gemm_bf16_nt_256_w4l<R, B, 0, false, 128, 128>)},
};
// tile 14's other kernels: whole-kernel priority (w4_prio), and the timing probes w4_probe = 1..3: steady-loop
// LDS-DMA (1), reads (2) or both (3) dropped
static const ActKernels kW4Prio = ACT_KERNELS(gemm_bf16_nt_256_w4l<R, B, 0, true, 256, 256>);
static const void* const kW4Probe[3] = {reinterpret_cast<const void*>(&gemm_bf16_nt_256_w4l<false, false, 1>),
                                        reinterpret_cast<const void*>(&gemm_bf16_nt_256_w4l<false, false, 2>),
                                        reinterpret_cast<const void*>(&gemm_bf16_nt_256_w4l<false, false, 3>)};
// split-K: the 8-phase kernel writing fp32 partials of one K slice, then splitk_reduce<relu, bias>
static const void* const kSplitK = reinterpret_cast<const void*>(&gemm_bf16_nt_256_8ph<false, false, true, false, true>);
static const void* const kSplitKReduce[4] = {reinterpret_cast<const void*>(&splitk_reduce<false, false>),
                                             reinterpret_cast<const void*>(&splitk_reduce<false, true>),
                                             reinterpret_cast<const void*>(&splitk_reduce<true, false>),
                                             reinterpret_cast<const void*>(&splitk_reduce<true, true>)};
// 6-8 (profiles/r01_gemm_tiles.json): correct, but none beats 128x128 / 2 stages / 2 per CU
// (4096x2048x2048: 697 / 783 / 898 vs 954 TF; co-run mix 659 / 682 / 733 vs 795 TF): the extra
// stage costs the second resident block, which hid the tile wait just as well.
// 1, 3, 4 read all fragments of a K tile before its first MFMA (HOIST): +0-7 % over per-k-step reads on
// the catalog shapes, 4096^3 1105 vs 1047 TF; mixed for 64x128 (profiles/r01_gemm_tiles_hoist.json).
// 11 / 12: a co-running pod's small GEMM gets ~1 block per CU of its share, so its 4 waves (one per
// SIMD) must hide the MALL / HBM latency of the next tiles by depth, not by a second resident block.
// 14 began as the lone-GEMM study of profiles/r06_lone_gemm/ (level with tile 10).
// Measured and dropped:
//  * 128x128 with 2 waves of 128x64 and 128x256 with 4 waves of 64x128 -- fewer LDS bytes per FLOP, but
//    753 / 670 TF vs 783 TF for 128x128 on the co-run mix: profiles/r01_gemm_tiles_with_2wave_variants.json;
//  * 128x128 with a 32-deep K tile, 2 and 3 stages -- 4 / 3 blocks per CU, 687 / 704 TF on the co-run mix:
//    twice the barriers per FLOP cost more than the extra residency hides; profiles/r01_gemm_tiles_bk32.json;
//  * a 256x256 kernel with 4 waves of 128x128 wave tiles, 3-4 LDS stages -- slower than the 8-phase
//    kernel at every catalog shape, profiles/r02_gemm_4wave_study.json;
//  * tile 14's schedule on v_mfma_f32_32x32x16_bf16 -- half the MFMA instructions, exact, but 1,434 vs
//    1,483 TF/s at 8192^3, profiles/r06_lone_gemm/mfma32/; also there: 32-deep sub-tiles in 4 slots with
//    one barrier per 32 or per 64 k, and register-staged global loads -- 5-15 % behind.

// cu_budget = CUs a GEMM can expect to own: the whole chip for a lone kernel (0 or >= all CUs),
// the pod's CU share when pods run side by side
static bool whole_chip(int cu_budget) { return cu_budget <= 0 || cu_budget >= kCus; }

// BM x BN tiles divide the shape and give at least `need` workgroups
template <int BM, int BN>
static bool fills(int M, int N, int need) {
  return M % BM == 0 && N % BN == 0 && (M / BM) * (N / BN) >= need;
}

int pick_gemm_tile(int M, int N, int cu_budget) {
  if (knob(k_gemm_tile)) return knob(k_gemm_tile);
  // Measured (profiles/r01_gemm_tiles.json): a lone kernel wants >= 2 workgroups per CU of the
  // 64/128-wide tiles (fill beats per-block efficiency) and the 256x256 tile only when it
  // still fills every CU (4096^3: 1172 vs 1089 TF); co-running pods want the largest
  // tile that gives one workgroup per CU of their share -- the other pods' kernels fill
  // the rest of the chip -- 128x128 on the whole catalog mix: 784 vs 715 TF aggregate.
  const bool alone = whole_chip(cu_budget);
  const int budget = alone ? kCus : cu_budget;
  const int per_cu = alone ? 2 : 1;
  const int p = knob(k_gemm_policy);
  const bool fits256 = fills<256, 256>(M, N, budget);
  if (alone && fits256) return p == 2 ? 4 : 10;
  if (!alone) {                                    // the co-run arms: the ORDER of the rules is the policy
    // 10 (A/B arm, round 6): such co-running GEMMs on the 4-wave kernel (tile 14) -- one wave per
    // SIMD at 416 registers and no LDS left over, so up to three 32-VGPR stream waves of the other
    // pods fit on each of its SIMDs, where the 8-phase kernel's two 240-register waves leave room
    // for one
    if (fits256 && (p == 10 || p == 11 || p == 13)) return 14;
    // 12 (A/B arm): every co-running GEMM the 256 x 256 tile divides on the 4-wave kernel, even with
    // fewer tiles than its share's CUs (the other pods' stream waves take the rest)
    if (p == 12 && M % 256 == 0 && N % 256 == 0) return 14;
    // 11 (A/B arm): arm 10, and a co-running GEMM too small for that but filling its share with
    // 256 x 128 blocks on the same 4-wave kernel (tile 15) instead of the 128 x 128 tile
    if (p == 11 && fills<256, 128>(M, N, budget)) return 15;
    if (fits256 && p >= 1) return 10;
    // 3 / 4 (A/B arms): a co-running GEMM too small for one 256x256 tile per CU of its share
    // takes 256x128 (8 waves, 2 / 3 LDS stages) when that still gives every CU of the share a
    // block -- twice the arithmetic intensity per staged byte of 128x128 (85 vs 64 FLOP/B)
    // (exactly 3 / 4: arms 5-7 below are other tiles, and a `>= 3` test here used to shadow them)
    if ((p == 3 || p == 4) && fills<256, 128>(M, N, budget)) return p == 3 ? 5 : 8;
    // 7: the co-running small GEMM on the 256x128 8-phase kernel when that gives every CU of the
    // share a block
    if (p == 7 && fills<256, 128>(M, N, budget)) return 13;
    // 5 / 6 (A/B arms): the co-running small GEMM's 128x128 tile with 3 / 4 LDS stages
    if ((p == 5 || p == 6) && fills<128, 128>(M, N, budget)) return p == 5 ? 11 : 12;
    // 13 (A/B arm): arm 10, and the co-running GEMMs the 128 x 128 tile fills on the 4-wave kernel
    // at 128 x 128 (tile 16) instead of the compiler-scheduled tile 1
    if (p == 13 && (M / 128) * (N / 128) >= budget) return 16;
  }
  if ((M / 128) * (N / 128) >= per_cu * budget) return 1;
  if ((M / 64) * (N / 128) >= per_cu * budget && N % 128 == 0) return 2;
  return 3;
}

// Split-K factor for a lone GEMM (cu_budget 0 / whole chip): the 8-phase 256x256 kernel with
// S K-slices when its tiles leave CUs idle -- tiles x S <= CUs, every slice >= 1024 deep and a
// multiple of 64 -- else 1.  Needs an fp32 workspace of S*M*N floats (splitk_workspace_floats).
int pick_split_k(int M, int N, int K, int cu_budget) {
  if (knob(k_gemm_tile)) return 1;
  const bool alone = whole_chip(cu_budget);
  // policy 8 (A/B arm): a co-running pod's GEMM with fewer 256 x 256 tiles
  // than CUs in its share runs the 8-phase kernel split S ways along K (S = tiles needed to
  // cover the share, at most 4, every slice >= 512 deep), fp32 partials reduced by
  // splitk_reduce, instead of the 128 x 128 tile
  if (!alone && knob(k_gemm_policy) == 8) {
    if (M % 256 || N % 256) return 1;
    const int tiles = (M / 256) * (N / 256);
    if (tiles >= cu_budget) return 1;
    int S = std::min(4, (cu_budget + tiles - 1) / tiles);
    while (S > 1 && (K % (64 * S) != 0 || K / S < 512)) --S;
    return S;
  }
  if (knob(k_split_k) == 0) return 1;
  if (!alone) return 1;
  if (M % 256 || N % 256) return 1;
  const int tiles = (M / 256) * (N / 256);
  if (tiles * 2 > kCus) return 1;
  int S = std::min(knob(k_split_k) > 0 ? knob(k_split_k) : 8, kCus / tiles);
  while (S > 1 && (K % (64 * S) != 0 || K / S < 1024)) --S;
  return S;
}

size_t splitk_workspace_floats(int M, int N, int K, int cu_budget) {
  const int S = pick_split_k(M, N, K, cu_budget);
  return S > 1 ? (size_t)S * M * N : 0;
}

// the tile gemm_bf16_nt launches for this shape (pick_gemm_tile + the kernels' shape limits)
static int resolve_gemm_tile(int M, int N, int K, int cu_budget) {
  int t = pick_gemm_tile(M, N, cu_budget);
  if (K < 128 && kTiles[t].small_k_fallback) t = kTiles[t].small_k_fallback;
  if (M % kTiles[t].bm || N % kTiles[t].bn) t = 3;   // 64x64 always divides (checked by the caller)
  return t;
}

// fp8 fill rule, as the bf16 picker: 128x128 when it gives every CU of the budget a block (two
// for a lone kernel), else 64x64
bool fp8_tile_128(int M, int N, int cu_budget) {
  return fills<128, 128>(M, N, whole_chip(cu_budget) ? 2 * kCus : cu_budget);
}

static void check_shape(int M, int N, int K, const char* who) {
  if (M <= 0 || N <= 0 || K <= 0 || M % 64 || N % 64) throw std::runtime_error(std::string(who) + ": bad shape");
}

// Every decision of a bf16 GEMM launch, on the host alone.  Order: forced tile or policy, small_k_fallback,
// tile 3 when the tile does not divide the shape (resolve_gemm_tile), then narrow_c_fallback.
GemmPlan plan_gemm(int M, int N, int K, int cu_budget, bool relu, bool bias, bool wide_ok, bool workspace) {
  check_shape(M, N, K, "plan_gemm");
  const int act = relu * 4 + bias * 2;
  GemmPlan p;
  p.split = workspace ? pick_split_k(M, N, K, cu_budget) : 1;
  if (p.split > 1) {
    const size_t n4 = (size_t)M * N / 4;
    p.launches = {{10, kSplitK, (M / 256) * (N / 256) * p.split, 512, 0, 0, M},
                  {0, kSplitKReduce[act / 2], (int)std::min<size_t>((n4 + 255) / 256, 8192), 256, 0, 0, M}};
    return p;
  }
  int t = resolve_gemm_tile(M, N, K, cu_budget);
  if (kTiles[t].epi == WIDE && !wide_ok) {
    if (knob(k_gemm_tile) == t) throw std::runtime_error("gemm tiles 14-16: C rows must be 16-byte aligned");
    // a policy on an unaligned C (only co-running GEMMs get these tiles unforced, so `lone` is false)
    t = kTiles[t].narrow_c_fallback;
  }
  const TileInfo& ti = kTiles[t];
  const void* kernel = ti.kernel[act + (ti.epi == WIDE || (ti.epi == BOTH && wide_ok))];
  if (t == 14 && knob(k_w4_prio)) kernel = kW4Prio[act + 1];
  if (t == 14 && knob(k_w4_probe)) kernel = kW4Probe[knob(k_w4_probe) - 1];
  // a lone GEMM (the whole chip) takes the plain GROUP_M order: 0.936 vs 0.913 of hipBLASLt at
  // 4096^3, 0.94 vs 0.916 at 4096x8192x4096, 0.935 vs 0.918 at 8192^2x2048, 0.914 vs 0.92 at 8192^3
  // (7 interleaved rounds, profiles/r04_gemm_xcd/); co-running pods keep the XCD-block order
  // (+2.6 % bench pods/s, profiles/r02_xcd_block_order_ab.txt)
  const bool lone = ti.lone_plain && knob(k_lone_plain_order) && whole_chip(cu_budget);
  // policy 9 (A/B arm, round 6): a co-running pod's 8-phase GEMM with more 256 x 256 tiles than
  // its CU share runs as back-to-back launches of whole tile rows of at most `cu_budget` tiles
  // each, so it never holds more CUs than its share and the other pods' stream kernels keep
  // the rest of the chip (profiles/r06_gap/: GEMM time not hidden under the streams is the
  // largest term of the step)
  int rows = M;
  if (t == 10 && !whole_chip(cu_budget) && knob(k_gemm_policy) == 9 && (M / 256) * (N / 256) > cu_budget)
    rows = std::max(1, cu_budget / (N / 256)) * 256;
  for (int m0 = 0; m0 < M; m0 += rows) {
    const int m = std::min(rows, M - m0);
    p.launches.push_back({t, kernel, (m / ti.bm) * (N / ti.bn), ti.threads,
                          lone ? 0 : pick_xcd_map(m / ti.bm, N / ti.bn), m0, m});
  }
  return p;
}

int gemm_workgroups(int M, int N, int K, int cu_budget, bool fp8, bool split_workspace) {
  check_shape(M, N, K, "gemm_workgroups");
  if (fp8) return fp8_tile_128(M, N, cu_budget) ? (M / 128) * (N / 128) : (M / 64) * (N / 64);
  const GemmPlan p = plan_gemm(M, N, K, cu_budget, false, false, true, split_workspace);
  int blocks = 0;
  for (const GemmLaunch& l : p.launches) blocks += l.tile ? l.grid : 0;   // tile 0 = splitk_reduce
  return blocks;
}

// relu / bias as compile-time flags: f(std::bool_constant<RELU>{}, std::bool_constant<BIAS>{})
template <class F>
static void with_act(bool relu, const float* bias, F&& f) {
  if (relu && bias) f(std::true_type{}, std::true_type{});
  else if (relu) f(std::true_type{}, std::false_type{});
  else if (bias) f(std::false_type{}, std::true_type{});
  else f(std::false_type{}, std::false_type{});
}

// one GEMM call as the launchers pass it on (T = the operands' element type)
template <class T>
struct GemmArgsT {
  const T *A, *B;
  __bf16* C;
  const float* bias;
  int M, N, K, lda, ldb, ldc;
  bool relu;
  hipStream_t s;
};
using GemmArgs = GemmArgsT<__bf16>;

// One planned launch, rows [m0, m0 + m) of the call.  The three kernel families take the same eleven
// leading arguments; the 8-phase kernel's twelfth, ws, is nullptr outside split-K, and the runtime reads
// only as many as the kernel declares.
static void launch_tile(const GemmLaunch& l, GemmArgs g, float* ws = nullptr) {
  g.A += (size_t)l.m0 * g.lda;
  g.C += (size_t)l.m0 * g.ldc;
  g.M = l.m;
  int xmap = l.xmap;
  void* args[] = {&g.A, &g.B, &g.C, &g.bias, &g.M, &g.N, &g.K, &g.lda, &g.ldb, &g.ldc, &xmap, &ws};
  HIP_CHECK(hipLaunchKernel(l.kernel, dim3(l.grid), dim3(l.block), args, 0, g.s));
}

// Host-side argument checks of both entry points: the kernels have no bounds checks by design.
static void check_gemm_args(const std::string& prefix, uintptr_t a, uintptr_t bt, uintptr_t c, uintptr_t bias, int M,
                            int N, int K, int lda, int ldb, int ldc, int k_multiple, int ld_multiple) {
  if (M <= 0 || N <= 0 || K <= 0) throw std::runtime_error(prefix + ": empty shape");
  if (M % 64 || N % 64 || K % k_multiple)
    throw std::runtime_error(prefix + ": M,N must be multiples of 64 and K of " + std::to_string(k_multiple));
  if (lda < K || ldb < K || ldc < N || lda % ld_multiple || ldb % ld_multiple)
    throw std::runtime_error(prefix + ": bad leading dims");
  check_align(reinterpret_cast<void*>(a), "A");
  check_align(reinterpret_cast<void*>(bt), "Bt");
  if (ldc % 4 || c % 8) throw std::runtime_error(prefix + ": C rows must be 8-byte aligned");
  if (bias) check_align(reinterpret_cast<void*>(bias), "bias");
}

void gemm_bf16_nt(uintptr_t a, uintptr_t bt, uintptr_t c, uintptr_t bias, int M, int N, int K, int lda, int ldb,
                  int ldc, bool relu, uintptr_t stream, int cu_budget, uintptr_t workspace, size_t workspace_floats) {
  check_gemm_args("gemm", a, bt, c, bias, M, N, K, lda, ldb, ldc, BK, 8);
  const GemmArgs g{reinterpret_cast<const __bf16*>(a), reinterpret_cast<const __bf16*>(bt), reinterpret_cast<__bf16*>(c),
                   reinterpret_cast<const float*>(bias), M, N, K, lda, ldb, ldc, relu, reinterpret_cast<hipStream_t>(stream)};
  const GemmPlan p = plan_gemm(M, N, K, cu_budget, relu, bias != 0, wide_ok(g.C, ldc), workspace != 0);
  if (p.split > 1) {   // the K slices' fp32 partials, then their reduction
    int S = p.split;
    if (workspace_floats < (size_t)S * M * N) throw std::runtime_error("gemm: split-K workspace too small");
    check_align(reinterpret_cast<void*>(workspace), "workspace");
    float* ws = reinterpret_cast<float*>(workspace);
    GemmArgs slice = g;
    slice.K = K / S;
    launch_tile(p.launches[0], slice, ws);
    const GemmLaunch& r = p.launches[1];
    void* args[] = {&ws, &S, &M, &N, &slice.bias, &slice.C, &ldc};
    HIP_CHECK(hipLaunchKernel(r.kernel, dim3(r.grid), dim3(r.block), args, 0, g.s));
    return;
  }
  if (p.launches[0].tile >= 14 && (size_t)256 * std::max(lda, ldb) * 2 >= ((size_t)1 << 31))
    throw std::runtime_error("gemm tiles 14-16: a 256-row operand block must span < 2 GiB");
  for (const GemmLaunch& l : p.launches) launch_tile(l, g);
}

template <int BM, int BN, int WGM, int WGN, int OCC>
static void launch_gemm_fp8(const GemmArgsT<uint8_t>& g) {
  const dim3 grid((g.M / BM) * (g.N / BN)), block(WGM * WGN * 64);
  with_act(g.relu, g.bias, [&](auto r, auto b) {
    hipLaunchKernelGGL((gemm_fp8_nt_kernel<BM, BN, WGM, WGN, OCC, decltype(r)::value, decltype(b)::value>), grid, block,
                       0, g.s, g.A, g.B, g.C, g.bias, g.M, g.N, g.K, g.lda, g.ldb, g.ldc);
  });
}

void gemm_fp8_nt(uintptr_t a, uintptr_t bt, uintptr_t c, uintptr_t bias, int M, int N, int K, int lda, int ldb,
                 int ldc, bool relu, uintptr_t stream, int cu_budget) {
  check_gemm_args("gemm_fp8", a, bt, c, bias, M, N, K, lda, ldb, ldc, 128, 16);
  const GemmArgsT<uint8_t> g{reinterpret_cast<const uint8_t*>(a), reinterpret_cast<const uint8_t*>(bt), reinterpret_cast<__bf16*>(c),
                             reinterpret_cast<const float*>(bias), M, N, K, lda, ldb, ldc, relu, reinterpret_cast<hipStream_t>(stream)};
  if (fp8_tile_128(M, N, cu_budget)) launch_gemm_fp8<128, 128, 2, 2, 2>(g);
  else launch_gemm_fp8<64, 64, 2, 2, 2>(g);
  HIP_CHECK(hipGetLastError());
}

}  // namespace gs
