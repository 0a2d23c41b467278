// The 8-phase GEMM kernel (tiles 9, 10, 13 and the split-K slices): gemm_bf16_nt_256_8ph.
#pragma once
#include "gemm_device.h"

namespace gs {

// ---------------------------------------------------------------------------------------
// 256x256 "8-phase" GEMM for lone, large GEMMs (a whole-GPU Guaranteed pod): 8 waves as
// 2 (M) x 4 (N) groups, one block per CU, 128 KiB LDS = 2 K-tile buffers x {A0, A1, B0, B1}
// half-tiles of 128 rows x 64 k.  Wave (wr, wc) owns rows h*128 + wr*64 + [0, 64) and
// columns g*128 + wc*32 + [0, 32) for h, g in {0, 1}, so a (h, g) output quadrant touches
// only half-tiles A_h and B_g.  Each K-tile is 4 phases, each phase = its fragment reads,
// ONE half-tile of glds (2 x 16 B per thread), a barrier, 16 MFMAs, a barrier:
//
//   phase 1: quadrant (0,0)  reads A0 (8 x ds_read_b128) + B0 (4, kept in registers)
//   phase 2: quadrant (0,1)  reads B1 (4)
//   phase 3: quadrant (1,1)  reads A1 (8)
//   phase 4: quadrant (1,0)  no reads (A1 and B0 already in registers)
//
// Half-tile j (A0, B0, B1, A1 = 0..3) of K-tile u is staged in global phase 4u - 5 + j
// (K-tile u runs phases 4u+1 .. 4u+4; the prologue covers the phases <= 0), so every half-tile
// is restaged >= 2 phases after its last read of K-tile u-2 (WAR with the two wave groups
// staggered by one barrier) and is retired by a counted vmcnt at phase 2 or 4 at least one
// phase before its first read (RAW): three half-tiles stay in flight (vmcnt(6)) in steady
// state, fewer as the K loop drains.  The wr = 1 group runs one barrier behind the wr = 0
// group, so on every SIMD (one wave of each group) one wave issues its reads and glds
// while the other runs MFMAs.
__device__ __forceinline__ void wait_vmcnt_rt(int n) {
  // s_waitcnt takes an immediate: n (loads allowed in flight) is 0 .. 6
  if (n >= 6) wait_vmcnt<6>();
  else if (n == 5) wait_vmcnt<5>();
  else if (n == 4) wait_vmcnt<4>();
  else if (n == 3) wait_vmcnt<3>();
  else if (n == 2) wait_vmcnt<2>();
  else if (n == 1) wait_vmcnt<1>();
  else wait_vmcnt<0>();
}

// SPLIT (split-K for lone GEMMs with fewer 256x256 tiles than CUs, e.g. tall-K 2048x4096x8192):
// the grid is tiles x S; block (s, tile) multiplies the K slice [s*K, (s+1)*K) (K = the slice
// length here) and stores its fp32 partial tile to ws[s] (row-major, ld = N) instead of C;
// splitk_reduce then sums the S partials, adds bias, applies the activation and writes bf16.
//
// BN = 128: the same 8-phase schedule on a 256 x 128 block tile (tile 13) for the GEMMs of a
// co-running pod that are too small to give every CU of its share a 256 x 256 tile (the
// catalog's M = 1024 layers at a 64-CU share): B half-tiles are 64 rows (one glds per thread
// instead of two), each wave owns 128 x 32 outputs (one 16-column fragment per B half), and the
// counted waits follow the unequal half-tile sizes (inflight_8ph).  Half the blocks of the
// 128 x 128 tile, each staging 85 FLOP per byte instead of 64, with the two staggered wave groups
// of the 8-phase kernel instead of one lock-step group.
template <int BN>
struct Tile8ph {
  static constexpr int HALF_A = 128 * 64 * 2;          // bytes of an A half-tile image (128 rows x 64 k)
  static constexpr int HALF_B = (BN / 2) * 64 * 2;     // a B half-tile (BN/2 rows x 64 k)
  static constexpr int BUF = 2 * HALF_A + 2 * HALF_B;  // one K-tile: A0 A1 B0 B1
  static constexpr int OA0 = 0, OA1 = HALF_A, OB0 = 2 * HALF_A, OB1 = 2 * HALF_A + HALF_B;
  static constexpr int NJ = BN / 128;                  // 16-column fragments per wave per B half
  static constexpr int WCOLS = BN / 8;                 // columns per wave per B half
  static constexpr int GA = 2, GB = BN / 128;          // glds per thread for an A / B half-tile
};

// glds (per thread) allowed in flight at the counted wait of global phase p: those of phases
// p-2 .. p that exist (phase q stages half-tile j = (q + 5) mod 4 -- A0, B0, B1, A1 for j = 0..3
// -- and nothing after last_stage)
template <int BN>
__device__ __forceinline__ int inflight_8ph(int p, int last_stage) {
  int n = 0;
#pragma unroll
  for (int q = p - 2; q <= p; ++q) {
    if (q > last_stage) continue;
    const int j = ((q + 5) % 4 + 4) % 4;
    n += (j == 0 || j == 3) ? Tile8ph<BN>::GA : Tile8ph<BN>::GB;
  }
  return n;
}

template <bool RELU, bool BIAS, bool PEEL = false, bool WIDE = false, bool SPLIT = false, int BN = 256>
__global__ void __launch_bounds__(512, 1)
gemm_bf16_nt_256_8ph(const __bf16* __restrict__ A, const __bf16* __restrict__ Bt, __bf16* __restrict__ C,
                     const float* __restrict__ bias, int M, int N, int K, int lda, int ldb, int ldc, int xmap,
                     float* __restrict__ ws = nullptr) {
  static_assert(BN == 256 || BN == 128, "8-phase block tile is 256 x 256 or 256 x 128");
  using TL = Tile8ph<BN>;
  constexpr int BUF = TL::BUF;
  constexpr int OA0 = TL::OA0, OA1 = TL::OA1, OB0 = TL::OB0, OB1 = TL::OB1;
  constexpr int NJ = TL::NJ;
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];

  int nwg = gridDim.x;
  int b = blockIdx.x;
  int split = 0;
  if constexpr (SPLIT) {
    nwg = (M / 256) * (N / BN);                    // tiles; the S slices of one tile are nwg apart
    split = b / nwg;
    b -= split * nwg;
    A += (size_t)split * K;
    Bt += (size_t)split * K;
  }
  int tm, tn;
  tile_coords(b, nwg, M / 256, N / BN, xmap, tm, tn);
  const int m0 = tm * 256, n0 = tn * BN;

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int lane = threadIdx.x & (kWave - 1);
  const int wr = wave >> 2, wc = wave & 3;
  const int frow = lane & 15, fk = lane >> 4;

  f32x4 acc[2][4][2][NJ];                          // [h][mi][g][nj]
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[h][i][g][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 ar[2][4], b0r[2][NJ], b1r[2][NJ];          // [kk][mi], [kk][nj]

  const int T = K / 64;
  const int last_stage = 4 * T - 6;                // global phase of the last glds
  // half-tile j of K-tile u: A rows (j = 0, 3) or B rows (j = 1, 2)
  auto stage = [&](int u, int j) {
    char* dst = smem + (u & 1) * BUF + (j == 0 ? OA0 : j == 3 ? OA1 : j == 1 ? OB0 : OB1);
    if (j == 0 || j == 3)
      stage_tile<128, 512, 64>(A, lda, m0 + (j == 3 ? 128 : 0), u * 64, dst, wave, lane);
    else
      stage_tile<BN / 2, 512, 64>(Bt, ldb, n0 + (j == 2 ? BN / 2 : 0), u * 64, dst, wave, lane);
  };
  auto read_a = [&](const char* half) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i) ar[kk][i] = lds_frag<64>(half, wr * 64 + i * 16 + frow, kk * 4 + fk);
  };
  auto read_b = [&](const char* half, bf16x8 (&br)[2][NJ]) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int j = 0; j < NJ; ++j) br[kk][j] = lds_frag<64>(half, wc * TL::WCOLS + j * 16 + frow, kk * 4 + fk);
  };
  auto mfma_quadrant = [&](int h, int g, bf16x8 (&br)[2][NJ]) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[h][i][g][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(br[kk][j], ar[kk][i], acc[h][i][g][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };
  // loads allowed in flight at the wait of global phase p: the glds of phases p-2 .. p that
  // exist (BN = 256: 2 per phase; BN = 128: 2 for an A half, 1 for a B half)
  auto inflight = [&](int p) { return inflight_8ph<BN>(p, last_stage); };
  // steady state: phase 2 of a K-tile waits with B0, B1, A1 in flight; phase 4 with A1, A0, B0
  constexpr int STEADY2 = 2 * TL::GB + TL::GA;
  constexpr int STEADY4 = 2 * TL::GA + TL::GB;

  // prologue: K-tile 0 and half-tiles A0, B0 of K-tile 1 (phases -5 .. 0)
#pragma unroll
  for (int j = 0; j < 4; ++j) stage(0, j);
  stage(1, 0);
  stage(1, 1);
  wait_vmcnt<TL::GA + TL::GB>();                   // K-tile 0 landed; K-tile 1's A0/B0 in flight
  barrier();
  if (wr == 1) barrier();                          // group 1 runs one barrier behind

  int t0 = 0;
  if constexpr (PEEL) {
    // Steady state (t <= T-3): every phase stages its half-tile and three half-tiles stay in
    // flight, so the waits are constant counts and nothing branches -- the generic loop below
    // only runs the last two K-tiles, where the pipeline drains.
    for (; t0 + 2 < T; ++t0) {
      const char* cur = smem + (t0 & 1) * BUF;
      read_b(cur + OB0, b0r);
      __builtin_amdgcn_sched_barrier(0);
      read_a(cur + OA0);
      stage(t0 + 1, 2);
      barrier();
      mfma_quadrant(0, 0, b0r);
      barrier();
      read_b(cur + OB1, b1r);
      stage(t0 + 1, 3);
      wait_vmcnt<STEADY2>();
      barrier();
      mfma_quadrant(0, 1, b1r);
      barrier();
      read_a(cur + OA1);
      stage(t0 + 2, 0);
      barrier();
      mfma_quadrant(1, 1, b1r);
      barrier();
      stage(t0 + 2, 1);
      wait_vmcnt<STEADY4>();
      barrier();
      mfma_quadrant(1, 0, b0r);
      barrier();
    }
  }
  for (int t = t0; t < T; ++t) {
    const char* cur = smem + (t & 1) * BUF;
    const int p0 = 4 * t;
    // phase 1: (0,0)
    read_b(cur + OB0, b0r);
    __builtin_amdgcn_sched_barrier(0);
    read_a(cur + OA0);
    if (t + 1 < T) stage(t + 1, 2);
    barrier();
    mfma_quadrant(0, 0, b0r);
    barrier();
    // phase 2: (0,1)
    read_b(cur + OB1, b1r);
    if (t + 1 < T) stage(t + 1, 3);
    wait_vmcnt_rt(inflight(p0 + 2));
    barrier();
    mfma_quadrant(0, 1, b1r);
    barrier();
    // phase 3: (1,1)
    read_a(cur + OA1);
    if (t + 2 < T) stage(t + 2, 0);
    barrier();
    mfma_quadrant(1, 1, b1r);
    barrier();
    // phase 4: (1,0)
    if (t + 2 < T) stage(t + 2, 1);
    wait_vmcnt_rt(inflight(p0 + 4));
    barrier();
    mfma_quadrant(1, 0, b0r);
    barrier();
  }
  if (wr == 0) barrier();                          // balance the barrier count

  if constexpr (SPLIT) {
    // fp32 partial tile (D = C^T layout: 4 consecutive columns of one row per lane, 16-B stores)
    float* P = ws + (size_t)split * M * N;
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int col = n0 + g * (BN / 2) + wc * TL::WCOLS + j * 16 + fk * 4;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int row = m0 + h * 128 + wr * 64 + i * 16 + frow;
            *reinterpret_cast<f32x4*>(P + (size_t)row * N + col) = acc[h][i][g][j];
          }
      }
    return;
  }

  // Epilogue (D = C^T layout, as in gemm_bf16_nt_kernel: a lane holds 4 consecutive columns of one
  // row).  Narrow: 8-B stores straight to C, row / col are C's.  Wide (wide_put / wide_store): row /
  // col are the block tile's; the whole 256 x BN bf16 block tile is assembled in
  // LDS (at most the LDS the K loop used; every wave is past its last LDS read and every
  // LDS-DMA has retired -- the drained pipeline's vmcnt(0) -- once the now-aligned wave
  // groups meet at one more barrier), then whole rows go out with 16-B stores: coalesced
  // stores instead of scattered 8-B ones (the scattered tail cost 7-20 % of the 256 x 256
  // kernel at K = 8192 .. 2048).
  static_assert(256 * BN * 2 <= 2 * BUF, "wide epilogue image exceeds the staging LDS");
  if constexpr (WIDE) barrier();
  const int r0 = WIDE ? 0 : m0, c0 = WIDE ? 0 : n0;
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = c0 + g * (BN / 2) + wc * TL::WCOLS + j * 16 + fk * 4;
      f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
      if (BIAS) bv = *reinterpret_cast<const f32x4*>(bias + (n0 - c0) + col);
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = r0 + h * 128 + wr * 64 + i * 16 + frow;
          f32x4 v = acc[h][i][g][j] + bv;
          bf16x4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = act_bf16<RELU>(v[r]);
          if constexpr (WIDE) wide_put<BN>(smem, row, col, o);
          else *reinterpret_cast<bf16x4*>(C + (size_t)row * ldc + col) = o;
        }
    }
  if constexpr (WIDE) {
    __syncthreads();
    wide_store<256, BN, 512>(smem, C, ldc, m0, n0);
  }
}

}  // namespace gs
