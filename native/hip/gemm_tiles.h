// The compiler-scheduled GEMM kernels: gemm_bf16_nt_kernel (block tiles 64x64 .. 256x256, 2-4 LDS
// stages) and gemm_fp8_nt_kernel (the same loop on the block-scaled fp8 MFMA).
#pragma once
#include "gemm_device.h"

namespace gs {

// Block tile BM x BN, WGM x WGN waves, each wave (BM/WGM) x (BN/WGN) = MI x NJ MFMA 16x16
// tiles.  Register reuse (LDS read bytes per FLOP) is set by the WAVE tile and global->LDS
// traffic per FLOP by the BLOCK tile (the 256x256 variant, 8 waves of 128x64, moves ~40 %
// fewer LDS bytes per FLOP than 128x128).  Counters at 8192^3 (profiles/r01_gemm_pmc.json):
// no LDS bank conflicts, LDS array ~30 % busy, waves waiting ~26 % of their cycles -- the
// 2-stage loop is bound by the wait for the next tile, which STAGES >= 3 (counted vmcnt,
// raw s_barrier, glds issued two tiles ahead) attacks.  Small tiles exist so that the
// small-M GEMMs of the workload catalog still launch >= 256 workgroups (one per CU).
//
// The MFMA is issued with the B fragment as its first operand, so each lane's 4
// accumulator registers are 4 CONSECUTIVE output columns of one row (D = C^T layout:
// col = lane&15 -> m, row = (lane>>4)*4 + r -> n): the epilogue stores 8-byte packed bf16x4
// (4x fewer store instructions than one bf16 per register) and loads bias as float4.
template <int BM, int BN, int WGM, int WGN, int OCC, bool RELU, bool BIAS, int STAGES = 2, int KT = BK,
          bool HOIST = false, bool WIDE = false>
__global__ void __launch_bounds__(WGM * WGN * 64, OCC)
gemm_bf16_nt_kernel(const __bf16* __restrict__ A, const __bf16* __restrict__ Bt, __bf16* __restrict__ C,
                    const float* __restrict__ bias, int M, int N, int K, int lda, int ldb, int ldc, int xmap) {
  constexpr int NT = WGM * WGN * 64;
  static_assert(KT == 32 || KT == 64, "K tile");
  constexpr int A_BYTES = BM * KT * 2, B_BYTES = BN * KT * 2;
  constexpr int WTM = BM / WGM, WTN = BN / WGN;       // wave tile
  constexpr int MI = WTM / 16, NJ = WTN / 16;
  static_assert(BM * KT * 2 / 16 % NT == 0 && BN * KT * 2 / 16 % NT == 0, "stage split");
  static_assert(STAGES >= 2 && STAGES <= 4, "stages");
  constexpr int LOADS = (BM + BN) * KT * 2 / 16 / NT;    // glds per thread per K-tile
  __shared__ __attribute__((aligned(16))) char smem[STAGES * (A_BYTES + B_BYTES)];

  // ---- XCD-aware tile order (tile_coords) -------------------------------------------
  int tm, tn;
  tile_coords(blockIdx.x, gridDim.x, M / BM, N / BN, xmap, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int lane = threadIdx.x & (kWave - 1);
  const int wm = wave / WGN, wn = wave % WGN;

  f32x4 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto tileA = [&](int buf) { return smem + buf * (A_BYTES + B_BYTES); };
  auto tileB = [&](int buf) { return smem + buf * (A_BYTES + B_BYTES) + A_BYTES; };

  const int nt = K / KT;
  const int frow = lane & 15;
  const int fk = lane >> 4;
  auto compute = [&](const char* a_t, const char* b_t) {
    if constexpr (HOIST) {
      // every fragment of the K tile is read before the first MFMA: the MFMAs of k-step 0
      // wait only for their own reads (counted lgkmcnt), k-step 1's reads fly under them
      bf16x8 af[KT / 32][MI], bf[KT / 32][NJ];
#pragma unroll
      for (int kk = 0; kk < KT / 32; ++kk) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) bf[kk][j] = lds_frag<KT>(b_t, wn * WTN + j * 16 + frow, kk * 4 + fk);
#pragma unroll
        for (int i = 0; i < MI; ++i) af[kk][i] = lds_frag<KT>(a_t, wm * WTM + i * 16 + frow, kk * 4 + fk);
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int kk = 0; kk < KT / 32; ++kk)
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NJ; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[kk][j], af[kk][i], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      return;
    }
#pragma unroll
    for (int kk = 0; kk < KT / 32; ++kk) {
      bf16x8 af[MI], bf[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) bf[j] = lds_frag<KT>(b_t, wn * WTN + j * 16 + frow, kk * 4 + fk);
#pragma unroll
      for (int i = 0; i < MI; ++i) af[i] = lds_frag<KT>(a_t, wm * WTM + i * 16 + frow, kk * 4 + fk);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[j], af[i], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
  };
  auto stage = [&](int t, int buf) {
    stage_tile<BM, NT, KT>(A, lda, m0, t * KT, tileA(buf), wave, lane);
    stage_tile<BN, NT, KT>(Bt, ldb, n0, t * KT, tileB(buf), wave, lane);
  };

  if constexpr (STAGES == 2) {
    stage(0, 0);
    __syncthreads();
    int buf = 0;
    for (int t = 0; t < nt; ++t) {
      if (t + 1 < nt) stage(t + 1, buf ^ 1);   // issue tile t+1 before the MFMAs of tile t
      compute(tileA(buf), tileB(buf));
      __syncthreads();   // tile t+1 landed (vmcnt(0) before the barrier) and tile t fully read
      buf ^= 1;
    }
  } else {
    // Prologue: tiles 0 .. STAGES-2 in flight.  Iteration t: wait until only the tiles
    // after t are outstanding (counted vmcnt -- loads retire in order), barrier (every
    // thread's part of tile t landed AND every wave finished reading tile t-1, whose
    // buffer tile t+STAGES-1 reuses), issue tile t+STAGES-1, compute tile t.
#pragma unroll
    for (int p = 0; p < STAGES - 1; ++p)
      if (p < nt) stage(p, p);
    for (int t = 0; t < nt; ++t) {
      const int ahead = nt - 1 - t;             // tiles after t already issued (<= STAGES-2)
      if (ahead >= STAGES - 2) {
        wait_vmcnt<LOADS * (STAGES - 2)>();
      } else if (STAGES == 4 && ahead == 1) {
        wait_vmcnt<LOADS>();
      } else {
        wait_vmcnt<0>();
      }
      barrier();
      if (t + STAGES - 1 < nt) stage(t + STAGES - 1, (t + STAGES - 1) % STAGES);
      compute(tileA(t % STAGES), tileB(t % STAGES));
    }
  }

  // The two epilogue loops below (and the narrow one again in gemm_fp8_nt_kernel) stay written
  // out: as one loop with two destinations (gemm_bf16_nt_256_8ph's form) or as a shared function
  // template over acc[MI][NJ] they compiled to differently scheduled code here.
  if constexpr (WIDE) {
    static_assert(BM * BN * 2 <= STAGES * (A_BYTES + B_BYTES), "wide epilogue image exceeds the staging LDS");
    __syncthreads();                          // every wave past its last fragment read
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = wn * WTN + j * 16 + fk * 4;
      f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
      if (BIAS) bv = *reinterpret_cast<const f32x4*>(bias + n0 + col);
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        f32x4 v = acc[i][j] + bv;
        bf16x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = act_bf16<RELU>(v[r]);
        wide_put<BN>(smem, wm * WTM + i * 16 + frow, col, o);
      }
    }
    __syncthreads();
    wide_store<BM, BN, NT>(smem, C, ldc, m0, n0);
    return;
  }

  // ---- epilogue (D = C^T layout): row m = lane&15, cols n..n+3 = (lane>>4)*4 + r ----
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int col = n0 + wn * WTN + j * 16 + fk * 4;
    f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
    if (BIAS) bv = *reinterpret_cast<const f32x4*>(bias + col);
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int row = m0 + wm * WTM + i * 16 + frow;
      f32x4 v = acc[i][j] + bv;
      bf16x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = act_bf16<RELU>(v[r]);
      *reinterpret_cast<bf16x4*>(C + (size_t)row * ldc + col) = o;
    }
  }
}

// ---------------------------------------------------------------------------------------
// FP8 (OCP e4m3fn) GEMM: C[M,N] = act(A[M,K] . Bt[N,K]^T (+bias)), fp8 in / f32 accumulate /
// bf16 out, on the block-scaled MFMA v_mfma_scale_f32_16x16x128_f8f6f4 with unit scales
// (e8m0 127 = 2^0): twice the bf16 rate per clock (MI355X_MICROARCH.md "Matrix cores"),
// where the non-scaled 16x16x32 fp8 form only matches bf16.  A K tile is 128 fp8 = 128 B per
// row -- byte for byte the bf16 kernel's 64-deep tile -- so staging reuses stage_tile (the
// fp8 rows are moved as 16-byte chunks through a bf16 view with half the K) and the same
// XOR-swizzled, conflict-free LDS image.  One MFMA consumes a whole K tile: lane group
// fk = lane>>4 supplies 32 k values, read as the two 16-B chunks 2fk and 2fk+1 of its row.
// Which k a lane byte stands for does not matter as long as A and B agree (they are read
// with the same map), so no k permutation is needed.  Tile order (GROUP_M, xmap = 0) and
// epilogue as the bf16 kernel (D = C^T layout, packed bf16x4 stores, fused bias + ReLU).
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
constexpr int kUnitScale = 0x7F7F7F7F;   // e8m0 1.0 in every byte (any OPSEL picks 127)

__device__ __forceinline__ i32x8 lds_frag_fp8(const char* lds_tile, int row, int fk) {
  const i32x4 lo = __builtin_bit_cast(i32x4, lds_frag<BK>(lds_tile, row, 2 * fk));
  const i32x4 hi = __builtin_bit_cast(i32x4, lds_frag<BK>(lds_tile, row, 2 * fk + 1));
  return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

template <int BM, int BN, int WGM, int WGN, int OCC, bool RELU, bool BIAS>
__global__ void __launch_bounds__(WGM * WGN * 64, OCC)
gemm_fp8_nt_kernel(const uint8_t* __restrict__ A8, const uint8_t* __restrict__ B8, __bf16* __restrict__ C,
                   const float* __restrict__ bias, int M, int N, int K, int lda, int ldb, int ldc) {
  constexpr int NT = WGM * WGN * 64;
  constexpr int KT8 = 128;                             // fp8 elements (bytes) per K tile
  constexpr int A_BYTES = BM * KT8, B_BYTES = BN * KT8;
  constexpr int WTM = BM / WGM, WTN = BN / WGN;
  constexpr int MI = WTM / 16, NJ = WTN / 16;
  static_assert(A_BYTES / 16 % NT == 0 && B_BYTES / 16 % NT == 0, "stage split");
  __shared__ __attribute__((aligned(16))) char smem[2 * (A_BYTES + B_BYTES)];
  // bf16 views of the fp8 rows for the 16-byte glds staging (K and ld halved)
  const __bf16* A = reinterpret_cast<const __bf16*>(A8);
  const __bf16* Bt = reinterpret_cast<const __bf16*>(B8);
  const int lda2 = lda / 2, ldb2 = ldb / 2;

  int tm, tn;
  tile_coords(blockIdx.x, gridDim.x, M / BM, N / BN, 0, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int lane = threadIdx.x & (kWave - 1);
  const int wm = wave / WGN, wn = wave % WGN;
  f32x4 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto tileA = [&](int buf) { return smem + buf * (A_BYTES + B_BYTES); };
  auto tileB = [&](int buf) { return smem + buf * (A_BYTES + B_BYTES) + A_BYTES; };
  const int frow = lane & 15;
  const int fk = lane >> 4;
  auto stage = [&](int t, int buf) {
    stage_tile<BM, NT, BK>(A, lda2, m0, t * BK, tileA(buf), wave, lane);
    stage_tile<BN, NT, BK>(Bt, ldb2, n0, t * BK, tileB(buf), wave, lane);
  };
  auto compute = [&](const char* a_t, const char* b_t) {
    i32x8 af[MI], bf[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) bf[j] = lds_frag_fp8(b_t, wn * WTN + j * 16 + frow, fk);
#pragma unroll
    for (int i = 0; i < MI; ++i) af[i] = lds_frag_fp8(a_t, wm * WTM + i * 16 + frow, fk);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bf[j], af[i], acc[i][j], 0, 0, 0, kUnitScale,
                                                                      0, kUnitScale);
    __builtin_amdgcn_s_setprio(0);
  };
  const int nt = K / KT8;
  stage(0, 0);
  __syncthreads();
  int buf = 0;
  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) stage(t + 1, buf ^ 1);
    compute(tileA(buf), tileB(buf));
    __syncthreads();
    buf ^= 1;
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int col = n0 + wn * WTN + j * 16 + fk * 4;
    f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
    if (BIAS) bv = *reinterpret_cast<const f32x4*>(bias + col);
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int row = m0 + wm * WTM + i * 16 + frow;
      f32x4 v = acc[i][j] + bv;
      bf16x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = act_bf16<RELU>(v[r]);
      *reinterpret_cast<bf16x4*>(C + (size_t)row * ldc + col) = o;
    }
  }
}

}  // namespace gs
