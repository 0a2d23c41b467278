// The 4-wave GEMM kernel with AGPR-tied inline-asm MFMAs (tiles 14-16): gemm_bf16_nt_256_w4l.
#pragma once
#include <type_traits>

#include "gemm_device.h"

namespace gs {

// Tile 14 (built for the lone-GEMM study; the co-run default since round 6,
// policy 10): the 256 x 256 block tile on FOUR waves of 128 x 128 -- hipBLASLt's shape
// (profiles/r05_lone_gemm_pmc/: 0.25 LDS reads per MFMA instead of the 8-phase kernel's 0.375).
// Tiles 15 / 16 are the same kernel on 256 x 128 / 128 x 128 blocks (A/B knobs).  Round 5's versions of this
// structure stalled once per K-tile (1,016 TF) or spilled: the compiler kept a VGPR copy of the
// 256 accumulators next to the AGPRs.  Here the MFMA is inline asm with the accumulator tied to
// an AGPR ("+a"), so the accumulators cannot leave the AGPR file.
__device__ __forceinline__ void mfma_agpr(f32x4& acc, const bf16x8& b, const bf16x8& a) {
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(b), "v"(a));
}

// The compiler cannot see that the asm above is an MFMA, so it cannot insert the wait states
// between an MFMA and a VALU access of its accumulator: these fences pin them.  An empty volatile
// asm that "modifies" every accumulator keeps the compiler's own accumulator accesses on their
// side of it (volatile asm statements keep their order).  agpr_after_init: after the accumulators'
// bias / zero fill, before the first MFMA; agpr_before_read: after the last MFMA, before the
// epilogue reads.
template <int NI, int NJ>
__device__ __forceinline__ void agpr_fence(f32x4 (&acc)[NI][NJ]) {
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) asm volatile("" : "+a"(acc[i][j]));
}
template <int NI, int NJ>
__device__ __forceinline__ void agpr_after_init(f32x4 (&acc)[NI][NJ]) {
  agpr_fence(acc);
  asm volatile("s_nop 7" ::: "memory");
}
template <int NI, int NJ>
__device__ __forceinline__ void agpr_before_read(f32x4 (&acc)[NI][NJ]) {
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");
  agpr_fence(acc);
}

// The schedule: 64-deep operand tiles in a 5-slot LDS ring.  Timing probes of a first version
// (32-deep sub-tiles in 4 slots, one barrier per 32 k; profiles/r06_lone_gemm/): its LDS-DMA cost
// the single wave per SIMD ~0.22 ms of 0.79 at 8192^3, and fetching 8 rows x 128 B per
// instruction (whole cache lines) instead of 16 rows x 64 B saved ~0.09 ms of that.  So the
// operand tiles here are BM / BN rows x 64 k (128-B rows, stage_tile's KT = 64 image and swizzle):
// A_t and B_t take ring slots (2t) % 5 and (2t+1) % 5 of the larger tile's size (256 x 256: 32 KiB
// each, 160 KiB = the CU's whole LDS; 128 x 128: 80 KiB, two blocks per CU).  K-tile t runs two
// halves of (BM / 32) x (BN / 32) MFMAs (64 at 256 x 256):
//   h0: MFMAs of k-step 0 (fragment set 0), reads of k-step 1 into set 1, glds of A_{t+2}
//       (into B_{t-1}'s slot);
//   lgkmcnt(0) + vmcnt (A_{t+1}, B_{t+1} landed; A_{t+2} may fly) + ONE barrier;
//   h1: MFMAs of k-step 1 (set 1), reads of K-tile t+1's k-step 0 into set 0, glds of B_{t+2}
//       (into A_t's slot).
// The barrier certifies for every wave that A_{t+1} / B_{t+1} landed (RAW for h1's reads) and
// that every read of A_t and B_{t-1} retired (WAR for the next two glds groups), so one barrier
// per 128 MFMAs suffices.
// PRIO (A/B arm, set_w4_prio): the waves run at s_setprio 1 from start to end, ahead of co-resident
// stream waves of other pods in the SIMD's issue arbitration.
template <bool RELU, bool BIAS, int PROBE = 0, bool PRIO = false, int BN = 256, int BM = 256>
__global__ void __launch_bounds__(256, BM == 128 ? 2 : 1)
gemm_bf16_nt_256_w4l(const __bf16* __restrict__ A, const __bf16* __restrict__ Bt, __bf16* __restrict__ C,
                     const float* __restrict__ bias, int M, int N, int K, int lda, int ldb, int ldc, int xmap) {
  static_assert((BM == 256 && (BN == 256 || BN == 128)) || (BM == 128 && BN == 128),
                "4-wave block tile is 256 x 256, 256 x 128 or 128 x 128");
  constexpr int KT = 64, NSLOT = 5;
  constexpr int SLOT = (BM > BN ? BM : BN) * KT * 2;  // one ring slot: the larger operand tile
  constexpr int GA = BM * KT * 2 / 16 / 256;       // glds per thread for an A tile (8 or 4)
  constexpr int GB = BN * KT * 2 / 16 / 256;       // ... for a B tile (8 or 4)
  constexpr int WM = BM / 2, WN = BN / 2;          // wave tile (2 x 2 waves)
  constexpr int NI = WM / 16, NJ = WN / 16;        // 16-row / 16-column fragments per wave
  constexpr int NG = NI * NJ / 4;                  // groups of 4 MFMAs per half
  __shared__ __attribute__((aligned(16))) char smem[NSLOT * SLOT];

  int tm, tn;
  tile_coords(blockIdx.x, gridDim.x, M / BM, N / BN, xmap, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int lane = threadIdx.x & (kWave - 1);
  const int wr = wave >> 1, wc = wave & 1;
  const int frow = lane & 15, fk = lane >> 4;

  // the accumulators start at the bias (D = C^T layout: 4 consecutive columns per lane), so the
  // epilogue holds no bias registers (at BN = 256 that kept the kernel at 148 VGPRs instead of 129)
  f32x4 acc[NI][NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    f32x4 b0 = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (BIAS) b0 = *reinterpret_cast<const f32x4*>(bias + n0 + wc * WN + j * 16 + fk * 4);
#pragma unroll
    for (int i = 0; i < NI; ++i) acc[i][j] = b0;
  }
  agpr_after_init(acc);
  if constexpr (PRIO) __builtin_amdgcn_s_setprio(1);
  // BN = 256: one A fragment set.  The MFMAs run row by row, so A fragment i is dead after row i
  // and the next k-step's fragment i is read into the same registers right behind it; B keeps two
  // sets.  96 fragment VGPRs instead of 128 put the kernel at 384 registers, so three 38-VGPR
  // stream waves of other pods fit beside each of its waves instead of two.
  constexpr bool SINGLE_A = NI == 8 && NJ == 8;
  bf16x8 fa[SINGLE_A ? 1 : 2][NI], fb[2][NJ];
  const int T = K / KT;                             // >= 2

  // piece q of operand tile X_u (B if isb): rows (q * 256 + wave * 64 + lane) >> 3, 8 per
  // instruction, by buffer_load ... lds through one descriptor per operand block: the per-thread
  // part is one 32-bit voffset per operand ((r >> 1) & 7 does not depend on q), the piece and
  // K-tile parts an SGPR soffset (the global_load_lds form with 64-bit per-lane addresses: within
  // 1-2 %, profiles/r06_lone_gemm/)
  const int rr = (wave * 64 + lane) >> 3, kq = ((wave * 64 + lane) & 7) ^ ((rr >> 1) & 7);
  const int voA = rr * lda * 2 + kq * 16, voB = rr * ldb * 2 + kq * 16;
  const auto rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(A + (size_t)m0 * lda), 0, BM * lda * 2, 0x00020000);
  const auto rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(Bt + (size_t)n0 * ldb), 0, BN * ldb * 2, 0x00020000);
  auto glds = [&](int u, bool isb, int q) {
    char* dst = smem + ((2 * u + (isb ? 1 : 0)) % NSLOT) * SLOT + (q * 256 + wave * 64) * 16;
    const int so = q * 32 * (isb ? ldb : lda) * 2 + u * KT * 2;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(isb ? rsB : rsA, (lptr_t)dst, 16, isb ? voB : voA, so, 0, 0);
  };
  auto slot = [&](int u, bool isb) -> const char* { return smem + ((2 * u + (isb ? 1 : 0)) % NSLOT) * SLOT; };

  // prologue: A_0 B_0 A_1 B_1 in flight; wait for A_0 / B_0; k-step 0 of K-tile 0 into set 0
#pragma unroll
  for (int u = 0; u < 2; ++u)
  {
#pragma unroll
    for (int q = 0; q < GA; ++q) glds(u, false, q);
#pragma unroll
    for (int q = 0; q < GB; ++q) glds(u, true, q);
  }
  wait_vmcnt<GA + GB>();
  barrier();
#pragma unroll
  for (int q = 0; q < NI; ++q) fa[0][q] = lds_frag<KT>(smem, wr * WM + q * 16 + frow, fk);
#pragma unroll
  for (int q = 0; q < NJ; ++q) fb[0][q] = lds_frag<KT>(smem + SLOT, wc * WN + q * 16 + frow, fk);

  // (Measured and removed: the four waves issuing their LDS-DMA pieces at different points -- in
  // pairs at groups w, w + 4, ... for wave w (1,277 vs 1,483 TF/s lone, -2.7 % pods/s) or the odd
  // waves in the odd groups (1,282 vs 1,493, -2.2 %); the waves' lockstep issue is the faster one,
  // profiles/r06_lone_gemm/stagger/, parity/.)
  // one half: 8 x NJ MFMAs on set S (k-step S of K-tile t) in NG groups of 4; the 8 + NJ reads of
  // (RU, k-step S^1) into set S^1 when RD, spread evenly (BN = 256: one per group); the glds of
  // operand tile (t+2, X = S) when ST, spread evenly (BN = 256: every second group; other
  // placements -- the glds in the odd groups, reads and glds in separate halves -- measured
  // 1-2 % slower, profiles/r06_lone_gemm/)
  auto half = [&](auto sc, auto rdc, auto stc, int t) {
    constexpr int S = decltype(sc)::value;
    constexpr bool RD = decltype(rdc)::value, ST = decltype(stc)::value;
    const int ru = S == 0 ? t : t + 1;             // h0 reads k-step 1 of t, h1 k-step 0 of t+1
    const char* ta = slot(ru, false);
    const char* tb = slot(ru, true);
    constexpr int NR = NI + NJ, NS = S == 0 ? GA : GB;
    constexpr int SA = SINGLE_A ? 0 : S;           // A set in use
#pragma unroll
    for (int g = 0; g < NG; ++g) {
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int i = (g * 4 + m) / NJ, j = (g * 4 + m) % NJ;
        mfma_agpr(acc[i][j], fb[S][j], fa[SA][i]);
      }
      if constexpr (RD && SINGLE_A) {              // row g/2 done: its next A fragment; B at even groups
        if (g & 1) fa[0][g >> 1] = lds_frag<KT>(ta, wr * WM + (g >> 1) * 16 + frow, (S ^ 1) * 4 + fk);
        else fb[S ^ 1][g >> 1] = lds_frag<KT>(tb, wc * WN + (g >> 1) * 16 + frow, (S ^ 1) * 4 + fk);
      } else if constexpr (RD) {
#pragma unroll
        for (int q = 0; q < NR; ++q) {
          if (q * NG / NR != g) continue;
          if (q < NI) fa[S ^ 1][q] = lds_frag<KT>(ta, wr * WM + q * 16 + frow, (S ^ 1) * 4 + fk);
          else fb[S ^ 1][q - NI] = lds_frag<KT>(tb, wc * WN + (q - NI) * 16 + frow, (S ^ 1) * 4 + fk);
        }
      }
      if constexpr (ST) {
#pragma unroll
        for (int p = 0; p < NS; ++p)
          if (p * NG / NS == g) glds(t + 2, S == 1, p);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  auto sync = [&](auto wc_) {
    __builtin_amdgcn_s_waitcnt(0xC07F);            // lgkmcnt(0): this wave's reads retired
    wait_vmcnt<decltype(wc_)::value>();
    barrier();
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using IG = std::integral_constant<int, GA>;      // A_{t+2} (staged in h0) may fly at the sync
  using Y = std::true_type;
  using F = std::false_type;
  // PROBE (timing study only): bit 0 drops the steady loop's glds, bit 1 its reads (wrong results)
  using SR = std::integral_constant<bool, !(PROBE & 2)>;
  using SS = std::integral_constant<bool, !(PROBE & 1)>;
  int t = 0;
  for (; t + 3 <= T; ++t) {                         // steady: stages A_{t+2}, B_{t+2}
    half(I0{}, SR{}, SS{}, t);
    sync(IG{});
    half(I1{}, SR{}, SS{}, t);
  }
  if (t + 2 == T) {                                 // K-tile T-2: nothing left to stage
    half(I0{}, Y{}, F{}, t);
    sync(I0{});
    half(I1{}, Y{}, F{}, t);
    ++t;
  }
  half(I0{}, Y{}, F{}, t);                          // K-tile T-1
  half(I1{}, F{}, F{}, t);
  agpr_before_read(acc);
  __builtin_amdgcn_s_waitcnt(0xC07F);
  barrier();

  // wide epilogue only (the host falls back to another kernel when C rows are not 16-B aligned)
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int col = wc * WN + j * 16 + fk * 4;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const f32x4 v = acc[i][j];
      bf16x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = act_bf16<RELU>(v[r]);
      wide_put<BN>(smem, wr * WM + i * 16 + frow, col, o);
    }
  }
  __syncthreads();
  wide_store<BM, BN, 256>(smem, C, ldc, m0, n0);
}

}  // namespace gs
