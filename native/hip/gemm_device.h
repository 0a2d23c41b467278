// Device-side pieces shared by every GEMM kernel of gemm.hip (gemm_tiles.h, gemm_8ph.h, gemm_w4.h):
// the XCD-aware tile order, the global -> LDS staging and its swizzled fragment reads, counted
// vmcnt waits, the fenced barrier, the activation and the LDS-staged wide epilogue.
#pragma once
#include "common.h"

namespace gs {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int BK = 64;
constexpr int GROUP_M = 8;

// Block index -> output tile.  Workgroups b and b + 8 run on the same XCD (round-robin dispatch;
// which XCD takes block 0 rotates with earlier dispatches -- tests/test_gpu_native.py reads
// HW_REG_XCC_ID), so the XCD-aware bijective remap first makes each XCD's workgroups one
// contiguous range of wgid.
// xmap = 0: GROUP_M-row grouped order over the whole grid (an XCD's range is a tall 8-row
// strip of tiles).  xmap = px | (gm << 8): the tile grid is cut into px x (8 / px) equal
// rectangles, XCD x walks rectangle x (gm-row grouped order inside), so the A row-strips and B column-strips
// one XCD's L2 has to fetch are those of a near-square block: on the co-run catalog shapes
// 18-33 % fewer strips per XCD than the tall strip (pick_xcd_map; the host only passes px when
// both dimensions divide and the grid is a multiple of 8).
__device__ __forceinline__ void tile_coords(int b, int nwg, int tiles_m, int tiles_n, int xmap, int& tm, int& tn) {
  const int xcd = b % kXcds;
  const int q = nwg / kXcds, rem = nwg % kXcds;
  const int wgid = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + b / kXcds;
  if (xmap & 0xFF) {
    const int px = xmap & 0xFF, GM = (xmap >> 8) & 0xFF;     // bands, rows per group inside the block
    const int py = kXcds / px;
    const int bm = tiles_m / px, bn = tiles_n / py;
    const int per = bm * bn;
    const int x = wgid / per, l = wgid - x * per;
    const int per_group = GM * bn;
    const int g = l / per_group;
    const int gsize = min(bm - g * GM, GM);
    const int r = l - g * per_group;
    tm = (x / py) * bm + g * GM + r % gsize;
    tn = (x % py) * bn + r / gsize;
    return;
  }
  const int per_group = GROUP_M * tiles_n;
  const int group = wgid / per_group;
  const int first_m = group * GROUP_M;
  const int gsize = min(tiles_m - first_m, GROUP_M);
  tm = first_m + (wgid % per_group) % gsize;
  tn = (wgid % per_group) / gsize;
}

typedef const void __attribute__((address_space(1)))* gptr_t;
typedef void __attribute__((address_space(3)))* lptr_t;

// Issue the glds for one ROWS x KT bf16 tile (rows [r0, r0+ROWS), k [k0, k0+KT)) of a
// row-major matrix with leading dimension ld (elements).  A row is KT*2 bytes = KT/8 16-byte
// chunks; logical chunk kc of row r lands at physical chunk kc ^ ((r >> 1) & (KT/8 - 1)).
// The LDS image itself is lane-linear (glds requirement), so the swizzle is applied on the
// per-lane SOURCE address (rule: linear dest + permuted source + same permutation on read).
// For KT = 64 (128-B rows) and KT = 32 (64-B rows) this makes every 16-lane group of a
// ds_read_b128 fragment read (rows r..r+15, one logical chunk) hit 16 distinct 16-B bank
// slots: conflict-free (checked against the gfx950 ds_read_b128 lane groups; PMC
// SQ_LDS_BANK_CONFLICT = 0, profiles/r01_gemm_pmc.json).
template <int ROWS, int NT, int KT = BK>
__device__ __forceinline__ void stage_tile(const __bf16* __restrict__ g, int ld, int r0, int k0,
                                           char* lds_tile, int wave, int lane) {
  constexpr int CH = KT / 8;          // 16-byte chunks per row
  constexpr int SH = CH == 8 ? 3 : 2;
#pragma unroll
  for (int i = 0; i < ROWS * KT * 2 / 16 / NT; ++i) {
    const int chunk = i * NT + wave * 64 + lane;
    const int r = chunk >> SH;
    const int p = chunk & (CH - 1);
    const int kc = p ^ ((r >> 1) & (CH - 1));
    const __bf16* src = g + (size_t)(r0 + r) * ld + k0 + kc * 8;
    char* dst = lds_tile + (i * NT + wave * 64) * 16;  // wave-uniform base
    __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)dst, 16, 0, 0);
  }
}

template <int KT = BK>
__device__ __forceinline__ bf16x8 lds_frag(const char* lds_tile, int row, int kchunk) {
  const int phys = kchunk ^ ((row >> 1) & (KT / 8 - 1));
  return *reinterpret_cast<const bf16x8*>(lds_tile + row * (KT * 2) + phys * 16);
}

// s_waitcnt with only the vmcnt field constrained (expcnt = 7, lgkmcnt = 15 = no wait);
// gfx9 encoding: vmcnt[3:0] -> bits 3:0, vmcnt[5:4] -> bits 15:14.
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  __builtin_amdgcn_s_waitcnt((N & 0xF) | ((N >> 4) << 14) | (0x7 << 4) | (0xF << 8));
}

// Raw s_barrier (no implied waitcnt: the caller has counted its own) that the compiler may not
// move code across.
__device__ __forceinline__ void barrier() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// The activation of every epilogue, and its rounding to bf16: ReLU is `v > 0 ? v : 0` (NaN -> 0,
// -0 -> +0; the numeric contract of ops/loadgen.py).  Scalar on purpose: a helper that takes or
// returns the whole bf16x4 makes the compiler pack the conversions differently.
template <bool RELU>
__device__ __forceinline__ __bf16 act_bf16(float x) {
  return (__bf16)(RELU ? (x > 0.f ? x : 0.f) : x);
}

// Wide epilogue of a BM x BN block tile (all kernels): the bf16 tile is assembled in the
// (then idle) staging LDS and stored as whole rows with 16-B stores instead of each lane's
// scattered 8-B pieces (the D = C^T layout gives a lane 4 consecutive columns of one row).
// Image: row r at r * BN * 2 bytes; its 8-B slot s (4 columns) at slot s ^ ((r & MASK) << 1)
// with MASK = min(15, BN / 8 - 1): a ds_write_b64 lane group (16 rows, one column) spreads
// over 8 bank pairs (2-way), and the 16-B chunk c of row r stays whole at chunk c ^ (r & MASK)
// for the ds_read_b128 pass.  Caller: every wave past its last LDS read, no LDS-DMA in flight.
template <int BN>
__device__ __forceinline__ void wide_put(char* img, int row, int col, bf16x4 o) {
  constexpr int MASK = (BN / 8 - 1) < 15 ? (BN / 8 - 1) : 15;
  const int slot = (col >> 2) ^ ((row & MASK) << 1);
  *reinterpret_cast<bf16x4*>(img + row * (BN * 2) + slot * 8) = o;
}

template <int BM, int BN, int NT>
__device__ __forceinline__ void wide_store(const char* img, __bf16* __restrict__ C, int ldc, int m0, int n0) {
  constexpr int MASK = (BN / 8 - 1) < 15 ? (BN / 8 - 1) : 15;
  constexpr int CPR = BN / 8;                           // 16-B chunks per row
  static_assert(BM * CPR % NT == 0, "wide epilogue split");
#pragma unroll
  for (int k = 0; k < BM * CPR / NT; ++k) {
    const int id = k * NT + (int)threadIdx.x;
    const int row = id / CPR, c = id % CPR;
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(img + row * (BN * 2) + ((c ^ (row & MASK)) << 4));
    *reinterpret_cast<bf16x8*>(C + (size_t)(m0 + row) * ldc + n0 + c * 8) = v;
  }
}

}  // namespace gs
