// Grouped expert GEMM of a mixture-of-experts MLP (gfx950 / MI355X): out[i, :] = bf16(A[src(i), :] . W[e]^T) for
// the rows i of the sorted, tile-aligned layout moe_route.hip builds -- e = tile_expert[i / 64], one weight matrix
// per 64-row tile, bf16 operands, fp32 accumulation on v_mfma_f32_16x16x32_bf16, one rounding.
//
//   gather_div = k >= 1   src(i) = sorted_ids[i] / k: the first projection reads TOKEN rows through the permutation
//   gather_div = 0        src(i) = i: the down projection reads the sorted intermediate in place
//
// Shape of the kernel (the pieces of gemm_device.h: the swizzled LDS image, lds_frag, counted vmcnt):
//  * block tile 64 x BN, BN = 128 where N % 128 == 0 and 64 otherwise; 256 threads, 2 x 2 waves of 32 x BN/2; three
//    LDS stages of (64 + BN) x 64 bf16 (72 / 48 KiB), the LDS-DMA loads issued two K tiles ahead.  At decode sizes
//    an expert has ~16 rows, so the op streams every expert's weights for one tile each: it is bound by HBM, and
//    what matters is bytes in flight, not MFMA issue;
//  * the A tile is a ROW GATHER: an LDS-DMA load takes its source address per lane, so stage_rows is stage_tile with
//    a row pointer per (thread, pass) instead of r0 + r -- the pointers (swizzled chunk included) are computed once
//    before the K loop from the 64 source rows the first wave put into LDS;
//  * a pad row (sorted_ids[i] >= n_slots) reads its tile's first row's source instead (a valid row: an expert's
//    slots come first in its tiles) and is written as +0.0 (0x0000) across its N columns by the epilogue;
//  * a workgroup whose tile is unused (tile_expert < 0) exits before it reads or writes anything else.  The grid is
//    max_tiles * (N / BN), fixed on the host (no sync, capturable);
//  * order: the XCD-contiguous remap of tile_coords (workgroups b, b + 8, ... share an XCD), then N-tile fastest --
//    the N-tiles of one M-tile, which share the gathered A rows, and the consecutive M-tiles of one expert, which
//    share its weights, are neighbours in one XCD's dispatch order and meet in its L2;
//  * the accumulation runs over K in one fixed order per output element, the same for every row of a tile: no
//    split-K, no atomics -- launches repeat bit for bit and a row's result does not depend on its place in a tile.
//
// No bounds checks on the operands by design: the host wrapper (ops/loadgen.py moe_gemm) validates them.
// Compiler's resource usage: BN = 128: 86 VGPRs, no AGPRs, 73,984 bytes of LDS, no scratch (2 workgroups per CU by
// LDS); BN = 64: 54 VGPRs, 49,408 bytes of LDS, no scratch (3 per CU).
// Measured on an MI355X as chains of launches replayed from one graph (profiles/r15_moe; 128 experts, top-8, randn
// routing): at 256 tokens 176.1 us for N = 1536, K = 2048 (805 MB of expert weights at 4.57 TB/s, 0.73 of the stream
// triad's 6.29 TB/s in the same run) and 97.1 us for N = 2048, K = 768 (0.66); at 2,048 tokens 312.8 and 177.8 us
// (330 and 290 TF/s on the useful rows, 3.2 times the time of the dense GEMM of equal useful flops).  Other tiles, stage
// counts and workgroup orders were not measured.
#include "api.h"
#include "gemm_device.h"

namespace gs {
namespace {

constexpr int kBM = 64, kThreads = 256, kStages = 3;

// The glds of a 64 x 64 bf16 A tile whose rows come from anywhere: rowp[i] is the address of this thread's chunk
// of row i * 32 + tid / 8 at k = 0 (swizzled source chunk included), the LDS image that of stage_tile<64, 256>.
__device__ __forceinline__ void stage_rows(const __bf16* const (&rowp)[2], int k0, char* lds_tile, int wave) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    char* dst = lds_tile + (i * kThreads + wave * 64) * 16;          // wave-uniform base
    __builtin_amdgcn_global_load_lds((gptr_t)(rowp[i] + k0), (lptr_t)dst, 16, 0, 0);
  }
}

template <int BN>
__global__ void __launch_bounds__(kThreads, 2)
moe_gemm_kernel(const __bf16* __restrict__ A, const __bf16* __restrict__ W, __bf16* __restrict__ C,
                const int* __restrict__ sorted_ids, const int* __restrict__ tile_expert, int n_slots, int gather_div,
                int tiles_n, int K, size_t lda, size_t ldw, size_t expert_stride, size_t ldc) {
  constexpr int WGM = 2, WGN = 2;
  constexpr int A_BYTES = kBM * BK * 2, B_BYTES = BN * BK * 2;
  constexpr int WTM = kBM / WGM, WTN = BN / WGN;
  constexpr int MI = WTM / 16, NJ = WTN / 16;
  constexpr int LOADS = (kBM + BN) * BK * 2 / 16 / kThreads;         // glds per thread per K tile
  __shared__ __attribute__((aligned(16))) char smem[kStages * (A_BYTES + B_BYTES)];
  __shared__ int src_row[kBM];                                       // the A row of each tile row; -1: a pad row

  // XCD-contiguous order, N-tile fastest
  const int b = blockIdx.x, nwg = gridDim.x;
  const int xcd = b % kXcds, q = nwg / kXcds, rem = nwg % kXcds;
  const int wgid = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + b / kXcds;
  const int tm = wgid / tiles_n, tn = wgid - tm * tiles_n;
  const int expert = tile_expert[tm];
  if (expert < 0) return;                                            // an unused tile: uniform over the workgroup
  const int m0 = tm * kBM, n0 = tn * BN;

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int lane = threadIdx.x & (kWave - 1);
  const int wm = wave / WGN, wn = wave % WGN;
  if (threadIdx.x < kBM) {
    const int id = sorted_ids[m0 + threadIdx.x];
    const bool valid = (unsigned)id < (unsigned)n_slots;
    src_row[threadIdx.x] = valid ? (gather_div ? id / gather_div : m0 + (int)threadIdx.x) : -1;
  }
  __syncthreads();
  const int first = src_row[0] < 0 ? 0 : src_row[0];
  const __bf16* rowp[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = i * (kThreads / 8) + (int)threadIdx.x / 8;
    const int kc = ((int)threadIdx.x & 7) ^ ((r >> 1) & 7);
    const int src = src_row[r] < 0 ? first : src_row[r];
    rowp[i] = A + (size_t)src * lda + kc * 8;
  }
  const __bf16* Bt = W + (size_t)expert * expert_stride;

  f32x4 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto tileA = [&](int buf) { return smem + buf * (A_BYTES + B_BYTES); };
  auto tileB = [&](int buf) { return smem + buf * (A_BYTES + B_BYTES) + A_BYTES; };
  const int nt = K / BK;
  const int frow = lane & 15, fk = lane >> 4;
  auto compute = [&](const char* a_t, const char* b_t) {
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
      bf16x8 af[MI], bf[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) bf[j] = lds_frag<BK>(b_t, wn * WTN + j * 16 + frow, kk * 4 + fk);
#pragma unroll
      for (int i = 0; i < MI; ++i) af[i] = lds_frag<BK>(a_t, wm * WTM + i * 16 + frow, kk * 4 + fk);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[j], af[i], acc[i][j], 0, 0, 0);
    }
  };
  auto stage = [&](int t, int buf) {
    stage_rows(rowp, t * BK, tileA(buf), wave);
    stage_tile<BN, kThreads, BK>(Bt, (int)ldw, n0, t * BK, tileB(buf), wave, lane);
  };

  // tiles 0 and 1 in flight; iteration t: wait until only the tile after t is outstanding (loads retire in order),
  // barrier (tile t landed for everyone, tile t - 1 read by everyone), issue tile t + 2 into t - 1's buffer
#pragma unroll
  for (int p = 0; p < kStages - 1; ++p)
    if (p < nt) stage(p, p);
  for (int t = 0; t < nt; ++t) {
    if (nt - 1 - t >= 1) {
      wait_vmcnt<LOADS>();
    } else {
      wait_vmcnt<0>();
    }
    barrier();
    if (t + kStages - 1 < nt) stage(t + kStages - 1, (t + kStages - 1) % kStages);
    compute(tileA(t % kStages), tileB(t % kStages));
  }

  // wide epilogue (D = C^T layout: a lane holds 4 consecutive columns of one row): the bf16 tile through the idle
  // staging LDS, whole rows out with 16-byte stores, a pad row as zeros
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int col = wn * WTN + j * 16 + fk * 4;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      bf16x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = act_bf16<false>(acc[i][j][r]);
      wide_put<BN>(smem, wm * WTM + i * 16 + frow, col, o);
    }
  }
  __syncthreads();
  constexpr int MASK = (BN / 8 - 1) < 15 ? (BN / 8 - 1) : 15;
  constexpr int CPR = BN / 8;
#pragma unroll
  for (int p = 0; p < kBM * CPR / kThreads; ++p) {
    const int id = p * kThreads + (int)threadIdx.x;
    const int row = id / CPR, c = id % CPR;
    bf16x8 v = *reinterpret_cast<const bf16x8*>(smem + row * (BN * 2) + ((c ^ (row & MASK)) << 4));
    if (src_row[row] < 0) v = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    *reinterpret_cast<bf16x8*>(C + (size_t)(m0 + row) * ldc + n0 + c * 8) = v;
  }
}

int block_n(int N) { return N % 128 == 0 ? 128 : 64; }

}  // namespace

int moe_gemm_workgroups(int T, int k, int E, int N) {
  if (N <= 0 || N % 64) throw std::runtime_error("moe_gemm: N must be a positive multiple of 64");
  const int64_t n = (int64_t)moe_max_tiles(T, k, E) * (N / block_n(N));
  if (n >= (int64_t)1 << 31) throw std::runtime_error("moe_gemm: more than 2^31 - 1 workgroups");
  return (int)n;
}

void moe_gemm_bf16(uintptr_t a, uintptr_t w, uintptr_t sorted_ids, uintptr_t tile_expert, uintptr_t out, int max_tiles,
                   int n_slots, int gather_div, int N, int K, int64_t lda, int64_t ldw, int64_t expert_stride,
                   int64_t ldc, uintptr_t stream) {
  if (max_tiles < 0 || n_slots < 0 || gather_div < 0) throw std::runtime_error("moe_gemm: negative sizes");
  if (N <= 0 || K <= 0 || N % 64 || K % 64) throw std::runtime_error("moe_gemm: N and K must be positive multiples of 64");
  if (lda < K || ldw < K || ldc < N || lda % 8 || ldw % 8 || ldc % 8 || expert_stride < 0 || expert_stride % 8)
    throw std::runtime_error("moe_gemm: row strides must be >= K / K / N, and every stride a multiple of 8 elements");
  if (ldw >= (int64_t)1 << 31) throw std::runtime_error("moe_gemm: the weights' row stride is past 2^31 - 1");
  if (a % 16 || w % 16 || out % 16) throw std::runtime_error("moe_gemm: a / w / out must be 16-byte aligned");
  if (sorted_ids % 4 || tile_expert % 4) throw std::runtime_error("moe_gemm: sorted_ids / tile_expert must be 4-byte aligned");
  if (max_tiles == 0) return;
  if (!a || !w || !out || !sorted_ids || !tile_expert) throw std::runtime_error("moe_gemm: every operand is needed");
  const int bn = block_n(N), tiles_n = N / bn;
  const int64_t grid = (int64_t)max_tiles * tiles_n;
  if (grid >= (int64_t)1 << 31) throw std::runtime_error("moe_gemm: more than 2^31 - 1 workgroups");
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const __bf16*>(a), reinterpret_cast<const __bf16*>(w),
                       reinterpret_cast<__bf16*>(out), reinterpret_cast<const int*>(sorted_ids),
                       reinterpret_cast<const int*>(tile_expert), n_slots, gather_div, tiles_n, K, (size_t)lda,
                       (size_t)ldw, (size_t)expert_stride, (size_t)ldc);
  };
  if (bn == 128) launch(moe_gemm_kernel<128>); else launch(moe_gemm_kernel<64>);
  HIP_CHECK(hipGetLastError());
}

}  // namespace gs
