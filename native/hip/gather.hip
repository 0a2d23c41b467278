// Embedding-bag row gather (gfx950 / MI355X): the indexed-rows pod phase.
//
//   out[b, 0:D] = bf16_rne( sum over j in [offsets[b], offsets[b+1]) of float(table[idx[j], 0:D]) )
//
// HBM-bound like the stream triad, but its traffic is random rows, it has no MFMA work, and short
// rows move few bytes per wave-instruction.  Shape of the kernel:
//
//  * one wave per bag, four bags per 256-thread workgroup; no LDS and no barrier, so a wave whose
//    bag index is past B simply leaves.  The workgroups walk the bags grid-stride;
//  * every row access is a 16-byte load per lane.  A wave-instruction covers 512 elements: for
//    D <= 512 that is G = 512 / D rows at once (lane group g = lane / (64 / G) takes row g of each
//    step, and the groups' partial sums are added across lanes once per bag); for D > 512 a row
//    takes C = D / 512 instructions;
//  * U = 4 steps (4 G rows) are loaded before the first is consumed, and the indices of the next
//    4 steps are loaded behind them -- a full row latency ahead of the row loads they feed;
//  * for D >= 512 the bag, its offsets and its indices are wave-uniform (scalar registers and
//    scalar loads); for D < 512 the index is per lane group (a vector load, 64 / G lanes share an
//    address);
//  * row addresses are 64-bit (idx * ld_table * 2 passes 4 GiB on a large table); the sum is fp32
//    in registers, rounded to bf16 once, stored 16 bytes per lane by lane group 0.
//
// No bounds checks here by design: the host wrapper (ops/loadgen.py embedding_bag) validates the
// shapes, strides and alignment, and on request the indices.
#include "api.h"
#include "common.h"

namespace gs {
namespace {

typedef short bf16x8_bits __attribute__((ext_vector_type(8)));      // 8 bf16 = one 16-byte access
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kBagsPerBlock = 4;      // waves of a 256-thread workgroup
constexpr int kInFlight = 4;          // steps loaded before the first is consumed

// acc[0:8] += the 8 bf16 of one 16-byte access (a bf16 is the upper half of its fp32)
__device__ __forceinline__ void add_row(float (&acc)[8], bf16x8_bits v) {
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] += __builtin_bit_cast(float, (uint32_t)(uint16_t)v[e] << 16);
}

template <int D>
__global__ void __launch_bounds__(256) embedding_bag_kernel(const __bf16* __restrict__ table,
                                                            const int* __restrict__ idx,
                                                            const int* __restrict__ offsets,
                                                            __bf16* __restrict__ out, int B, size_t ld_table,
                                                            size_t ld_out) {
  constexpr int G = D <= 512 ? 512 / D : 1;       // rows per wave-instruction
  constexpr int C = D <= 512 ? 1 : D / 512;       // wave-instructions per row
  constexpr int LPR = kWave / G;                  // lanes per row
  constexpr int U = kInFlight;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const unsigned g = G == 1 ? 0u : (unsigned)(lane / LPR);
  const int col = (lane % LPR) * 8;
  const __bf16* tcol = table + col;
  for (long bag = (long)blockIdx.x * kBagsPerBlock + wave; bag < B; bag += (long)gridDim.x * kBagsPerBlock) {
    const unsigned beg = (unsigned)offsets[bag], end = (unsigned)offsets[bag + 1];
    float acc[C][8];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[c][e] = 0.f;
    if (beg < end) {
      // index positions past the bag's end are clamped to its last one: every index load is
      // unconditional and stays inside the bag; whether its row is used is decided below
      const unsigned last = end - 1;
      unsigned j0 = beg;
      unsigned id[U];
#pragma unroll
      for (int u = 0; u < U; ++u) id[u] = (unsigned)idx[min(j0 + u * G + g, last)];
      // full steps: U * G rows, no conditions
      for (; j0 + U * G <= end; j0 += U * G) {
        bf16x8_bits v[U][C];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          auto p = reinterpret_cast<const bf16x8_bits*>(tcol + (size_t)id[u] * ld_table);
#pragma unroll
          for (int c = 0; c < C; ++c) v[u][c] = p[c * kWave];
        }
        unsigned nid[U];
#pragma unroll
        for (int u = 0; u < U; ++u) nid[u] = (unsigned)idx[min(j0 + (U + u) * G + g, last)];
        // keep the index loads here, behind the row loads and in front of the adds: sunk to the
        // loop's end, they are waited for at once and every step pays index, then rows
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
          for (int c = 0; c < C; ++c) add_row(acc[c], v[u][c]);
          id[u] = nid[u];
        }
      }
      // the ragged last step: only the rows inside the bag are loaded
      if (j0 < end) {
        bf16x8_bits v[U][C];
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
          for (int c = 0; c < C; ++c) v[u][c] = bf16x8_bits{0, 0, 0, 0, 0, 0, 0, 0};
          if (j0 + u * G + g < end) {
            auto p = reinterpret_cast<const bf16x8_bits*>(tcol + (size_t)id[u] * ld_table);
#pragma unroll
            for (int c = 0; c < C; ++c) v[u][c] = p[c * kWave];
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int c = 0; c < C; ++c) add_row(acc[c], v[u][c]);
      }
    }
    if (G > 1) {
#pragma unroll
      for (int m = LPR; m < kWave; m <<= 1)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[0][e] += __shfl_xor(acc[0][e], m, kWave);
    }
    if (g == 0) {
      auto o = reinterpret_cast<bf16x8*>(out + (size_t)bag * ld_out + col);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        bf16x8 r;
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = (__bf16)acc[c][e];
        o[c * kWave] = r;
      }
    }
  }
}

template <int D>
void launch_bag(const __bf16* table, const int* idx, const int* offsets, __bf16* out, int B, size_t ld_table,
                size_t ld_out, int grid, hipStream_t st) {
  hipLaunchKernelGGL(embedding_bag_kernel<D>, dim3(grid), dim3(256), 0, st, table, idx, offsets, out, B, ld_table,
                     ld_out);
}

}  // namespace

int embedding_bag_workgroups(int B, int blocks) {
  const int need = B / kBagsPerBlock + (B % kBagsPerBlock ? 1 : 0);
  return blocks > 0 && blocks < need ? blocks : need;
}

void embedding_bag_bf16(uintptr_t table, uintptr_t idx, uintptr_t offsets, uintptr_t out, int B, int D,
                        int64_t ld_table, int64_t ld_out, int blocks, uintptr_t stream) {
  if (B < 0) throw std::runtime_error("embedding_bag: negative bag count");
  if (ld_table < D || ld_out < D || ld_table % 8 || ld_out % 8)
    throw std::runtime_error("embedding_bag: row strides must be >= D and multiples of 8 elements");
  if (table % 16 || out % 16) throw std::runtime_error("embedding_bag: table / out must be 16-byte aligned");
  if (idx % 4 || offsets % 4) throw std::runtime_error("embedding_bag: idx / offsets must be 4-byte aligned");
  if (B == 0) return;
  auto T = reinterpret_cast<const __bf16*>(table);
  auto I = reinterpret_cast<const int*>(idx);
  auto O = reinterpret_cast<const int*>(offsets);
  auto Y = reinterpret_cast<__bf16*>(out);
  auto st = reinterpret_cast<hipStream_t>(stream);
  const int grid = embedding_bag_workgroups(B, blocks);
  const size_t lt = (size_t)ld_table, lo = (size_t)ld_out;
  switch (D) {
    case 64: launch_bag<64>(T, I, O, Y, B, lt, lo, grid, st); break;
    case 128: launch_bag<128>(T, I, O, Y, B, lt, lo, grid, st); break;
    case 256: launch_bag<256>(T, I, O, Y, B, lt, lo, grid, st); break;
    case 512: launch_bag<512>(T, I, O, Y, B, lt, lo, grid, st); break;
    case 1024: launch_bag<1024>(T, I, O, Y, B, lt, lo, grid, st); break;
    case 2048: launch_bag<2048>(T, I, O, Y, B, lt, lo, grid, st); break;
    default: throw std::runtime_error("embedding_bag: D must be a power of two in [64, 2048]");
  }
  HIP_CHECK(hipGetLastError());
}

}  // namespace gs
