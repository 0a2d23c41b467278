// stream_triad -- a = b + s*c over float4 (16 B/lane) -- the HBM-bound phase of a synthetic pod
// (the MFMA-bound phase is native/hip/gemm.hip).  The triad_variant knob is a process-wide launch
// setting read on the launching host thread, like the GEMM knobs (api.h, gemm.hip).
#include <algorithm>

#include "api.h"
#include "common.h"

namespace gs {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) stream_triad_kernel(float4* __restrict__ a, const float4* __restrict__ b,
                                                           const float4* __restrict__ c, float s, size_t n4) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n4; i += stride) {
    float4 x = b[i], y = c[i];
    a[i] = make_float4(x.x + s * y.x, x.y + s * y.y, x.z + s * y.z, x.w + s * y.w);
  }
}

// Unrolled variant: each thread moves U float4 per trip with all loads issued before
// any store (U outstanding 16-B loads per stream per lane), block-contiguous so every
// load instruction is one coalesced 1 KiB wave access; NT selects non-temporal
// (streaming) loads/stores so the one-touch stream does not evict L2/MALL lines.
// WT: the result goes out with `global_store_dwordx4 ... sc1` (write-through, the line is DROPPED
// from the XCD's L2, MI355X_MICROARCH.md "stores of each flavour") instead of a non-temporal store
// (which keeps the line in L2): a one-touch output stream then does not evict the co-running
// GEMMs' operand panels from L2 (round-6 A/B, variant 8).  Vector stores only.
// THREADS is the workgroup size the kernel is launched with (indexing reads blockDim.x); no LDS and no
// barrier at any size, so a large workgroup costs a co-running GEMM block nothing but registers.
template <int U, bool NT, bool WT = false, int THREADS = 256>
__global__ void __launch_bounds__(THREADS) stream_triad_u(float4* __restrict__ a_, const float4* __restrict__ b_,
                                                          const float4* __restrict__ c_, float s, size_t n4) {
  auto a = reinterpret_cast<f32x4*>(a_);
  auto b = reinterpret_cast<const f32x4*>(b_);
  auto c = reinterpret_cast<const f32x4*>(c_);
  const size_t tile = (size_t)blockDim.x * U;
  const size_t step = (size_t)gridDim.x * tile;
  for (size_t base = (size_t)blockIdx.x * tile + threadIdx.x; base < n4; base += step) {
    f32x4 x[U], y[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const size_t i = base + (size_t)k * blockDim.x;
      if (i < n4) {
        if (NT) {
          x[k] = __builtin_nontemporal_load(b + i);
          y[k] = __builtin_nontemporal_load(c + i);
        } else {
          x[k] = b[i];
          y[k] = c[i];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const size_t i = base + (size_t)k * blockDim.x;
      if (i < n4) {
        const f32x4 r = x[k] + s * y[k];
        if (WT)
          asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(a + i), "v"(r) : "memory");
        else if (NT)
          __builtin_nontemporal_store(r, a + i);
        else
          a[i] = r;
      }
    }
  }
}

// The grid: `blocks` workgroups, but no more than have a tile (float4 per workgroup and trip) of their own --
// a workgroup beyond ceil(n4 / tile) would find base >= n4 and retire at once (the catalog's 64 MiB arrays
// are 4096 tiles of the 256 x 4 kernel: half of the default 8192 blocks did nothing).
static int triad_grid(int blocks, size_t n4, size_t tile) {
  const size_t tiles = (n4 + tile - 1) / tile;
  return (int)std::max<size_t>(1, std::min<size_t>((size_t)blocks, tiles));
}

template <int U, bool NT, bool WT = false, int THREADS = 256>
static void launch_triad_u(int blocks, hipStream_t st, float4* a, const float4* b, const float4* c, float s,
                           size_t n4) {
  hipLaunchKernelGGL((stream_triad_u<U, NT, WT, THREADS>), dim3(triad_grid(blocks, n4, (size_t)THREADS * U)),
                     dim3(THREADS), 0, st, a, b, c, s, n4);
}

// The triad_variant knob.  6 = auto: working set (3 arrays) <= 96 MiB -> cached 2x-unrolled loads (the
// stream stays in the 256 MiB Infinity Cache across iterations: 7.1 TB/s measured), larger ->
// variant 5, the non-temporal 2x kernel in 1024-thread workgroups (profiles/r13_triad_wg/).
// 3 = non-temporal 4x in 256-thread workgroups (what 6 picked before; the lone stream's fastest: 6.5-6.7
// TB/s against 6.1-6.4 for 5 and 7), 7 = non-temporal 3x in 1024-thread workgroups.
//
// Why the workgroup shape matters beside GEMMs.  Registers are allocated in granules of 8 from 512 per SIMD
// lane.  The 4-wave 256 x 256 GEMM block (tile 14, gemm_w4.h) takes 129 VGPRs + 256 AGPRs = 392 per SIMD,
// one wave per SIMD, and all of the CU's LDS, so it needs a CU with at most 512 - 392 = 120 registers per
// SIMD in use.  Variant 3 (38 VGPRs, allocated 40) in 256-thread workgroups puts one wave per SIMD per
// workgroup, 8 workgroups per CU; the GEMM block fits only once five of them have retired with no refill,
// and a queued stream workgroup fits again after every single retirement -- the GEMM block lands only where
// a stream kernel drains.  A 1024-thread workgroup is 4 waves per SIMD: two fill the CU's 32 wave slots,
// the third cannot start before one has retired whole, and at that instant 512 - 4R registers per SIMD are
// free: 416 >= 392 for variant 5 (22 VGPRs, R = 24), so the GEMM block and the next stream workgroup become
// placeable together, and one stream workgroup (96 <= 120) keeps running beside the GEMM block.  Variant 7
// (30 VGPRs, R = 32) leaves 384 < 392 and 4R = 128 > 120: it would need tile 14 at 128 VGPRs.  512- and
// 768-thread workgroups refill after one wave per SIMD retires, before the GEMM block could land.  No LDS
// and no barrier in any of them.  Measured (profiles/r13_triad_wg/): a tile-14 GEMM stream on 64 CUs beside
// one 3 x 256 MiB stream runs 240 TF/s beside variant 5 against 215 beside variant 3, and the bench 6.20
// against 6.58 ms per step, though variant 5 alone is 4-6 % slower than variant 3.
void stream_triad(uintptr_t a, uintptr_t b, uintptr_t c, float s, size_t n_floats, int blocks, uintptr_t stream) {
  if (n_floats % 4) throw std::runtime_error("triad: n must be a multiple of 4");
  check_align(reinterpret_cast<void*>(a), "a");
  check_align(reinterpret_cast<void*>(b), "b");
  check_align(reinterpret_cast<void*>(c), "c");
  if (blocks <= 0) blocks = 8192;
  auto st = reinterpret_cast<hipStream_t>(stream);
  auto A = reinterpret_cast<float4*>(a);
  auto B = reinterpret_cast<const float4*>(b);
  auto Cc = reinterpret_cast<const float4*>(c);
  const size_t n4 = n_floats / 4;
  int variant = knob(k_triad_variant);
  if (variant == 6) variant = (n_floats * 12 <= (size_t)96 << 20) ? 1 : 5;
  // 9 / 10 (A/B arms): write-through stores only for the largest streams (arrays >= 256 / 128 MiB,
  // where a lone sc1 stream gains most), non-temporal below
  if (variant == 9 || variant == 10) variant = n_floats * 4 >= ((size_t)(variant == 9 ? 256 : 128) << 20) ? 8 : 3;
  switch (variant) {
    case 0:
      hipLaunchKernelGGL(stream_triad_kernel, dim3(triad_grid(blocks, n4, 256)), dim3(256), 0, st, A, B, Cc, s, n4);
      break;
    case 1: launch_triad_u<2, false>(blocks, st, A, B, Cc, s, n4); break;
    case 2: launch_triad_u<4, false>(blocks, st, A, B, Cc, s, n4); break;
    case 3: launch_triad_u<4, true>(blocks, st, A, B, Cc, s, n4); break;
    case 4: launch_triad_u<8, true>(blocks, st, A, B, Cc, s, n4); break;
    case 7: launch_triad_u<3, true, false, 1024>(blocks, st, A, B, Cc, s, n4); break;
    case 8: launch_triad_u<4, true, true>(blocks, st, A, B, Cc, s, n4); break;
    default: launch_triad_u<2, true, false, 1024>(blocks, st, A, B, Cc, s, n4); break;
  }
  HIP_CHECK(hipGetLastError());
}

}  // namespace gs
