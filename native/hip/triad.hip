// stream_triad -- a = b + s*c over float4 (16 B/lane) -- the HBM-bound phase of a synthetic pod
// (the MFMA-bound phase is native/hip/gemm.hip).  The triad_variant knob is a process-wide launch
// setting read on the launching host thread, like the GEMM knobs (api.h, gemm.hip).
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
template <int U, bool NT, bool WT = false>
__global__ void __launch_bounds__(256) stream_triad_u(float4* __restrict__ a_, const float4* __restrict__ b_,
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

// The triad_variant knob.  6 = auto: working set (3 arrays) <= 96 MiB -> cached 2x-unrolled loads (the
// stream stays in the 256 MiB Infinity Cache across iterations: 7.1 TB/s measured), larger ->
// non-temporal 4x (6.5 TB/s vs 6.1 for torch.add) -- profiles/r01_kernel_bench.json.
// 5 = non-temporal 2x (22 VGPRs), 7 = non-temporal 3x (<= 32 VGPRs): a triad wave small enough
// to fit beside an 8-phase GEMM block's 2 x 240 VGPRs per SIMD (the 4x variant's 38 VGPRs do
// not, so a CU running a 256 x 256 GEMM block takes no triad wave at all; round 6 A/B)
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
  if (variant == 6) variant = (n_floats * 12 <= (size_t)96 << 20) ? 1 : 3;
  // 9 / 10 (A/B arms): write-through stores only for the largest streams (arrays >= 256 / 128 MiB,
  // where a lone sc1 stream gains most), non-temporal below
  if (variant == 9 || variant == 10) variant = n_floats * 4 >= ((size_t)(variant == 9 ? 256 : 128) << 20) ? 8 : 3;
  switch (variant) {
    case 0: hipLaunchKernelGGL(stream_triad_kernel, dim3(blocks), dim3(256), 0, st, A, B, Cc, s, n4); break;
    case 1: hipLaunchKernelGGL((stream_triad_u<2, false>), dim3(blocks), dim3(256), 0, st, A, B, Cc, s, n4); break;
    case 2: hipLaunchKernelGGL((stream_triad_u<4, false>), dim3(blocks), dim3(256), 0, st, A, B, Cc, s, n4); break;
    case 3: hipLaunchKernelGGL((stream_triad_u<4, true>), dim3(blocks), dim3(256), 0, st, A, B, Cc, s, n4); break;
    case 4: hipLaunchKernelGGL((stream_triad_u<8, true>), dim3(blocks), dim3(256), 0, st, A, B, Cc, s, n4); break;
    case 7: hipLaunchKernelGGL((stream_triad_u<3, true>), dim3(blocks), dim3(256), 0, st, A, B, Cc, s, n4); break;
    case 8: hipLaunchKernelGGL((stream_triad_u<4, true, true>), dim3(blocks), dim3(256), 0, st, A, B, Cc, s, n4); break;
    default: hipLaunchKernelGGL((stream_triad_u<2, true>), dim3(blocks), dim3(256), 0, st, A, B, Cc, s, n4); break;
  }
  HIP_CHECK(hipGetLastError());
}

}  // namespace gs
