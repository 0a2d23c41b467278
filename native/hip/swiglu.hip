// SwiGLU (gfx950 / MI355X): out = silu(gate) * up, the step of a decoder block's MLP between the fused gate / up
// projection and the down projection.  An element-wise bf16 stream that pairs column j with column F + j of the
// same row, with a transcendental and an IEEE division per element.
//
//   g, u         = fp32(gate_up[row, j]), fp32(gate_up[row, F + j])
//   e            = exp2(-g * log2e)                                   fp32 product, the hardware v_exp_f32
//   s            = g / (1.0f + e)                                     fp32 add, IEEE division
//   out[row, j]  = bf16(s * u)                                        fp32 product, one rounding
//
// gate_up is [T, 2F] (gate columns [0, F), up columns [F, 2F): what a fused gate / up projection writes), out is
// [T, F], both with row strides; F is a multiple of 8.  Shape of the kernel:
//
//  * the work is flattened over (row, 16-byte chunk of 8 outputs): chunk i is columns 8 (i % (F / 8)) .. + 7 of
//    row i / (F / 8).  A workgroup of 256 threads covers the 1,024 chunks [1024 b, 1024 b + 1024) -- 8,192
//    outputs --, thread t taking the chunks t, t + 256, t + 512 and t + 768 of them: its 8 loads are in flight
//    before the first use, and each load instruction of a wave is one coalesced 1 KiB access wherever it
//    does not cross a row end.  The grid is ceil(T * F / 8192) (swiglu_workgroups); offsets are 64-bit;
//  * consequences of the arithmetic: g = +-0 gives e == 1 and s = +-0; g >= 128 gives e == 0 exactly, so s == g
//    and out = bf16(g * u); g <= -128 gives e == +Inf and s = -0.0; g = -Inf gives NaN (Inf / Inf), as
//    torch.nn.functional.silu does; g = +Inf gives +-Inf * u.  A NaN or Inf in g or u reaches its own output
//    element and no other;
//  * built without -ffast-math: the division is v_div_scale / v_div_fmas / v_div_fixup.
//
// No bounds checks here by design: the host wrapper (ops/loadgen.py swiglu) validates shapes, strides,
// alignment and overlap.
// 50 VGPRs, no AGPRs, no LDS, nothing spilled, 8 waves per SIMD.  Measured on an MI355X as chains of launches
// replayed from one graph (profiles/r12_norm_act): 5.6 us for 256 x 14336 against a launch floor of 1.8 us,
// 29.3 us for 2048 x 14336 (from the Infinity Cache: 1.00e12 outputs/s) and 133.7 us for 8192 x 14336 (from HBM:
// 0.88e12 outputs/s, 5.27 TB/s, 0.80 of the stream triad's 6.60 TB/s in the same run) -- the memory side bounds it,
// not the exponential and the division.  Other chunk counts per thread were not measured.
#include "api.h"
#include "paged_attn.h"

namespace gs {
namespace {

constexpr int kThreads = 256;
constexpr int kChunks = 4;                               // 16-byte output chunks per thread
constexpr int kSpan = kThreads * kChunks;                // chunks per workgroup: 8192 outputs

__global__ void __launch_bounds__(kThreads) swiglu_kernel(const __bf16* __restrict__ gate_up, __bf16* __restrict__ out,
                                                          int F, int64_t total, size_t ld_in, size_t ld_out) {
  const int per_row = F >> 3;                            // chunks of a row
  const int64_t first = (int64_t)blockIdx.x * kSpan + threadIdx.x;
  bf16x8 g[kChunks], u[kChunks];
  size_t dst[kChunks];
#pragma unroll
  for (int k = 0; k < kChunks; ++k) {
    const int64_t chunk = first + k * kThreads;
    if (chunk < total) {
      const int64_t row = chunk / per_row;
      const int col = (int)(chunk - row * per_row) << 3;
      const __bf16* src = gate_up + (size_t)row * ld_in + col;
      g[k] = *reinterpret_cast<const bf16x8*>(src);
      u[k] = *reinterpret_cast<const bf16x8*>(src + F);
      dst[k] = (size_t)row * ld_out + col;
    }
  }
#pragma unroll
  for (int k = 0; k < kChunks; ++k) {
    const int64_t chunk = first + k * kThreads;
    if (chunk < total) {
      bf16x8 o;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float gf = (float)g[k][i];
        const float e = __builtin_amdgcn_exp2f(__fmul_rn(-gf, kLog2e));
        const float s = gf / (1.0f + e);
        o[i] = (__bf16)__fmul_rn(s, (float)u[k][i]);
      }
      *reinterpret_cast<bf16x8*>(out + dst[k]) = o;
    }
  }
}

}  // namespace

int swiglu_workgroups(int T, int F) {
  if (T < 0 || F <= 0 || F % 8) throw std::runtime_error("swiglu: T must be >= 0 and F a positive multiple of 8");
  const int64_t chunks = (int64_t)T * (F / 8);
  const int64_t n = (chunks + kSpan - 1) / kSpan;
  if (n >= (int64_t)1 << 31) throw std::runtime_error("swiglu: more than 2^31 - 1 workgroups");
  return (int)n;
}

void swiglu_bf16(uintptr_t gate_up, uintptr_t out, int T, int F, int64_t ld_in, int64_t ld_out, uintptr_t stream) {
  const int grid = swiglu_workgroups(T, F);
  if (!gate_up || !out) throw std::runtime_error("swiglu: gate_up and out are needed");
  if (ld_in < 2 * (int64_t)F || ld_out < F || ld_in % 8 || ld_out % 8)
    throw std::runtime_error("swiglu: row strides must be >= 2 F / F and multiples of 8 elements");
  if (gate_up % 16 || out % 16) throw std::runtime_error("swiglu: gate_up / out must be 16-byte aligned");
  if (grid == 0) return;
  hipLaunchKernelGGL(swiglu_kernel, dim3(grid), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const __bf16*>(gate_up), reinterpret_cast<__bf16*>(out), F,
                     (int64_t)T * (F / 8), (size_t)ld_in, (size_t)ld_out);
  HIP_CHECK(hipGetLastError());
}

}  // namespace gs
