// Residual add + RMSNorm (gfx950 / MI355X): the step of a decoder block in front of the QKV projection and in
// front of the MLP.  A row reduction followed by a rescale of the same row: two bf16 streams in, two out.
//
//   h            = fp32(x) + fp32(residual)                          one fp32 add
//   res_out      = bf16(h)                                           round to nearest even
//   hb           = fp32(res_out)                                     the ROUNDED stream; fp32(x) without a residual
//   ss           = sum of hb^2 over the row                          fp32, fmaf
//   r            = 1.0f / sqrtf(ss / float(D) + eps)                 IEEE division, add, correctly rounded sqrt, IEEE division
//   y            = bf16((hb * r) * fp32(weight))                     two fp32 multiplies in that order, one rounding
//
// x, residual, res_out and y are [T, D] with row strides, weight is [D]; D is a multiple of 8 in [8, 8192].
// Shape of the kernel:
//
//  * one 256-thread workgroup per row (add_rmsnorm_workgroups = T).  Thread t owns the 16-byte chunks t,
//    t + 256, t + 512 and t + 768 of the row -- those with 8 * chunk < D.  The row stays in registers (32 fp32
//    per thread at D = 8192): every input byte is read once, every output byte written once, 16 bytes per
//    access; row offsets are 64-bit;
//  * the norm is computed from the rounded stream, so add_rmsnorm(x, w, residual) gives bit for bit the y of
//    add_rmsnorm(res_out, w) without a residual;
//  * ss: per-thread partials (fmaf over the thread's chunks in order), a wave butterfly (__shfl_xor, 32 .. 1:
//    a + b == b + a, so every lane of a wave ends with the same bits), then the four wave partials through LDS,
//    summed by every thread as ((p0 + p1) + p2) + p3.  All threads of a row hold the same ss; there are no
//    atomics, so two launches on the same inputs are bit-identical;
//  * a thread loads all its chunks of x and residual before it stores any of res_out, and no other thread
//    touches them: res_out may be exactly residual (the in-place update of the residual stream);
//  * NaN, Inf and zeros are not special-cased: a NaN in a row makes ss and so the row's whole y NaN, and in
//    res_out only its own element; an all-zero row gives r = 1 / sqrt(eps) and zeros with the sign of
//    hb * w, NaN with eps == 0 (0 * Inf); no other row is ever affected;
//  * built without -ffast-math: the divisions are v_div_scale / v_div_fmas / v_div_fixup, the square root
//    v_sqrt_f32 with its +-1 ulp fix-up.  No rsqrtf.
//
// No bounds checks here by design: the host wrapper (ops/loadgen.py add_rmsnorm) validates shapes, strides,
// alignment and overlap.
// 66 VGPRs with a residual (7 waves per SIMD), 59 without (8), no AGPRs, 16 bytes of LDS, nothing spilled.
// Measured on an MI355X as chains of launches replayed from one graph (profiles/r12_norm_act): 3.4 us for
// 256 x 4096 against a launch floor of 2.1 us, 11.3 us for 2048 x 4096 (from the Infinity Cache) and 96.5 us for
// 8192 x 8192: 5.56 TB/s, 0.84 of the stream triad's 6.60 TB/s in the same run.
#include "api.h"
#include "paged_attn.h"

namespace gs {
namespace {

constexpr int kThreads = 256;
constexpr int kChunks = 4;                               // 16-byte chunks of a row per thread: D <= 8192
constexpr int kMaxD = 8 * kThreads * kChunks;

template <bool kResidual>
__global__ void __launch_bounds__(kThreads) add_rmsnorm_kernel(
    const __bf16* __restrict__ x, const __bf16* residual, const __bf16* __restrict__ weight, __bf16* res_out,
    __bf16* __restrict__ y, int D, size_t ld_x, size_t ld_res, size_t ld_res_out, size_t ld_y, float eps) {
  __shared__ float part[kThreads / kWave];
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  const int nchunks = D >> 3;
  const __bf16* xr = x + row * ld_x;

  bf16x8 xv[kChunks], rv[kChunks], wv[kChunks];
#pragma unroll
  for (int c = 0; c < kChunks; ++c) {
    const int chunk = tid + c * kThreads;
    if (chunk < nchunks) {
      xv[c] = *reinterpret_cast<const bf16x8*>(xr + 8 * chunk);
      if (kResidual) rv[c] = *reinterpret_cast<const bf16x8*>(residual + row * ld_res + 8 * chunk);
      wv[c] = *reinterpret_cast<const bf16x8*>(weight + 8 * chunk);
    }
  }

  float hb[kChunks][8];
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < kChunks; ++c) {
    const int chunk = tid + c * kThreads;
    if (chunk < nchunks) {
      bf16x8 ro;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float v = (float)xv[c][e];
        if (kResidual) {
          ro[e] = (__bf16)(v + (float)rv[c][e]);
          v = (float)ro[e];
        }
        hb[c][e] = v;
        ss = __fmaf_rn(v, v, ss);
      }
      if (kResidual) *reinterpret_cast<bf16x8*>(res_out + row * ld_res_out + 8 * chunk) = ro;
    }
  }

#pragma unroll
  for (int m = kWave / 2; m > 0; m >>= 1) ss += __shfl_xor(ss, m, kWave);
  if ((tid & (kWave - 1)) == 0) part[tid / kWave] = ss;
  __syncthreads();
  ss = ((part[0] + part[1]) + part[2]) + part[3];
  const float r = 1.0f / sqrtf(ss / (float)D + eps);

#pragma unroll
  for (int c = 0; c < kChunks; ++c) {
    const int chunk = tid + c * kThreads;
    if (chunk < nchunks) {
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (__bf16)__fmul_rn(__fmul_rn(hb[c][e], r), (float)wv[c][e]);
      *reinterpret_cast<bf16x8*>(y + row * ld_y + 8 * chunk) = o;
    }
  }
}

}  // namespace

int add_rmsnorm_workgroups(int T) {
  if (T < 0) throw std::runtime_error("add_rmsnorm: negative T");
  return T;
}

void add_rmsnorm_bf16(uintptr_t x, uintptr_t residual, uintptr_t weight, uintptr_t res_out, uintptr_t y, int T, int D,
                      int64_t ld_x, int64_t ld_res, int64_t ld_res_out, int64_t ld_y, float eps, uintptr_t stream) {
  if (T < 0) throw std::runtime_error("add_rmsnorm: negative T");
  if (D < 8 || D > kMaxD || D % 8) throw std::runtime_error("add_rmsnorm: D must be a multiple of 8 in [8, 8192]");
  if (!x || !weight || !y || (residual && !res_out) || (!residual && res_out))
    throw std::runtime_error("add_rmsnorm: x, weight and y are needed, residual and res_out come together");
  if (ld_x < D || ld_y < D || ld_x % 8 || ld_y % 8 ||
      (residual && (ld_res < D || ld_res_out < D || ld_res % 8 || ld_res_out % 8)))
    throw std::runtime_error("add_rmsnorm: row strides must be >= D and multiples of 8 elements");
  if (x % 16 || residual % 16 || weight % 16 || res_out % 16 || y % 16)
    throw std::runtime_error("add_rmsnorm: x / residual / weight / res_out / y must be 16-byte aligned");
  if (!(eps >= 0.f) || eps > 3.402823466e38f) throw std::runtime_error("add_rmsnorm: eps must be finite and >= 0");
  const int grid = add_rmsnorm_workgroups(T);
  if (grid == 0) return;
  auto st = reinterpret_cast<hipStream_t>(stream);
  auto X = reinterpret_cast<const __bf16*>(x);
  auto R = reinterpret_cast<const __bf16*>(residual);
  auto W = reinterpret_cast<const __bf16*>(weight);
  auto RO = reinterpret_cast<__bf16*>(res_out);
  auto Y = reinterpret_cast<__bf16*>(y);
  if (residual)
    hipLaunchKernelGGL(add_rmsnorm_kernel<true>, dim3(grid), dim3(kThreads), 0, st, X, R, W, RO, Y, D, (size_t)ld_x,
                       (size_t)ld_res, (size_t)ld_res_out, (size_t)ld_y, eps);
  else
    hipLaunchKernelGGL(add_rmsnorm_kernel<false>, dim3(grid), dim3(kThreads), 0, st, X, R, W, RO, Y, D, (size_t)ld_x,
                       (size_t)ld_res, (size_t)ld_res_out, (size_t)ld_y, eps);
  HIP_CHECK(hipGetLastError());
}

}  // namespace gs
