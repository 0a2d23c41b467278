// MoE combine (gfx950 / MI355X): the weighted scatter-back of the experts' outputs to token order,
//
//   out[t, :] = bf16(sum over j = 0 .. k - 1 of topk_w[t, j] * fp32(y[slot_pos[t * k + j], :]))
//
// y bf16 [P_max, D] in the sorted layout of moe_route.hip, slot_pos int32 [T * k] its inverse map, topk_w fp32
// [T, k], out bf16 [T, D]; D a multiple of 8, row strides in elements.  In fp32: acc = 0.0f, then for j = 0 .. k - 1
// in that order acc = fmaf(w[t, j], y, acc) -- a fused multiply-add whatever the contraction setting -- and one
// rounding to bf16.  Nothing is skipped: a NaN or Inf in y or w reaches its own (t, column) by IEEE rules (0 * NaN
// is NaN) and no other.  A gather, not a scatter: every output element has one writer, so there are no atomics and a
// replay gives the same.
//
// The work is flattened over (token, 16-byte chunk of 8 outputs), one chunk per thread, 256 threads per workgroup:
// ceil(T * D / 2048) workgroups (moe_combine_workgroups).  A thread issues its k row loads (16 bytes each) before
// the first fma.  No bounds checks here by design: the host wrapper (ops/loadgen.py moe_combine) validates.
// 54 VGPRs, no LDS, no scratch.  Measured on an MI355X (profiles/r15_moe): 3.8 us for 256 tokens x 2048 x top-8,
// 13.6 us for 2,048 tokens (76 MB from the Infinity Cache: 5.56 TB/s).
#include "api.h"
#include "paged_attn.h"

namespace gs {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxTopK = 8;

__global__ void __launch_bounds__(kThreads) moe_combine_kernel(const __bf16* __restrict__ y, const int* __restrict__ slot_pos,
                                                               const float* __restrict__ topk_w, __bf16* __restrict__ out,
                                                               int D, int k, int64_t total, size_t ld_y, size_t ld_out) {
  const int64_t chunk = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (chunk >= total) return;
  const int per_row = D >> 3;
  const int t = (int)(chunk / per_row);
  const int col = (int)(chunk - (int64_t)t * per_row) << 3;
  bf16x8 v[kMaxTopK];
  float w[kMaxTopK];
#pragma unroll
  for (int j = 0; j < kMaxTopK; ++j) {
    if (j < k) {
      w[j] = topk_w[t * k + j];
      v[j] = *reinterpret_cast<const bf16x8*>(y + (size_t)slot_pos[t * k + j] * ld_y + col);
    }
  }
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.0f;
#pragma unroll
  for (int j = 0; j < kMaxTopK; ++j) {
    if (j < k) {
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = __fmaf_rn(w[j], (float)v[j][i], acc[i]);
    }
  }
  bf16x8 o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = (__bf16)acc[i];
  *reinterpret_cast<bf16x8*>(out + (size_t)t * ld_out + col) = o;
}

}  // namespace

int moe_combine_workgroups(int T, int D) {
  if (T < 0 || D <= 0 || D % 8) throw std::runtime_error("moe_combine: T must be >= 0 and D a positive multiple of 8");
  const int64_t n = ((int64_t)T * (D / 8) + kThreads - 1) / kThreads;
  if (n >= (int64_t)1 << 31) throw std::runtime_error("moe_combine: more than 2^31 - 1 workgroups");
  return (int)n;
}

void moe_combine_bf16(uintptr_t y, uintptr_t slot_pos, uintptr_t topk_w, uintptr_t out, int T, int D, int k, int64_t ld_y,
                      int64_t ld_out, uintptr_t stream) {
  const int grid = moe_combine_workgroups(T, D);
  if (k < 1 || k > kMaxTopK) throw std::runtime_error("moe_combine: top_k must be in [1, 8]");
  if ((int64_t)T * k >= (int64_t)1 << 31) throw std::runtime_error("moe_combine: more than 2^31 - 1 slots");
  if (ld_y < D || ld_out < D || ld_y % 8 || ld_out % 8)
    throw std::runtime_error("moe_combine: row strides must be >= D and multiples of 8 elements");
  if (y % 16 || out % 16) throw std::runtime_error("moe_combine: y / out must be 16-byte aligned");
  if (slot_pos % 4 || topk_w % 4) throw std::runtime_error("moe_combine: slot_pos / topk_w must be 4-byte aligned");
  if (grid == 0) return;
  if (!y || !slot_pos || !topk_w || !out) throw std::runtime_error("moe_combine: every operand is needed");
  hipLaunchKernelGGL(moe_combine_kernel, dim3(grid), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const __bf16*>(y), reinterpret_cast<const int*>(slot_pos),
                     reinterpret_cast<const float*>(topk_w), reinterpret_cast<__bf16*>(out), D, k,
                     (int64_t)T * (D / 8), (size_t)ld_y, (size_t)ld_out);
  HIP_CHECK(hipGetLastError());
}

}  // namespace gs
