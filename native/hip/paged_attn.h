// What the two paged-KV attention kernels (decode_attn.hip, prefill_attn.hip) share: the fixed sizes of
// the cache layout, the MFMA fragment types and the host-side operand checks of their launch functions.
#pragma once
#include <string>

#include "common.h"

namespace gs {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short bf16x8_bits __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kHeadDim = 128;
constexpr int kBlockTokens = 32;
constexpr int kMaxGroup = 16;                     // the MFMA's column dimension
constexpr float kLog2e = 1.44269504088896340736f;

// the 8 K fragments of one (block, KV head) slab: tile t, k-step kk is d = 32 kk + 8 g .. + 7 of
// the lane's token 8 (rho >> 2) + 4 t + (rho & 3) -- p already points at the lane's place
__device__ __forceinline__ void load_k(bf16x8 (&kf)[2][4], const __bf16* p) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
      kf[t][kk] = *reinterpret_cast<const bf16x8*>(p + t * 4 * kHeadDim + kk * 32);
}

// What the readers of an FP8 cache (decode_attn_kv8.hip, prefill_attn_kv8.hip) share: the byte fragments
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// the 4 K pieces of one (block, KV head) slab: tile t, half h is d = 64 h + 16 g .. + 15 of the lane's token
// 8 (rho >> 2) + 4 t + (rho & 3) -- p already points at the lane's place
__device__ __forceinline__ void load_k8(u32x4 (&kf)[2][2], const uint8_t* p) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int h = 0; h < 2; ++h) kf[t][h] = *reinterpret_cast<const u32x4*>(p + t * 4 * kHeadDim + h * 64);
}

// What the decode kernels (decode_attn.hip over a bf16 cache, decode_attn_kv8.hip over an FP8 one) share beyond
// that: the per-wave partials in LDS, their merge and the final division.
constexpr int kWaves = 4;
constexpr int kOLd = kHeadDim + 4;                // fp32 row of the LDS image: 528 bytes, 16-byte aligned
constexpr int kPartLd = kOLd;                     // a split's workspace row: 128 accumulators, m, l, 2 words unused
constexpr int kMaxKvSplits = 32;

struct Partials {
  float o[kWaves][kMaxGroup][kOLd];
  float m[kWaves][kMaxGroup];
  float l[kWaves][kMaxGroup];
};

// The merge of the four waves' partials for head c of the group, elements d0 .. d0 + 7: each is
// weighed by a_w = exp(m_w - max m).  acc = sum_w a_w O_w, mx = max_w m_w, lsum = sum_w a_w l_w
__device__ __forceinline__ void merge_waves(const Partials& sm, int c, int d0, float (&acc)[8], float& mx,
                                            float& lsum) {
  const float ninf = -__builtin_inff();
  float mw[kWaves];
  mx = ninf;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    mw[w] = sm.m[w][c];
    mx = fmaxf(mx, mw[w]);
  }
  lsum = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    // a wave without blocks (all of them when ctx == 0) has m = -inf: weight 0, never (-inf) - (-inf)
    const float a = mw[w] == ninf ? 0.f : __builtin_amdgcn_exp2f((mw[w] - mx) * kLog2e);
    lsum += a * sm.l[w][c];
    const f32x4 lo = *reinterpret_cast<const f32x4*>(&sm.o[w][c][d0]);
    const f32x4 hi = *reinterpret_cast<const f32x4*>(&sm.o[w][c][d0 + 4]);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[e] += a * lo[e];
      acc[4 + e] += a * hi[e];
    }
  }
}

// lsum == 0 only for ctx == 0 (every weight 0): +0.0.  A NaN normaliser divides: NaN out
__device__ __forceinline__ bf16x8 normalised(const float (&acc)[8], float lsum) {
  bf16x8 r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = (__bf16)(lsum == 0.f ? 0.f : acc[e] / lsum);
  return r;
}

// The same with the FP8 cache's V scale: bf16((acc / lsum) * v_scale), the division first
__device__ __forceinline__ bf16x8 normalised(const float (&acc)[8], float lsum, float v_scale) {
  bf16x8 r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = (__bf16)(lsum == 0.f ? 0.f : __fmul_rn(acc[e] / lsum, v_scale));
  return r;
}

// A split's undivided partial of one head, elements d0 .. d0 + 7, to its workspace row: the 128 accumulators,
// then m and l (written by the thread with d0 == 0)
__device__ __forceinline__ void store_split_row(float* row, int d0, const float (&acc)[8], float mx, float lsum) {
  *reinterpret_cast<f32x4*>(row + d0) = f32x4{acc[0], acc[1], acc[2], acc[3]};
  *reinterpret_cast<f32x4*>(row + d0 + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
  if (d0 == 0) {
    row[kHeadDim] = mx;
    row[kHeadDim + 1] = lsum;
  }
}

// The kv_splits workspace rows of output row `row` (= s * Hq + h), elements d0 .. d0 + 7, combined by
// merge_waves' formula over splits: acc = sum_p a_p O_p, lsum = sum_p a_p l_p.  This is the loop of
// paged_decode_merge_kernel (decode_attn.hip), which keeps it in its own body: called from here the compiler
// schedules that kernel differently, and the bf16 kernels are kept instruction for instruction; the FP8 merge
// kernel calls this
__device__ __forceinline__ void merge_splits(const float* __restrict__ workspace, int row, int kv_splits, int d0,
                                             float (&acc)[8], float& lsum) {
  const float ninf = -__builtin_inff();
  const float* part = workspace + (size_t)row * kv_splits * kPartLd;
  float mx = ninf;
#pragma unroll 4
  for (int p = 0; p < kv_splits; ++p) mx = fmaxf(mx, part[(size_t)p * kPartLd + kHeadDim]);
  lsum = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll 4                                     // four splits' loads in flight
  for (int p = 0; p < kv_splits; ++p) {
    const float* pr = part + (size_t)p * kPartLd;
    const float mp = pr[kHeadDim];
    // an empty split (all of them when ctx == 0) has m = -inf: weight 0, never (-inf) - (-inf)
    const float a = mp == ninf ? 0.f : __builtin_amdgcn_exp2f((mp - mx) * kLog2e);
    lsum += a * pr[kHeadDim + 1];
    const f32x4 lo = *reinterpret_cast<const f32x4*>(pr + d0);
    const f32x4 hi = *reinterpret_cast<const f32x4*>(pr + d0 + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[e] += a * lo[e];
      acc[4 + e] += a * hi[e];
    }
  }
}

// One wave's partial into LDS: O^T register r of db is d = 16 db + 4 g + r of head col (col = lane & 15,
// g = lane >> 4); the barrier behind it is the caller's
__device__ __forceinline__ void store_partial(Partials& sm, int wave, int col, int g, const f32x4 (&o)[8], float m,
                                              float l) {
#pragma unroll
  for (int db = 0; db < 8; ++db) *reinterpret_cast<f32x4*>(&sm.o[wave][col][16 * db + 4 * g]) = o[db];
  if (g == 0) {
    sm.m[wave][col] = m;
    sm.l[wave][col] = l;
  }
}

inline bool attn_group_supported(int group) { return group == 1 || group == 2 || group == 4 || group == 8 || group == 16; }

// The throws of paged_decode_bf16 and paged_prefill_bf16: sizes, group, strides, alignment.  `rows` names
// what ld_q / ld_out step over ("sequence" or "token").
inline void check_paged_operands(const std::string& name, const char* rows, uintptr_t q, uintptr_t k_cache,
                                 uintptr_t v_cache, uintptr_t block_table, uintptr_t ctx_lens, uintptr_t out, int S,
                                 int Hq, int Hkv, int64_t ld_q, int64_t ld_out, int64_t ld_table) {
  if (S < 0 || Hq <= 0 || Hkv <= 0) throw std::runtime_error(name + ": negative or zero sizes");
  if (Hq % Hkv || !attn_group_supported(Hq / Hkv)) throw std::runtime_error(name + ": Hq / Hkv must be 1, 2, 4, 8 or 16");
  const int64_t slab = (int64_t)Hq * kHeadDim;
  if (ld_q < slab || ld_out < slab || ld_q % 8 || ld_out % 8)
    throw std::runtime_error(name + ": q / out " + rows + " strides must be >= Hq * 128 and multiples of 8 elements");
  if (ld_table < 0) throw std::runtime_error(name + ": negative block-table stride");
  if (q % 16 || out % 16 || k_cache % 16 || v_cache % 16)
    throw std::runtime_error(name + ": q / out / k_cache / v_cache must be 16-byte aligned");
  if (block_table % 4 || ctx_lens % 4) throw std::runtime_error(name + ": block_table / ctx_lens must be 4-byte aligned");
}

}  // namespace gs
