// What the paged-KV kernels (decode_attn.hip, decode_attn_kv8.hip, prefill_attn.hip, prefill_attn_kv8.hip,
// rope_append.hip) share: the fixed sizes of the cache layout, the MFMA fragment types, the two cache formats
// (bf16 and FP8) and the host-side operand checks of their launch functions.
#pragma once
#include <string>

#include "common.h"

namespace gs {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short bf16x8_bits __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int kHeadDim = 128;
constexpr int kBlockTokens = 32;
constexpr int kMaxGroup = 16;                     // the MFMA's column dimension
constexpr float kLog2e = 1.44269504088896340736f;

// The two cache formats, described once for the kernels that walk a cache (decode_attn.hip, decode_attn_kv8.hip,
// the two prefill kernels) or write one (rope_append.hip): the element type, the register images of a block's K
// and of one V fragment, where the lane's d starts in a row, which d the k-step kk of the S^T MFMAs multiplies,
// how a block's K is loaded, and whether the format has scales.  The byte -> bf16 conversion in front of an MFMA
// is NOT here: decode and prefill use different instructions on purpose, each file has its own.  Nor is the mask of
// the slots past ctx in a sequence's last block (for FP8 the byte AND with keep / mlo / mhi): it deliberately stays
// in each kernel's own loop, because as a function of the format the compiler's code for paged_prefill_kv8_kernel
// changed, and the decode walks are kept as they were (profiles/r19_kv_format).

// bf16: k_cache [NB, Hkv, 32, 128] and v_cache [NB, Hkv, 128, 32] of __bf16.  The lane holds d = 32 kk + 8 g
// .. + 7 of its token for k-step kk (8 loads of 16 bytes per block and lane) and, per V fragment, the tokens
// 8 g .. 8 g + 7 of one d (8 loads of 16 bytes)
struct KvBf16 {
  typedef __bf16 Elem;
  typedef bf16x8 KBlock[2][4];                    // [tile t][k-step kk]
  typedef bf16x8 VFrag;
  static constexpr bool kScales = false;
  static constexpr int kLaneD = 8;                // the lane's first d in a row is kLaneD * g
  static __device__ __forceinline__ int q_offset(int kk) { return 32 * kk; }

  // the 8 K fragments of one (block, KV head) slab: tile t, k-step kk is d = 32 kk + 8 g .. + 7 of
  // the lane's token 8 (rho >> 2) + 4 t + (rho & 3) -- p already points at the lane's place
  static __device__ __forceinline__ void load_k(KBlock& kf, const __bf16* p) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) kf[t][kk] = *reinterpret_cast<const bf16x8*>(p + t * 4 * kHeadDim + kk * 32);
  }
};

// FP8 (THE FP8 KV FORMAT, api.h): the same two layouts of OCP e4m3fn bytes, one fp32 scale per KV head.  A K row is
// 128 bytes: the lane loads the two 16-byte pieces d = 64 h + 16 g .. + 15 of its token, and k-step kk = 2 h + e
// takes bytes 8 e .. 8 e + 7 of piece h -- a permutation of bf16's d map under which the Q^T fragments are loaded
// too (q_offset), so every (q[d], K[d]) pair still meets once (decode_attn_kv8.hip's header has the argument).
// A V fragment is 8 bytes
struct KvFp8 {
  typedef uint8_t Elem;
  typedef u32x4 KBlock[2][2];                     // [tile t][piece h]: k-steps 2 h and 2 h + 1
  typedef u32x2 VFrag;
  static constexpr bool kScales = true;
  static constexpr int kLaneD = 16;
  static __device__ __forceinline__ int q_offset(int kk) { return 64 * (kk >> 1) + 8 * (kk & 1); }

  // the 4 K pieces of one (block, KV head) slab: tile t, piece h is d = 64 h + 16 g .. + 15 of the lane's token
  // 8 (rho >> 2) + 4 t + (rho & 3) -- p already points at the lane's place
  static __device__ __forceinline__ void load_k(KBlock& kf, const uint8_t* p) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int h = 0; h < 2; ++h) kf[t][h] = *reinterpret_cast<const u32x4*>(p + t * 4 * kHeadDim + h * 64);
  }
};

// What only the decode kernels (decode_attn.hip over a bf16 cache, decode_attn_kv8.hip over an FP8 one) share:
// the per-wave partials in LDS, their merge and the final division.
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

// The throws of every launch function over an FP8 cache: the two per-KV-head scale vectors
inline void check_scales(const std::string& name, uintptr_t k_scale, uintptr_t v_scale) {
  if (!k_scale || !v_scale) throw std::runtime_error(name + ": k_scale and v_scale are needed");
  if (k_scale % 4 || v_scale % 4) throw std::runtime_error(name + ": k_scale / v_scale must be 4-byte aligned");
}

}  // namespace gs
