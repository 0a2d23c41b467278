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
