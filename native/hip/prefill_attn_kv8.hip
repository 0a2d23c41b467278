// Paged-KV prefill (append) attention over an FP8 cache (gfx950 / MI355X): prefill_attn.hip's kernel with K and V
// stored as OCP e4m3fn bytes and one fp32 scale per KV head (THE FP8 KV FORMAT, api.h).
//
//   p            = ctx[s] - q_len[s] + i                                                     g = h / (Hq/Hkv)
//   scores[t]    = (scale * k_scale[g]) * sum_d q[row,h,d] * e4m3(K[token t of s, g, d])     t in [0, p]
//   out[row,h,:] = bf16_rne( ((sum_t softmax(scores)[t] * e4m3(V[t, g, :])) / l) * v_scale[g] )
//
// What is as in prefill_attn.hip (read its header): the grid (paged_prefill_workgroups, heavy tiles first), one
// 256-thread workgroup per (sequence, KV head, tile of 128 columns), four waves of two 16-column MFMA tiles each
// with no cross-wave merge, the token <-> row map of the S^T tiles, causal skipping per wave, the mask-free /
// masked / last-block split in one loop with wave-uniform branches, the clamped table reads, the rescale only
// where some maximum rose, the fp32 softmax with l summed from the fp32 probabilities and P rounded to bf16, one
// IEEE division at the end, 64-bit addresses, no LDS, no barrier.  What is as in decode_attn_kv8.hip (read its
// header): the 16-byte K pieces under the permuted d map d = 64 h + 16 g + 8 e + j with the Q^T fragments loaded
// by the same map (4 K loads per block and lane), the 8-byte V loads (8 per block and lane), scale * k_scale[g]
// multiplied once in fp32, v_scale[g] on the quotient, the V bytes past ctx ANDed to 0x00 before the conversion
// and the scores there set to -inf by a select.  What differs from both:
//
//  * this kernel is MFMA-bound, so the byte -> bf16 conversion sits beside the bottleneck.  Every K and every V
//    fragment is converted once per block and feeds the MFMAs of both column tiles: the MFMA loops have the
//    column tile innermost (prefill_attn.hip's O^T product is tile-outer), so both tiles' softmax is done before
//    the first O^T MFMA.  16 fragment conversions against 32 MFMAs per block and wave;
//  * the conversion is v_cvt_scalef32_pk_bf16_fp8 with scale 1.0: one instruction per two elements, 4 per
//    fragment, where decode_attn_kv8.hip's v_cvt_pk_f32_fp8 + v_cvt_pk_bf16_f32 pair takes 8.  It is exact on
//    all 254 finite codes and keeps the NaNs NaN (tests/test_gpu_prefill_kv8_exact.py, all codes);
//  * the byte fragments are half the registers of the bf16 kernel's: 4 + 8 loads hold 32 VGPRs, not 64.
//
//  * 184 VGPRs, no AGPRs, no LDS, nothing spilled, 2 waves per SIMD (profiles/r18_prefill_kv8).
//
// No bounds checks here by design: the host wrapper (ops/loadgen.py paged_prefill_attention_kv8) validates
// shapes, strides and alignment, and on request ctx_lens, q_start, the block ids and the scales.
#include "api.h"
#include "paged_attn.h"

namespace gs {
namespace {

constexpr int kColTiles = 2;                              // MFMA column tiles per wave
constexpr int kWaveColumns = 16 * kColTiles;
constexpr int kColumns = kWaves * kWaveColumns;           // query columns per workgroup, prefill_attn.hip's

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// 8 e4m3fn bytes (lo: elements 0 .. 3, hi: 4 .. 7, element j in bits 8 j of its word) as 8 bf16, exactly
__device__ __forceinline__ bf16x8 fp8x8_to_bf16(unsigned lo, unsigned hi) {
  const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false);
  const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
  const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false);
  const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
  return bf16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

__global__ void __launch_bounds__(256, 2) paged_prefill_kv8_kernel(
    const __bf16* __restrict__ q, const uint8_t* __restrict__ k_cache, const uint8_t* __restrict__ v_cache,
    const float* __restrict__ k_scale, const float* __restrict__ v_scale, const int* __restrict__ block_table,
    const int* __restrict__ ctx_lens, const int* __restrict__ q_start, __bf16* __restrict__ out, int S, int Hq,
    int Hkv, size_t ld_q, size_t ld_out, size_t ld_table, float scale) {
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  // heavy tiles first: the grid is [tile (descending)][sequence][KV head]
  const int per_tile = S * Hkv;
  const int tile = (int)(gridDim.x / per_tile) - 1 - (int)(blockIdx.x / per_tile);
  const int s = (blockIdx.x % per_tile) / Hkv, kvh = blockIdx.x % Hkv;
  const int group = Hq / Hkv;
  const int row0 = q_start[s];
  const int q_len = q_start[s + 1] - row0;
  const int64_t ncols = (int64_t)q_len * group;
  const int64_t c0 = (int64_t)tile * kColumns + wave * kWaveColumns;      // the wave's first column
  if (c0 >= ncols) return;
  const int ctx = ctx_lens[s];
  const float sscale = __fmul_rn(scale, k_scale[kvh]);
  const int col = lane & 15, g = lane >> 4;
  const float ninf = -__builtin_inff();
  const int p_base = ctx - q_len;                                          // position of chunk token 0
  const int64_t c_last = (c0 + kWaveColumns - 1 < ncols ? c0 + kWaveColumns - 1 : ncols - 1);
  const int p_min = p_base + (int)(c0 / group), p_max = p_base + (int)(c_last / group);
  const int last = p_max / kBlockTokens;                                   // the wave's last block
  const int nfull = (p_min + 1) / kBlockTokens;                            // blocks [0, nfull) need no mask

  // per column tile: this lane's column, whether the chunk has it, its position, its Q^T fragments (head h of
  // the group, k-step kk = 2 hh + e is d = 64 hh + 16 g + 8 e .. + 7; zero columns past the chunk, never stored)
  bool have[kColTiles];
  int pos[kColTiles];
  bf16x8 qf[kColTiles][4];
#pragma unroll
  for (int j = 0; j < kColTiles; ++j) {
    const int64_t c = c0 + 16 * j + col;
    have[j] = c < ncols;
    const int64_t cc = have[j] ? c : ncols - 1;
    const int i = (int)(cc / group), h = (int)(cc % group);
    pos[j] = p_base + i;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) qf[j][kk] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (have[j]) {
      const __bf16* qp = q + (size_t)(row0 + i) * ld_q + (size_t)(kvh * group + h) * kHeadDim + KvFp8::kLaneD * g;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) qf[j][kk] = *reinterpret_cast<const bf16x8*>(qp + KvFp8::q_offset(kk));
    }
  }

  float m[kColTiles], l[kColTiles];
  f32x4 o[kColTiles][8];
#pragma unroll
  for (int j = 0; j < kColTiles; ++j) {
    m[j] = ninf;
    l[j] = 0.f;
#pragma unroll
    for (int db = 0; db < 8; ++db) o[j][db] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const int* trow = block_table + (size_t)s * ld_table;
  constexpr size_t kSlab = (size_t)kBlockTokens * kHeadDim;                // bytes of one (block, KV head) of K or V
  // the lane's place in a slab
  const uint8_t* klane = k_cache + (size_t)(8 * (col >> 2) + (col & 3)) * kHeadDim + KvFp8::kLaneD * g;
  const uint8_t* vlane = v_cache + (size_t)col * kBlockTokens + 8 * g;
  int b = 0;
  size_t slab = ((size_t)trow[0] * Hkv + kvh) * kSlab;
  int next_id = trow[min(1, last)];
  KvFp8::KBlock kf;
  KvFp8::load_k(kf, klane + slab);

  // One loop with wave-uniform branches around the mask code, as in prefill_attn.hip
  for (; b <= last; ++b) {
    const bool masked = b >= nfull;                  // some token of the block lies above some column's position (or past ctx)
    KvFp8::VFrag vb[8];
#pragma unroll
    for (int db = 0; db < 8; ++db)
      vb[db] = *reinterpret_cast<const u32x2*>(vlane + slab + (size_t)db * 16 * kBlockTokens);
    // S^T = K . Q^T: each K fragment converted once, for both column tiles; that done, the K registers take the
    // next block's
    f32x4 sc[kColTiles][2];
#pragma unroll
    for (int j = 0; j < kColTiles; ++j)
#pragma unroll
      for (int t = 0; t < 2; ++t) sc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const u32x4 w = kf[t][kk >> 1];
        const bf16x8 ka = (kk & 1) ? fp8x8_to_bf16(w[2], w[3]) : fp8x8_to_bf16(w[0], w[1]);
#pragma unroll
        for (int j = 0; j < kColTiles; ++j)
          sc[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka, qf[j][kk], sc[j][t], 0, 0, 0);
      }
    __builtin_amdgcn_sched_barrier(0);
    slab = ((size_t)next_id * Hkv + kvh) * kSlab;
    KvFp8::load_k(kf, klane + slab);
    next_id = trow[min(b + 2, last)];
    __builtin_amdgcn_sched_barrier(0);
    const int tok0 = b * kBlockTokens + 8 * g;       // this lane's first token
    if (masked && (b + 1) * kBlockTokens > ctx) {    // the sequence's last block, not full
      // the lane's bytes past ctx become 0x00, +0.0: byte i of the pair of words is token tok0 + i
      const int keep = min(max(ctx - tok0, 0), 8);
      const unsigned mlo = keep >= 4 ? ~0u : (1u << (8 * keep)) - 1u;
      const unsigned mhi = keep >= 8 ? ~0u : keep <= 4 ? 0u : (1u << (8 * (keep - 4))) - 1u;
#pragma unroll
      for (int db = 0; db < 8; ++db) vb[db] = u32x2{vb[db][0] & mlo, vb[db][1] & mhi};
    }
    bf16x8 pf[kColTiles];
#pragma unroll
    for (int j = 0; j < kColTiles; ++j) {
      float sv[8];                                   // tokens tok0 .. tok0 + 7, this lane's column
      const int below = pos[j] - tok0;               // tokens tok0 + i with i > below lie above the column's position
#pragma unroll
      for (int i = 0; i < 8; ++i) sv[i] = sc[j][i >> 2][i & 3] * sscale;
      if (masked) {
#pragma unroll
        for (int i = 0; i < 8; ++i) sv[i] = i > below ? ninf : sv[i];
      }
      float mb = fmaxf(fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3])), fmaxf(fmaxf(sv[4], sv[5]), fmaxf(sv[6], sv[7])));
      mb = fmaxf(mb, __shfl_xor(mb, 16, kWave));
      mb = fmaxf(mb, __shfl_xor(mb, 32, kWave));
      const float mn = fmaxf(m[j], mb);              // finite: token 0 is at or below every position
      const float alpha = __builtin_amdgcn_exp2f((m[j] - mn) * kLog2e);   // m = -inf at first: 0
      m[j] = mn;
      float ps = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float p = __builtin_amdgcn_exp2f((sv[i] - mn) * kLog2e);
        ps += p;
        pf[j][i] = (__bf16)p;
      }
      l[j] = l[j] * alpha + ps;                      // this lane's 8 tokens; the 4 lane groups are added at the end
      // O^T = alpha O^T + V^T . P; alpha is exactly 1 in every column whose maximum stood
      if (__any(alpha != 1.f)) {
#pragma unroll
        for (int db = 0; db < 8; ++db) o[j][db] *= alpha;
      }
    }
    // each V fragment converted once, for both column tiles
#pragma unroll
    for (int db = 0; db < 8; ++db) {
      const bf16x8 va = fp8x8_to_bf16(vb[db][0], vb[db][1]);
#pragma unroll
      for (int j = 0; j < kColTiles; ++j) o[j][db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pf[j], o[j][db], 0, 0, 0);
    }
  }

  // O^T register r of db is d = 16 db + 4 g + r of the lane's column: 8-byte stores
  const float vs = v_scale[kvh];
#pragma unroll
  for (int j = 0; j < kColTiles; ++j) {
    float lj = l[j];
    lj += __shfl_xor(lj, 16, kWave);
    lj += __shfl_xor(lj, 32, kWave);
    if (have[j]) {
      typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
      const int64_t c = c0 + 16 * j + col;
      __bf16* orow = out + (size_t)(row0 + (int)(c / group)) * ld_out + (size_t)(kvh * group + (int)(c % group)) * kHeadDim;
#pragma unroll
      for (int db = 0; db < 8; ++db) {
        bf16x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = (__bf16)__fmul_rn(o[j][db][e] / lj, vs);
        *reinterpret_cast<bf16x4*>(orow + 16 * db + 4 * g) = r;
      }
    }
  }
}

}  // namespace

void paged_prefill_kv8(uintptr_t q, uintptr_t k_cache, uintptr_t v_cache, uintptr_t k_scale, uintptr_t v_scale,
                       uintptr_t block_table, uintptr_t ctx_lens, uintptr_t q_start, uintptr_t out, int S, int Hq,
                       int Hkv, int max_q_len, int64_t ld_q, int64_t ld_out, int64_t ld_table, float scale,
                       uintptr_t stream) {
  check_paged_operands("paged_prefill_kv8", "token", q, k_cache, v_cache, block_table, ctx_lens, out, S, Hq, Hkv, ld_q,
                       ld_out, ld_table);
  if (max_q_len < 0) throw std::runtime_error("paged_prefill_kv8: negative max_q_len");
  if (q_start % 4) throw std::runtime_error("paged_prefill_kv8: q_start must be 4-byte aligned");
  check_scales("paged_prefill_kv8", k_scale, v_scale);
  const int grid = paged_prefill_workgroups(S, Hq, Hkv, max_q_len);
  if (grid == 0) return;
  hipLaunchKernelGGL(paged_prefill_kv8_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const __bf16*>(q), reinterpret_cast<const uint8_t*>(k_cache),
                     reinterpret_cast<const uint8_t*>(v_cache), reinterpret_cast<const float*>(k_scale),
                     reinterpret_cast<const float*>(v_scale), reinterpret_cast<const int*>(block_table),
                     reinterpret_cast<const int*>(ctx_lens), reinterpret_cast<const int*>(q_start),
                     reinterpret_cast<__bf16*>(out), S, Hq, Hkv, (size_t)ld_q, (size_t)ld_out, (size_t)ld_table, scale);
  HIP_CHECK(hipGetLastError());
}

}  // namespace gs
