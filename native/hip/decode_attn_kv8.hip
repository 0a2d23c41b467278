// Paged-KV decode attention over an FP8 cache (gfx950 / MI355X): decode_attn.hip's two kernels and its merge
// with K and V stored as OCP e4m3fn bytes and one fp32 scale per KV head (THE FP8 KV FORMAT, api.h) -- half the
// bytes of a kernel that runs at the HBM roofline.
//
//   scores[t]   = (scale * k_scale[g]) * sum_d q[s,h,d] * e4m3(K[token t of s, g, d])      g = h / (Hq/Hkv)
//   out[s,h,:]  = bf16_rne( (sum_t softmax(scores)[t] * e4m3(V[token t of s, g, :])) * v_scale[g] )
//
// e4m3fn -> bf16 is exact (every one of the 254 non-NaN codes has at most 4 significant bits and an exponent
// inside bf16's range, subnormals included; 0x7F and 0xFF are the NaNs), so the bytes are converted in
// registers just before use -- v_cvt_pk_f32_fp8, two bytes to two floats, then v_cvt_pk_bf16_f32 -- and both
// products stay v_mfma_f32_16x16x32_bf16 with fp32 accumulation: the arithmetic is the bf16 kernel's on the
// dequantised codes, the two scales factored out of the sums.  What is as in decode_attn.hip (read its header):
// one 256-thread workgroup per (sequence, KV head) or per (sequence, KV head, split), four waves round-robin
// over the blocks, the token <-> row map of the S^T tiles (lane (col, g) ends up with tokens 8 g .. 8 g + 7 of
// head col), the online softmax in registers, P packed to bf16 as the B fragment of O^T = V^T . P, the masked
// slots past ctx in the sequence's last block, the clamped table reads, the next block's K requested behind
// the current block's V, the LDS merge (paged_attn.h), THE PARTITION RULE and the 132-float workspace rows.
// What differs:
//
//  * a K row is 128 bytes.  Lane (col, g) loads, for its token of tile t, the two 16-byte pieces
//    d = 64 h + 16 g .. + 15 (h = 0, 1): one load instruction of a wave covers 16 rows x 64 contiguous bytes.
//    k-step kk = 2 h + e of the S^T MFMAs takes bytes 8 e .. 8 e + 7 of piece h, i.e. d = 64 h + 16 g + 8 e + j
//    for the fragment's element j -- a permutation of the bf16 kernel's d = 32 kk + 8 g + j, and the Q^T fragments
//    are loaded by the same map, so every (q[d], K[d]) pair still meets once.  4 loads of 16 bytes per block and
//    lane instead of 8;
//  * a V row (one d, 32 tokens) is 32 bytes; the A fragment of O^T (row d = 16 db + col, tokens 8 g .. 8 g + 7)
//    is one 8-byte load, a wave covering 16 rows = 512 contiguous bytes.  8 loads of 8 bytes;
//  * scale and k_scale[g] are multiplied once in fp32 and that product multiplies the fp32 scores; v_scale[g]
//    multiplies the quotient acc / lsum (one fp32 multiply, then the single bf16 rounding).  The split kernel
//    writes partials unscaled by v_scale; the merge kernel applies it;
//  * a NaN byte inside ctx follows the bf16 kernel's NaN rule; past ctx it is masked like any other value (the
//    scores by a select, the V bytes by an AND to 0x00 = +0.0 before the conversion).
//
// No bounds checks here by design: the host wrapper (ops/loadgen.py paged_decode_attention_kv8) validates shapes,
// strides and alignment, and on request ctx_lens, the block ids and the scales.
#include <type_traits>

#include "api.h"
#include "paged_attn.h"

namespace gs {
namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// 8 e4m3fn bytes (lo: elements 0 .. 3, hi: 4 .. 7, element j in bits 8 j of its word) as 8 bf16, exactly
__device__ __forceinline__ bf16x8 fp8x8_to_bf16(unsigned lo, unsigned hi) {
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
  const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
  bf16x8 r;
  r[0] = (__bf16)a[0];
  r[1] = (__bf16)a[1];
  r[2] = (__bf16)b[0];
  r[3] = (__bf16)b[1];
  r[4] = (__bf16)c[0];
  r[5] = (__bf16)c[1];
  r[6] = (__bf16)d[0];
  r[7] = (__bf16)d[1];
  return r;
}

// walk_blocks of decode_attn.hip over byte caches; sscale = scale * k_scale[kvh]
__device__ __forceinline__ void walk_blocks_kv8(Partials& sm, const __bf16* __restrict__ q,
                                                const uint8_t* __restrict__ k_cache,
                                                const uint8_t* __restrict__ v_cache,
                                                const int* __restrict__ block_table, int s, int kvh, int ctx,
                                                int blk_lo, int blk_hi, int group, int Hkv, size_t ld_q,
                                                size_t ld_table, float sscale) {
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int col = lane & 15, g = lane >> 4;
  const float ninf = -__builtin_inff();

  float m = ninf, l = 0.f;
  f32x4 o[8];
#pragma unroll
  for (int db = 0; db < 8; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (blk_lo + wave < blk_hi) {
    // Q^T fragments: head col of the group, k-step kk = 2 h + e is d = 64 h + 16 g + 8 e .. + 7; zero columns
    // past the group
    bf16x8 qf[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) qf[kk] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (col < group) {
      const __bf16* qp = q + (size_t)s * ld_q + (size_t)(kvh * group + col) * kHeadDim + 16 * g;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) qf[kk] = *reinterpret_cast<const bf16x8*>(qp + (kk >> 1) * 64 + (kk & 1) * 8);
    }
    const int* trow = block_table + (size_t)s * ld_table;
    const int last = blk_hi - 1;
    constexpr size_t kSlab = (size_t)kBlockTokens * kHeadDim;        // bytes of one (block, KV head) of K or V
    // the lane's place in a slab
    const uint8_t* klane = k_cache + (size_t)(8 * (col >> 2) + (col & 3)) * kHeadDim + 16 * g;
    const uint8_t* vlane = v_cache + (size_t)col * kBlockTokens + 8 * g;
    int b = blk_lo + wave;
    size_t slab = ((size_t)trow[b] * Hkv + kvh) * kSlab;
    int next_id = trow[min(b + kWaves, last)];
    u32x4 kf[2][2];
    KvFp8::load_k(kf, klane + slab);
    auto step = [&](auto more_c) {
      constexpr bool more = decltype(more_c)::value;
      u32x2 vb[8];
#pragma unroll
      for (int db = 0; db < 8; ++db)
        vb[db] = *reinterpret_cast<const u32x2*>(vlane + slab + (size_t)db * 16 * kBlockTokens);
      u32x4 kn[2][2];
      if constexpr (more) {
        slab = ((size_t)next_id * Hkv + kvh) * kSlab;
        KvFp8::load_k(kn, klane + slab);
        next_id = trow[min(b + 2 * kWaves, last)];
      }
      // S^T = K . Q^T
      f32x4 sc[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        sc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const u32x4 w = kf[t][kk >> 1];
          const bf16x8 ka = (kk & 1) ? fp8x8_to_bf16(w[2], w[3]) : fp8x8_to_bf16(w[0], w[1]);
          sc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka, qf[kk], sc[t], 0, 0, 0);
        }
      }
      float sv[8];                                 // tokens 8 g .. 8 g + 7 of the block, head col
#pragma unroll
      for (int i = 0; i < 8; ++i) sv[i] = sc[i >> 2][i & 3] * sscale;
      if constexpr (!more) {
        const int valid = ctx - b * kBlockTokens;  // < 32 only in the sequence's last block
        if (valid < kBlockTokens) {
#pragma unroll
          for (int i = 0; i < 8; ++i) sv[i] = 8 * g + i >= valid ? ninf : sv[i];
          // the lane's bytes past ctx become 0x00, +0.0: byte i of the pair of words is token 8 g + i
          const int keep = min(max(valid - 8 * g, 0), 8);
          const unsigned mlo = keep >= 4 ? ~0u : (1u << (8 * keep)) - 1u;
          const unsigned mhi = keep >= 8 ? ~0u : keep <= 4 ? 0u : (1u << (8 * (keep - 4))) - 1u;
#pragma unroll
          for (int db = 0; db < 8; ++db) vb[db] = u32x2{vb[db][0] & mlo, vb[db][1] & mhi};
        }
      }
      float mb = fmaxf(fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3])), fmaxf(fmaxf(sv[4], sv[5]), fmaxf(sv[6], sv[7])));
      mb = fmaxf(mb, __shfl_xor(mb, 16, kWave));
      mb = fmaxf(mb, __shfl_xor(mb, 32, kWave));
      const float mn = fmaxf(m, mb);               // finite: the block has at least one token inside ctx
      const float alpha = __builtin_amdgcn_exp2f((m - mn) * kLog2e);      // m = -inf at first: 0
      m = mn;
      bf16x8 pf;
      float ps = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float p = __builtin_amdgcn_exp2f((sv[i] - mn) * kLog2e);
        ps += p;
        pf[i] = (__bf16)p;
      }
      l = l * alpha + ps;                          // this lane's 8 tokens; the 4 lane groups are added at the end
      // O^T = alpha O^T + V^T . P
#pragma unroll
      for (int db = 0; db < 8; ++db) {
        o[db] *= alpha;
        o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fp8x8_to_bf16(vb[db][0], vb[db][1]), pf, o[db], 0, 0, 0);
      }
      if constexpr (more) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int h = 0; h < 2; ++h) kf[t][h] = kn[t][h];
      }
    };
    for (; b + kWaves < blk_hi; b += kWaves) step(std::true_type{});
    step(std::false_type{});
    l += __shfl_xor(l, 16, kWave);
    l += __shfl_xor(l, 32, kWave);
  }

  store_partial(sm, wave, col, g, o, m, l);
  __syncthreads();
}

__global__ void __launch_bounds__(256, 4) paged_decode_kv8_kernel(
    const __bf16* __restrict__ q, const uint8_t* __restrict__ k_cache, const uint8_t* __restrict__ v_cache,
    const float* __restrict__ k_scale, const float* __restrict__ v_scale, const int* __restrict__ block_table,
    const int* __restrict__ ctx_lens, __bf16* __restrict__ out, int Hq, int Hkv, size_t ld_q, size_t ld_out,
    size_t ld_table, float scale) {
  __shared__ Partials sm;
  const int tid = threadIdx.x;
  const int s = blockIdx.x / Hkv, kvh = blockIdx.x % Hkv;
  const int group = Hq / Hkv;
  const int ctx = ctx_lens[s];
  const int nblk = (ctx + kBlockTokens - 1) / kBlockTokens;
  walk_blocks_kv8(sm, q, k_cache, v_cache, block_table, s, kvh, ctx, 0, nblk, group, Hkv, ld_q, ld_table,
                  __fmul_rn(scale, k_scale[kvh]));

  // merge: thread (head c, 8 consecutive d)
  const int c = tid >> 4, d0 = (tid & 15) * 8;
  if (c < group) {
    float acc[8], mx, lsum;
    merge_waves(sm, c, d0, acc, mx, lsum);
    *reinterpret_cast<bf16x8*>(out + (size_t)s * ld_out + (size_t)(kvh * group + c) * kHeadDim + d0) =
        normalised(acc, lsum, v_scale[kvh]);
  }
}

// One split of one (sequence, KV head), written undivided and unscaled by v_scale to the workspace
__global__ void __launch_bounds__(256, 4) paged_decode_split_kv8_kernel(
    const __bf16* __restrict__ q, const uint8_t* __restrict__ k_cache, const uint8_t* __restrict__ v_cache,
    const float* __restrict__ k_scale, const int* __restrict__ block_table, const int* __restrict__ ctx_lens,
    float* __restrict__ workspace, int Hq, int Hkv, int kv_splits, size_t ld_q, size_t ld_table, float scale) {
  __shared__ Partials sm;
  const int tid = threadIdx.x;
  const int p = blockIdx.x % kv_splits, sk = blockIdx.x / kv_splits;
  const int s = sk / Hkv, kvh = sk % Hkv;
  const int group = Hq / Hkv;
  const int ctx = ctx_lens[s];
  const int nblk = (ctx + kBlockTokens - 1) / kBlockTokens;
  const int bps = (nblk + kv_splits - 1) / kv_splits;
  const int blk_lo = min(p * bps, nblk), blk_hi = min((p + 1) * bps, nblk);          // empty: lo == hi
  walk_blocks_kv8(sm, q, k_cache, v_cache, block_table, s, kvh, ctx, blk_lo, blk_hi, group, Hkv, ld_q, ld_table,
                  __fmul_rn(scale, k_scale[kvh]));

  const int c = tid >> 4, d0 = (tid & 15) * 8;
  if (c < group) {
    float acc[8], mx, lsum;
    merge_waves(sm, c, d0, acc, mx, lsum);           // an empty split: zeros, m = -inf, l = 0
    store_split_row(workspace + (((size_t)s * Hq + kvh * group + c) * kv_splits + p) * kPartLd, d0, acc, mx, lsum);
  }
}

// paged_decode_merge_kernel with the V scale of the row's KV head on the quotient
__global__ void __launch_bounds__(256) paged_decode_merge_kv8_kernel(const float* __restrict__ workspace,
                                                                     const float* __restrict__ v_scale,
                                                                     __bf16* __restrict__ out, int rows, int Hq,
                                                                     int group, int kv_splits, size_t ld_out) {
  const int row = blockIdx.x * 16 + (threadIdx.x >> 4), d0 = (threadIdx.x & 15) * 8;
  if (row >= rows) return;
  float acc[8], lsum;
  merge_splits(workspace, row, kv_splits, d0, acc, lsum);
  const int s = row / Hq, h = row % Hq;
  *reinterpret_cast<bf16x8*>(out + (size_t)s * ld_out + (size_t)h * kHeadDim + d0) =
      normalised(acc, lsum, v_scale[h / group]);
}

}  // namespace

void paged_decode_kv8(uintptr_t q, uintptr_t k_cache, uintptr_t v_cache, uintptr_t k_scale, uintptr_t v_scale,
                      uintptr_t block_table, uintptr_t ctx_lens, uintptr_t out, int S, int Hq, int Hkv, int64_t ld_q,
                      int64_t ld_out, int64_t ld_table, float scale, uintptr_t stream) {
  check_paged_operands("paged_decode_kv8", "sequence", q, k_cache, v_cache, block_table, ctx_lens, out, S, Hq, Hkv,
                       ld_q, ld_out, ld_table);
  check_scales("paged_decode_kv8", k_scale, v_scale);
  if ((int64_t)S * Hkv >= (int64_t)1 << 31) throw std::runtime_error("paged_decode_kv8: more than 2^31 - 1 workgroups");
  if (S == 0) return;
  hipLaunchKernelGGL(paged_decode_kv8_kernel, dim3(paged_decode_workgroups(S, Hkv)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const __bf16*>(q),
                     reinterpret_cast<const uint8_t*>(k_cache), reinterpret_cast<const uint8_t*>(v_cache),
                     reinterpret_cast<const float*>(k_scale), reinterpret_cast<const float*>(v_scale),
                     reinterpret_cast<const int*>(block_table), reinterpret_cast<const int*>(ctx_lens),
                     reinterpret_cast<__bf16*>(out), Hq, Hkv, (size_t)ld_q, (size_t)ld_out, (size_t)ld_table, scale);
  HIP_CHECK(hipGetLastError());
}

void paged_decode_split_kv8(uintptr_t q, uintptr_t k_cache, uintptr_t v_cache, uintptr_t k_scale, uintptr_t v_scale,
                            uintptr_t block_table, uintptr_t ctx_lens, uintptr_t workspace, uintptr_t out, int S,
                            int Hq, int Hkv, int kv_splits, int64_t ld_q, int64_t ld_out, int64_t ld_table,
                            float scale, uintptr_t stream) {
  check_paged_operands("paged_decode_split_kv8", "sequence", q, k_cache, v_cache, block_table, ctx_lens, out, S, Hq,
                       Hkv, ld_q, ld_out, ld_table);
  check_scales("paged_decode_split_kv8", k_scale, v_scale);
  if (kv_splits < 2 || kv_splits > kMaxKvSplits)
    throw std::runtime_error("paged_decode_split_kv8: kv_splits must be in [2, " + std::to_string(kMaxKvSplits) + "]");
  if (workspace % 16) throw std::runtime_error("paged_decode_split_kv8: workspace must be 16-byte aligned");
  if ((int64_t)S * Hkv * kv_splits >= (int64_t)1 << 31 || (int64_t)S * Hq >= (int64_t)1 << 31)
    throw std::runtime_error("paged_decode_split_kv8: more than 2^31 - 1 workgroups");
  if (S == 0) return;
  if (!workspace) throw std::runtime_error("paged_decode_split_kv8: no workspace");
  hipLaunchKernelGGL(paged_decode_split_kv8_kernel, dim3(paged_decode_split_workgroups(S, Hkv, kv_splits)), dim3(256),
                     0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const __bf16*>(q),
                     reinterpret_cast<const uint8_t*>(k_cache), reinterpret_cast<const uint8_t*>(v_cache),
                     reinterpret_cast<const float*>(k_scale), reinterpret_cast<const int*>(block_table),
                     reinterpret_cast<const int*>(ctx_lens), reinterpret_cast<float*>(workspace), Hq, Hkv, kv_splits,
                     (size_t)ld_q, (size_t)ld_table, scale);
  HIP_CHECK(hipGetLastError());
  const int rows = S * Hq;
  hipLaunchKernelGGL(paged_decode_merge_kv8_kernel, dim3((rows + 15) / 16), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const float*>(workspace),
                     reinterpret_cast<const float*>(v_scale), reinterpret_cast<__bf16*>(out), rows, Hq, Hq / Hkv,
                     kv_splits, (size_t)ld_out);
  HIP_CHECK(hipGetLastError());
}

}  // namespace gs
