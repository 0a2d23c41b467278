// Paged-KV decode attention (gfx950 / MI355X): the LLM-serving decode phase.
//
//   scores[t]   = scale * sum_d q[s,h,d] * K[token t of s, h / (Hq/Hkv), d]        t in [0, ctx[s])
//   out[s,h,:]  = bf16_rne( sum_t softmax(scores)[t] * V[token t of s, h / (Hq/Hkv), :] )
//
// One new token per sequence, head dim 128, cache blocks of 32 tokens; token t of sequence s sits
// in physical block block_table[s, t / 32], slot t % 32.  k_cache is [NB, Hkv, 32, 128] (a token's
// row d-contiguous), v_cache [NB, Hkv, 128, 32] (token-contiguous, the transposed V of paged
// attention servers).  HBM-bound like the triad and the gather, but its traffic goes through a
// block table, its products run on the matrix cores and it has a softmax in the loop.  Shape of
// the kernel:
//
//  * one 256-thread workgroup per (sequence, KV head); its four waves take the sequence's blocks
//    round-robin, each with its own running maximum m, normaliser l and O, merged once through
//    LDS (33.5 KiB) at the end.  A wave that got no block has m = -inf and weight 0 in the merge;
//  * both products are v_mfma_f32_16x16x32_bf16 with the KV head's query heads as the 16 columns
//    (heads past Hq / Hkv are zero columns, never stored).  S^T = K . Q^T, two 16-token tiles per
//    block: row rho of tile t is token 8 (rho >> 2) + 4 t + (rho & 3), so the lane with head
//    lane & 15 ends up with tokens 8 g .. 8 g + 7 (g = lane >> 4) in order, registers r of tile t
//    being token 8 g + 4 t + r.  The maximum and the sum are 8 register operations and two
//    shuffles (xor 16, xor 32); the 8 probabilities, packed to bf16, ARE the B fragment of
//    O^T = V^T . P, whose A fragment (row d, tokens 8 g .. 8 g + 7) is one 16-byte load of the
//    token-contiguous V.  No LDS and no lane movement between the two products;
//  * scale multiplies the fp32 scores; the online softmax (running maximum), l (summed from the
//    fp32 probabilities) and O are fp32; only P is rounded to bf16 for the MFMA, and the output
//    once at the end.  ctx == 0 gives a row of +0.0;
//  * only a sequence's last block can have slots past ctx: their scores are replaced by -inf (a
//    select, so a NaN does not survive) and their V elements by zero (0 * NaN is NaN).  Table
//    entries at or beyond ceil(ctx / 32) are never read, nor any block the table does not name;
//  * the next block's K (8 loads of 16 bytes per lane) and the block id after it are requested
//    while the current block computes, behind the current block's V.  All addresses are 64-bit;
//  * the kernel is bounded to 128 registers (4 waves per SIMD, the 4 workgroups per CU its LDS
//    allows): the compiler then needs 124 VGPRs and no AGPRs and spills nothing, where unbounded
//    it took 150 + 32 for 2 waves per SIMD and measured slower at every context length.
//
// Not here: cross-workgroup split-KV.  A few long sequences (S * Hkv below the CU count) leave
// CUs idle; the load generator's decode batches are wide, so the grid fills the chip.
//
// No bounds checks here by design: the host wrapper (ops/loadgen.py paged_decode_attention)
// validates shapes, strides and alignment, and on request ctx_lens and the block ids.
#include <type_traits>

#include "api.h"
#include "paged_attn.h"

namespace gs {
namespace {

constexpr int kWaves = 4;
constexpr int kOLd = kHeadDim + 4;                // fp32 row of the LDS image: 528 bytes, 16-byte aligned

struct Partials {
  float o[kWaves][kMaxGroup][kOLd];
  float m[kWaves][kMaxGroup];
  float l[kWaves][kMaxGroup];
};

__global__ void __launch_bounds__(256, 4) paged_decode_kernel(const __bf16* __restrict__ q,
                                                           const __bf16* __restrict__ k_cache,
                                                           const __bf16* __restrict__ v_cache,
                                                           const int* __restrict__ block_table,
                                                           const int* __restrict__ ctx_lens,
                                                           __bf16* __restrict__ out, int Hq, int Hkv, size_t ld_q,
                                                           size_t ld_out, size_t ld_table, float scale) {
  __shared__ Partials sm;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int s = blockIdx.x / Hkv, kvh = blockIdx.x % Hkv;
  const int group = Hq / Hkv;
  const int col = lane & 15, g = lane >> 4;
  const int ctx = ctx_lens[s];
  const int nblk = (ctx + kBlockTokens - 1) / kBlockTokens;
  const float ninf = -__builtin_inff();

  float m = ninf, l = 0.f;
  f32x4 o[8];
#pragma unroll
  for (int db = 0; db < 8; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (wave < nblk) {
    // Q^T fragments: head col of the group, d = 32 kk + 8 g .. + 7; zero columns past the group
    bf16x8 qf[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) qf[kk] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (col < group) {
      const __bf16* qp = q + (size_t)s * ld_q + (size_t)(kvh * group + col) * kHeadDim + 8 * g;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) qf[kk] = *reinterpret_cast<const bf16x8*>(qp + kk * 32);
    }
    const int* trow = block_table + (size_t)s * ld_table;
    const int last = nblk - 1;
    constexpr size_t kSlab = (size_t)kBlockTokens * kHeadDim;        // one (block, KV head) of K or V
    // the lane's place in a slab
    const __bf16* klane = k_cache + (size_t)(8 * (col >> 2) + (col & 3)) * kHeadDim + 8 * g;
    const __bf16* vlane = v_cache + (size_t)col * kBlockTokens + 8 * g;
    int b = wave;
    size_t slab = ((size_t)trow[b] * Hkv + kvh) * kSlab;
    // table positions past the sequence's last block are clamped to it: every id load is
    // unconditional and reads an entry that names a block
    int next_id = trow[min(b + kWaves, last)];
    bf16x8 kf[2][4];
    load_k(kf, klane + slab);
    // one block.  more: another block of this wave follows -- its K and the id of the one after
    // are loaded behind this block's V, and it is a full block (only the sequence's last block,
    // which is its wave's last, can have slots past ctx); the two cases are separate code, so
    // the waits count the loads in flight exactly
    auto step = [&](auto more_c) {
      constexpr bool more = decltype(more_c)::value;
      bf16x8 vf[8];
#pragma unroll
      for (int db = 0; db < 8; ++db)
        vf[db] = *reinterpret_cast<const bf16x8*>(vlane + slab + (size_t)db * 16 * kBlockTokens);
      bf16x8 kn[2][4];
      if constexpr (more) {
        slab = ((size_t)next_id * Hkv + kvh) * kSlab;
        load_k(kn, klane + slab);
        next_id = trow[min(b + 2 * kWaves, last)];
      }
      // S^T = K . Q^T
      f32x4 sc[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        sc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) sc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t][kk], qf[kk], sc[t], 0, 0, 0);
      }
      float sv[8];                                 // tokens 8 g .. 8 g + 7 of the block, head col
#pragma unroll
      for (int i = 0; i < 8; ++i) sv[i] = sc[i >> 2][i & 3] * scale;
      if constexpr (!more) {
        const int valid = ctx - b * kBlockTokens;  // < 32 only in the sequence's last block
        if (valid < kBlockTokens) {
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const bool past = 8 * g + i >= valid;
            sv[i] = past ? ninf : sv[i];
#pragma unroll
            for (int db = 0; db < 8; ++db) {
              bf16x8_bits v = __builtin_bit_cast(bf16x8_bits, vf[db]);
              v[i] = past ? (short)0 : v[i];
              vf[db] = __builtin_bit_cast(bf16x8, v);
            }
          }
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
        o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[db], pf, o[db], 0, 0, 0);
      }
      if constexpr (more) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) kf[t][kk] = kn[t][kk];
      }
    };
    for (; b + kWaves < nblk; b += kWaves) step(std::true_type{});
    step(std::false_type{});
    l += __shfl_xor(l, 16, kWave);
    l += __shfl_xor(l, 32, kWave);
  }

  // the wave's partial: O^T register r of db is d = 16 db + 4 g + r of head col
#pragma unroll
  for (int db = 0; db < 8; ++db) *reinterpret_cast<f32x4*>(&sm.o[wave][col][16 * db + 4 * g]) = o[db];
  if (g == 0) {
    sm.m[wave][col] = m;
    sm.l[wave][col] = l;
  }
  __syncthreads();

  // merge: thread (head c, 8 consecutive d) weighs the four partials by exp(m_w - max m)
  const int c = tid >> 4, d0 = (tid & 15) * 8;
  if (c < group) {
    float mw[kWaves], mx = ninf;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      mw[w] = sm.m[w][c];
      mx = fmaxf(mx, mw[w]);
    }
    float acc[8], lsum = 0.f;
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
    bf16x8 r;
    // lsum == 0 only for ctx == 0 (all four weights 0): +0.0.  A NaN normaliser divides: NaN out
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (__bf16)(lsum == 0.f ? 0.f : acc[e] / lsum);
    *reinterpret_cast<bf16x8*>(out + (size_t)s * ld_out + (size_t)(kvh * group + c) * kHeadDim + d0) = r;
  }
}

}  // namespace

int paged_decode_workgroups(int S, int Hkv) { return S * Hkv; }

void paged_decode_bf16(uintptr_t q, uintptr_t k_cache, uintptr_t v_cache, uintptr_t block_table, uintptr_t ctx_lens,
                       uintptr_t out, int S, int Hq, int Hkv, int64_t ld_q, int64_t ld_out, int64_t ld_table,
                       float scale, uintptr_t stream) {
  check_paged_operands("paged_decode", "sequence", q, k_cache, v_cache, block_table, ctx_lens, out, S, Hq, Hkv, ld_q,
                       ld_out, ld_table);
  if ((int64_t)S * Hkv >= (int64_t)1 << 31) throw std::runtime_error("paged_decode: more than 2^31 - 1 workgroups");
  if (S == 0) return;
  hipLaunchKernelGGL(paged_decode_kernel, dim3(paged_decode_workgroups(S, Hkv)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const __bf16*>(q),
                     reinterpret_cast<const __bf16*>(k_cache), reinterpret_cast<const __bf16*>(v_cache),
                     reinterpret_cast<const int*>(block_table), reinterpret_cast<const int*>(ctx_lens),
                     reinterpret_cast<__bf16*>(out), Hq, Hkv, (size_t)ld_q, (size_t)ld_out, (size_t)ld_table, scale);
  HIP_CHECK(hipGetLastError());
}

}  // namespace gs
