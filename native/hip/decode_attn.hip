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
//    allows): the compiler then needs 128 VGPRs and no AGPRs and spills nothing (124 while the walk
//    was this kernel's own body; as walk_blocks, shared with the split kernel, the instruction mix
//    is the same, the schedule and the allocation differ), where unbounded it took 150 + 32 for 2
//    waves per SIMD and measured slower at every context length.
//
// Split-KV ("flash-decoding"), for a few long sequences whose S * Hkv workgroups leave CUs idle (8
// sequences over 8 KV heads are 64 workgroups on 256 CUs, whatever the context): two plain launches
// on one stream, paged_decode_split_kernel and paged_decode_merge_kernel.
//
//  * the split kernel has one workgroup per (sequence, KV head, split p), blockIdx.x =
//    (s * Hkv + kvh) * kv_splits + p.  THE PARTITION RULE (part of the contract; the tests place
//    tokens by it): with nblk = ceil(ctx / 32) and bps = ceil(nblk / kv_splits), split p takes the
//    blocks [p * bps, min(nblk, (p + 1) * bps)) and is empty where p * bps >= nblk.  Inside its
//    range the workgroup is paged_decode_kernel -- the same function, walk_blocks below, with the
//    range as arguments: waves round-robin over the range, table positions clamped to the range's
//    last block (so no entry at or beyond ceil(ctx / 32) is read), the masked slots past ctx in the
//    sequence's last block, the merge of the four waves through LDS (merge_waves).  It does not
//    divide: per head of the group it writes a row of kPartLd = 132 fp32 to the workspace, row
//    (s * Hq + h) * kv_splits + p: the 128 accumulators sum_w a_w O_w, then m = max_w m_w and
//    l = sum_w a_w l_w (two words of padding keep the rows 16-byte aligned; they are never read).
//    An empty split writes zeros, m = -inf and l = 0 like any other: every word the merge reads
//    has been written by this launch;
//  * the merge kernel has 16 threads per (sequence, head), 8 consecutive d each, and combines the
//    kv_splits rows with the formula of merge_waves: weight 0 where m_p == -inf, else
//    exp2((m_p - max m) * log2 e); lsum == 0 ? +0.0 : acc / lsum; one bf16 rounding.  One more
//    fp32 merge level, the same division, the same single rounding: ctx == 0 gives +0.0 and the
//    NaN rule of the unsplit kernel carries over.
//
// No bounds checks here by design: the host wrapper (ops/loadgen.py paged_decode_attention)
// validates shapes, strides and alignment, and on request ctx_lens and the block ids.
#include <type_traits>

#include "api.h"
#include "paged_attn.h"

namespace gs {
namespace {

// The walk of one workgroup over the blocks [blk_lo, blk_hi) of sequence s (ctx tokens) for KV head
// kvh: the whole sequence for paged_decode_kernel, one split's range for paged_decode_split_kernel.
// Leaves each wave's partial (O, m, l) in sm, behind a barrier.  Only block ceil(ctx / 32) - 1 can
// have slots past ctx, and it is the last block of the one range that holds it.
__device__ __forceinline__ void walk_blocks(Partials& sm, const __bf16* __restrict__ q,
                                            const __bf16* __restrict__ k_cache, const __bf16* __restrict__ v_cache,
                                            const int* __restrict__ block_table, int s, int kvh, int ctx, int blk_lo,
                                            int blk_hi, int group, int Hkv, size_t ld_q, size_t ld_table, float scale) {
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
    const int last = blk_hi - 1;
    constexpr size_t kSlab = (size_t)kBlockTokens * kHeadDim;        // one (block, KV head) of K or V
    // the lane's place in a slab
    const __bf16* klane = k_cache + (size_t)(8 * (col >> 2) + (col & 3)) * kHeadDim + 8 * g;
    const __bf16* vlane = v_cache + (size_t)col * kBlockTokens + 8 * g;
    int b = blk_lo + wave;
    size_t slab = ((size_t)trow[b] * Hkv + kvh) * kSlab;
    // table positions past the range's last block are clamped to it: every id load is
    // unconditional and reads an entry that names a block
    int next_id = trow[min(b + kWaves, last)];
    bf16x8 kf[2][4];
    KvBf16::load_k(kf, klane + slab);
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
        KvBf16::load_k(kn, klane + slab);
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
    for (; b + kWaves < blk_hi; b += kWaves) step(std::true_type{});
    step(std::false_type{});
    l += __shfl_xor(l, 16, kWave);
    l += __shfl_xor(l, 32, kWave);
  }

  store_partial(sm, wave, col, g, o, m, l);
  __syncthreads();
}

__global__ void __launch_bounds__(256, 4) paged_decode_kernel(const __bf16* __restrict__ q,
                                                           const __bf16* __restrict__ k_cache,
                                                           const __bf16* __restrict__ v_cache,
                                                           const int* __restrict__ block_table,
                                                           const int* __restrict__ ctx_lens,
                                                           __bf16* __restrict__ out, int Hq, int Hkv, size_t ld_q,
                                                           size_t ld_out, size_t ld_table, float scale) {
  __shared__ Partials sm;
  const int tid = threadIdx.x;
  const int s = blockIdx.x / Hkv, kvh = blockIdx.x % Hkv;
  const int group = Hq / Hkv;
  const int ctx = ctx_lens[s];
  const int nblk = (ctx + kBlockTokens - 1) / kBlockTokens;
  walk_blocks(sm, q, k_cache, v_cache, block_table, s, kvh, ctx, 0, nblk, group, Hkv, ld_q, ld_table, scale);

  // merge: thread (head c, 8 consecutive d)
  const int c = tid >> 4, d0 = (tid & 15) * 8;
  if (c < group) {
    float acc[8], mx, lsum;
    merge_waves(sm, c, d0, acc, mx, lsum);
    *reinterpret_cast<bf16x8*>(out + (size_t)s * ld_out + (size_t)(kvh * group + c) * kHeadDim + d0) =
        normalised(acc, lsum);
  }
}

// One split of one (sequence, KV head): the blocks the partition rule in the header gives it, walked
// and merged like paged_decode_kernel's, written undivided to the workspace.
__global__ void __launch_bounds__(256, 4) paged_decode_split_kernel(
    const __bf16* __restrict__ q, const __bf16* __restrict__ k_cache, const __bf16* __restrict__ v_cache,
    const int* __restrict__ block_table, const int* __restrict__ ctx_lens, float* __restrict__ workspace, int Hq,
    int Hkv, int kv_splits, size_t ld_q, size_t ld_table, float scale) {
  __shared__ Partials sm;
  const int tid = threadIdx.x;
  const int p = blockIdx.x % kv_splits, sk = blockIdx.x / kv_splits;
  const int s = sk / Hkv, kvh = sk % Hkv;
  const int group = Hq / Hkv;
  const int ctx = ctx_lens[s];
  const int nblk = (ctx + kBlockTokens - 1) / kBlockTokens;
  const int bps = (nblk + kv_splits - 1) / kv_splits;
  const int blk_lo = min(p * bps, nblk), blk_hi = min((p + 1) * bps, nblk);          // empty: lo == hi
  walk_blocks(sm, q, k_cache, v_cache, block_table, s, kvh, ctx, blk_lo, blk_hi, group, Hkv, ld_q, ld_table, scale);

  const int c = tid >> 4, d0 = (tid & 15) * 8;
  if (c < group) {
    float acc[8], mx, lsum;
    merge_waves(sm, c, d0, acc, mx, lsum);           // an empty split: zeros, m = -inf, l = 0
    float* row = workspace + (((size_t)s * Hq + kvh * group + c) * kv_splits + p) * kPartLd;
    store_split_row(row, d0, acc, mx, lsum);
  }
}

// The kv_splits partials of each (sequence, head) into out: thread (row = s * Hq + h, 8 consecutive
// d), 16 rows per workgroup.  The formula is merge_waves' and normalised()'s, over splits.
__global__ void __launch_bounds__(256) paged_decode_merge_kernel(const float* __restrict__ workspace,
                                                                 __bf16* __restrict__ out, int rows, int Hq,
                                                                 int kv_splits, size_t ld_out) {
  const int row = blockIdx.x * 16 + (threadIdx.x >> 4), d0 = (threadIdx.x & 15) * 8;
  if (row >= rows) return;
  const float ninf = -__builtin_inff();
  const float* part = workspace + (size_t)row * kv_splits * kPartLd;
  float mx = ninf;
#pragma unroll 4
  for (int p = 0; p < kv_splits; ++p) mx = fmaxf(mx, part[(size_t)p * kPartLd + kHeadDim]);
  float acc[8], lsum = 0.f;
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
  const int s = row / Hq, h = row % Hq;
  *reinterpret_cast<bf16x8*>(out + (size_t)s * ld_out + (size_t)h * kHeadDim + d0) = normalised(acc, lsum);
}

}  // namespace

int paged_decode_workgroups(int S, int Hkv) { return S * Hkv; }

int paged_decode_split_workgroups(int S, int Hkv, int kv_splits) { return S * Hkv * kv_splits; }

size_t paged_decode_split_workspace_floats(int S, int Hq, int kv_splits) {
  return (size_t)S * Hq * kv_splits * kPartLd;
}

void paged_decode_split_bf16(uintptr_t q, uintptr_t k_cache, uintptr_t v_cache, uintptr_t block_table,
                             uintptr_t ctx_lens, uintptr_t workspace, uintptr_t out, int S, int Hq, int Hkv,
                             int kv_splits, int64_t ld_q, int64_t ld_out, int64_t ld_table, float scale,
                             uintptr_t stream) {
  check_paged_operands("paged_decode_split", "sequence", q, k_cache, v_cache, block_table, ctx_lens, out, S, Hq, Hkv,
                       ld_q, ld_out, ld_table);
  if (kv_splits < 2 || kv_splits > kMaxKvSplits)
    throw std::runtime_error("paged_decode_split: kv_splits must be in [2, " + std::to_string(kMaxKvSplits) + "]");
  if (workspace % 16) throw std::runtime_error("paged_decode_split: workspace must be 16-byte aligned");
  if ((int64_t)S * Hkv * kv_splits >= (int64_t)1 << 31 || (int64_t)S * Hq >= (int64_t)1 << 31)
    throw std::runtime_error("paged_decode_split: more than 2^31 - 1 workgroups");
  if (S == 0) return;
  if (!workspace) throw std::runtime_error("paged_decode_split: no workspace");
  hipLaunchKernelGGL(paged_decode_split_kernel, dim3(paged_decode_split_workgroups(S, Hkv, kv_splits)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const __bf16*>(q),
                     reinterpret_cast<const __bf16*>(k_cache), reinterpret_cast<const __bf16*>(v_cache),
                     reinterpret_cast<const int*>(block_table), reinterpret_cast<const int*>(ctx_lens),
                     reinterpret_cast<float*>(workspace), Hq, Hkv, kv_splits, (size_t)ld_q, (size_t)ld_table, scale);
  HIP_CHECK(hipGetLastError());
  const int rows = S * Hq;
  hipLaunchKernelGGL(paged_decode_merge_kernel, dim3((rows + 15) / 16), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const float*>(workspace),
                     reinterpret_cast<__bf16*>(out), rows, Hq, kv_splits, (size_t)ld_out);
  HIP_CHECK(hipGetLastError());
}

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
