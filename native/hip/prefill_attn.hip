// Paged-KV prefill (append) attention (gfx950 / MI355X): the LLM-serving prefill phase, chunked.
//
//   row         = q_start[s] + i,  i in [0, q_len[s]),  q_len[s] = q_start[s + 1] - q_start[s]
//   p           = ctx[s] - q_len[s] + i                            the query's position in its sequence
//   scores[t]   = scale * sum_d q[row,h,d] * K[token t of s, h / (Hq/Hkv), d]        t in [0, p]
//   out[row,h,:] = bf16_rne( sum_t softmax(scores)[t] * V[token t of s, h / (Hq/Hkv), :] )
//
// The cache is the decode kernel's (decode_attn.hip): head dim 128, blocks of 32 tokens, token t of
// sequence s in block block_table[s, t / 32], slot t % 32; k_cache [NB, Hkv, 32, 128], v_cache
// [NB, Hkv, 128, 32].  The chunk's own K / V are in the cache already (ctx counts them).  With every
// q_len == 1 this is the decode attention.  MFMA-bound where decode is HBM-bound: every K / V slab is
// used by all the chunk's queries of the KV head, and every MFMA sits behind v_exps, cross-lane maxima
// and a rescale of the accumulators.  Shape of the kernel:
//
//  * the decode kernel's orientation.  S^T = K . Q^T on v_mfma_f32_16x16x32_bf16: tokens are rows, a
//    tile has 16 query columns; column c of a (sequence, KV head) is chunk token c / group, head
//    c % group of the group.  Row rho of token tile t is token 8 (rho >> 2) + 4 t + (rho & 3), so the
//    lane of column lane & 15 holds tokens 8 g .. 8 g + 7 (g = lane >> 4) of the block in order; the
//    8 probabilities, packed to bf16, are the B fragment of O^T = V^T . P, whose A fragment (row d,
//    tokens 8 g .. 8 g + 7) is one 16-byte load of the token-contiguous V.  No LDS, no lane movement
//    between the two products, no barrier;
//  * one 256-thread workgroup per (sequence, KV head, tile of kColumns = 128 columns); each of its
//    four waves owns 32 columns (two MFMA column tiles that share every K and V fragment the wave
//    loads) for the whole walk, with its own running maximum m, normaliser l and O per column: no
//    cross-wave merge.  A wave whose columns lie past the chunk exits at once, and so does a workgroup
//    past its sequence's chunk (the grid is sized by max_q_len).  The heavy (late) tiles of every
//    sequence are launched first;
//  * causal skipping per wave: blocks above the wave's largest position are never loaded; blocks
//    wholly at or below its smallest position run mask-free code; the others -- the ones a column's
//    diagonal crosses, and with them the sequence's last block, whose slots past ctx lie above every
//    position -- replace the scores of tokens t > p by -inf with a select (a NaN does not survive).
//    The V elements of slots past ctx are replaced by zero (0 * NaN is NaN).  A block that lies
//    wholly above one column's position but not above the wave's leaves that column unchanged:
//    block 0 has made its m finite, so alpha = 1 and every p = 0;
//  * a block's V (8 loads of 16 bytes per lane) is requested first, then the S^T MFMAs of both column
//    tiles are issued; the K registers are then free and take the next block's K (8 loads) and the
//    block id after it, which arrive behind the softmax and the O^T MFMAs.  A second K register set,
//    as in the decode kernel, spills here.  Table positions past the wave's last block are clamped
//    to it (the last block's K is loaded twice).  All addresses are 64-bit;
//  * scale multiplies the fp32 scores; the online softmax, l (summed from the fp32 probabilities) and
//    O are fp32; only P is rounded to bf16 for the MFMA, and the output once at the end after one
//    IEEE division.  The accumulators are rescaled only in blocks that raise some column's maximum;
//  * 212 VGPRs, no AGPRs, no LDS, nothing spilled, 2 waves per SIMD (profiles/r09_prefill_attn).
//
// No bounds checks here by design: the host wrapper (ops/loadgen.py paged_prefill_attention)
// validates shapes, strides and alignment, and on request ctx_lens, q_start and the block ids.
#include "api.h"
#include "paged_attn.h"

namespace gs {
namespace {

constexpr int kWaves = 4;
constexpr int kColTiles = 2;                              // MFMA column tiles per wave
constexpr int kWaveColumns = 16 * kColTiles;
constexpr int kColumns = kWaves * kWaveColumns;           // query columns per workgroup

__global__ void __launch_bounds__(256, 2) paged_prefill_attn_kernel(
    const __bf16* __restrict__ q, const __bf16* __restrict__ k_cache, const __bf16* __restrict__ v_cache,
    const int* __restrict__ block_table, const int* __restrict__ ctx_lens, const int* __restrict__ q_start,
    __bf16* __restrict__ out, int S, int Hq, int Hkv, size_t ld_q, size_t ld_out, size_t ld_table, float scale) {
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
  const int col = lane & 15, g = lane >> 4;
  const float ninf = -__builtin_inff();
  const int p_base = ctx - q_len;                                          // position of chunk token 0
  const int64_t c_last = (c0 + kWaveColumns - 1 < ncols ? c0 + kWaveColumns - 1 : ncols - 1);
  const int p_min = p_base + (int)(c0 / group), p_max = p_base + (int)(c_last / group);
  const int last = p_max / kBlockTokens;                                   // the wave's last block
  const int nfull = (p_min + 1) / kBlockTokens;                            // blocks [0, nfull) need no mask

  // per column tile: this lane's column, whether the chunk has it, its position, its Q^T fragments
  // (head h of the group, d = 32 kk + 8 g .. + 7; zero columns past the chunk, never stored)
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
      const __bf16* qp = q + (size_t)(row0 + i) * ld_q + (size_t)(kvh * group + h) * kHeadDim + KvBf16::kLaneD * g;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) qf[j][kk] = *reinterpret_cast<const bf16x8*>(qp + KvBf16::q_offset(kk));
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
  constexpr size_t kSlab = (size_t)kBlockTokens * kHeadDim;                // one (block, KV head) of K or V
  // the lane's place in a slab
  const __bf16* klane = k_cache + (size_t)(8 * (col >> 2) + (col & 3)) * kHeadDim + KvBf16::kLaneD * g;
  const __bf16* vlane = v_cache + (size_t)col * kBlockTokens + 8 * g;
  int b = 0;
  size_t slab = ((size_t)trow[0] * Hkv + kvh) * kSlab;
  int next_id = trow[min(1, last)];
  KvBf16::KBlock kf;
  KvBf16::load_k(kf, klane + slab);

  // One loop with wave-uniform branches around the mask code: as two loops, a mask-free one and a
  // masked one, the register state carried from one into the other cost 19 to 34 spilled VGPRs.
  for (; b <= last; ++b) {
    const bool masked = b >= nfull;                  // some token of the block lies above some column's position (or past ctx)
    bf16x8 vf[8];
#pragma unroll
    for (int db = 0; db < 8; ++db)
      vf[db] = *reinterpret_cast<const bf16x8*>(vlane + slab + (size_t)db * 16 * kBlockTokens);
    // S^T = K . Q^T for the wave's column tiles; that done, the K registers take the next block's
    f32x4 sc[kColTiles][2];
#pragma unroll
    for (int j = 0; j < kColTiles; ++j)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        sc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
          sc[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t][kk], qf[j][kk], sc[j][t], 0, 0, 0);
      }
    __builtin_amdgcn_sched_barrier(0);
    slab = ((size_t)next_id * Hkv + kvh) * kSlab;
    KvBf16::load_k(kf, klane + slab);
    next_id = trow[min(b + 2, last)];
    __builtin_amdgcn_sched_barrier(0);
    const int tok0 = b * kBlockTokens + 8 * g;       // this lane's first token
    if (masked && (b + 1) * kBlockTokens > ctx) {    // the sequence's last block, not full
      // a 32-bit word of a V fragment holds tokens tok0 + 2 w and tok0 + 2 w + 1
      u32x4 keep;
#pragma unroll
      for (int w = 0; w < 4; ++w)
        keep[w] = (tok0 + 2 * w < ctx ? 0x0000FFFFu : 0u) | (tok0 + 2 * w + 1 < ctx ? 0xFFFF0000u : 0u);
#pragma unroll
      for (int db = 0; db < 8; ++db) vf[db] = __builtin_bit_cast(bf16x8, __builtin_bit_cast(u32x4, vf[db]) & keep);
    }
#pragma unroll
    for (int j = 0; j < kColTiles; ++j) {
      float sv[8];                                   // tokens tok0 .. tok0 + 7, this lane's column
      const int below = pos[j] - tok0;               // tokens tok0 + i with i > below lie above the column's position
#pragma unroll
      for (int i = 0; i < 8; ++i) sv[i] = sc[j][i >> 2][i & 3] * scale;
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
      bf16x8 pf;
      float ps = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float p = __builtin_amdgcn_exp2f((sv[i] - mn) * kLog2e);
        ps += p;
        pf[i] = (__bf16)p;
      }
      l[j] = l[j] * alpha + ps;                      // this lane's 8 tokens; the 4 lane groups are added at the end
      // O^T = alpha O^T + V^T . P; alpha is exactly 1 in every column whose maximum stood
      if (__any(alpha != 1.f)) {
#pragma unroll
        for (int db = 0; db < 8; ++db) o[j][db] *= alpha;
      }
#pragma unroll
      for (int db = 0; db < 8; ++db) o[j][db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[db], pf, o[j][db], 0, 0, 0);
    }
  }

  // O^T register r of db is d = 16 db + 4 g + r of the lane's column: 8-byte stores
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
        for (int e = 0; e < 4; ++e) r[e] = (__bf16)(o[j][db][e] / lj);
        *reinterpret_cast<bf16x4*>(orow + 16 * db + 4 * g) = r;
      }
    }
  }
}

int64_t column_tiles(int Hq, int Hkv, int max_q_len) {
  return ((int64_t)max_q_len * (Hq / Hkv) + kColumns - 1) / kColumns;
}

}  // namespace

int paged_prefill_workgroups(int S, int Hq, int Hkv, int max_q_len) {
  if (S < 0 || Hq <= 0 || Hkv <= 0 || Hq % Hkv || max_q_len < 0)
    throw std::runtime_error("paged_prefill: negative or zero sizes");
  const int64_t n = (int64_t)S * Hkv * column_tiles(Hq, Hkv, max_q_len);
  if (n >= (int64_t)1 << 31) throw std::runtime_error("paged_prefill: more than 2^31 - 1 workgroups");
  return (int)n;
}

void paged_prefill_bf16(uintptr_t q, uintptr_t k_cache, uintptr_t v_cache, uintptr_t block_table, uintptr_t ctx_lens,
                        uintptr_t q_start, uintptr_t out, int S, int Hq, int Hkv, int max_q_len, int64_t ld_q,
                        int64_t ld_out, int64_t ld_table, float scale, uintptr_t stream) {
  check_paged_operands("paged_prefill", "token", q, k_cache, v_cache, block_table, ctx_lens, out, S, Hq, Hkv, ld_q, ld_out,
                       ld_table);
  if (max_q_len < 0) throw std::runtime_error("paged_prefill: negative max_q_len");
  if (q_start % 4) throw std::runtime_error("paged_prefill: q_start must be 4-byte aligned");
  const int grid = paged_prefill_workgroups(S, Hq, Hkv, max_q_len);
  if (grid == 0) return;
  hipLaunchKernelGGL(paged_prefill_attn_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const __bf16*>(q), reinterpret_cast<const __bf16*>(k_cache),
                     reinterpret_cast<const __bf16*>(v_cache), reinterpret_cast<const int*>(block_table),
                     reinterpret_cast<const int*>(ctx_lens), reinterpret_cast<const int*>(q_start),
                     reinterpret_cast<__bf16*>(out), S, Hq, Hkv, (size_t)ld_q, (size_t)ld_out, (size_t)ld_table, scale);
  HIP_CHECK(hipGetLastError());
}

}  // namespace gs
