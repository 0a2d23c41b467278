// RoPE + paged-KV append (gfx950 / MI355X): the step of a decoder layer between the fused QKV projection
// and the paged attentions (decode_attn.hip, prefill_attn.hip) -- the only writer of their cache.
//
//   row          = q_start[s] + i,  i in [0, q_len[s]),  q_len[s] = q_start[s + 1] - q_start[s]
//   p            = ctx[s] - q_len[s] + i                            the token's position in its sequence
//   c, s         = cos_sin[p, 0:64], cos_sin[p, 64:128]             fp32, supplied by the caller
//   y[e]         = fmaf(x[e], c[e], -(x[e + 64] * s[e]))            e in [0, 64): rotate-half pairing
//   y[e + 64]    = fmaf(x[e + 64], c[e], x[e] * s[e])               fp32, one rounding to bf16
//   q_out[row, h, :]                          = y of qkv[row, h, :]            h in [0, Hq)
//   k_cache[block, g, p % 32, :]              = y of qkv[row, Hq + g, :]       g in [0, Hkv)
//   v_cache[block, g, :, p % 32]              = qkv[row, Hq + Hkv + g, :]      bit for bit
//   block        = block_table[s, p / 32]
//
// qkv is [Tq, Hq + 2 Hkv, 128], the output of the fused QKV GEMM; the caches are the attentions'
// (k_cache [NB, Hkv, 32, 128], v_cache [NB, Hkv, 128, 32]).  Small, latency-dominated and write-scattering:
// no MFMA, no transcendentals, a few hundred bytes per lane.  Shape of the kernel:
//
//  * the grid is S * Hkv * ((max_q_len + 30) / 32 + 1) workgroups of 256 threads (rope_append_workgroups; a
//    chunk of L tokens that starts in slot 31 touches 1 + ceil((L - 1) / 32) blocks).  Workgroup (s, g, j)
//    takes the chunk's tokens of the j-th cache block the chunk touches, for KV head g: K head g, V head g and
//    the q heads of group g.  One workgroup owns the new slots of a (block, KV head) slab, so no two write
//    the same 16 bytes; a workgroup past the chunk's last block exits at once;
//  * V first: the workgroup's n <= 32 tokens x 128 d tile is loaded 16 bytes per lane (16 lanes per 256-byte
//    row) into 8 KiB of LDS, row-major with the 16-byte chunk index XORed by 2 ((row >> 3) & 3) -- the four
//    lanes that later read rows 8 apart at one d then sit on different banks;
//  * then q and K, while the V loads are in flight: 8 lanes per 256-byte row, a lane holding the 16 bytes
//    at d = 8 l and their partners at d = 64 + 8 l, so a pair never leaves its lane; both halves are loaded
//    and stored 16 bytes per lane.  The rows of a token are its group's q heads (contiguous in qkv) and then
//    its K head; they share the token's cos_sin row, 64 bytes per lane of it;
//  * after one barrier the V tile is written token-contiguous: item (d, v) is the 8 slots 8 v .. 8 v + 7 of
//    row d of the slab; four consecutive lanes hold one d, a wave 16 consecutive d (1 KiB contiguous).  An
//    item wholly inside the chunk's slots is one 16-byte store; a ragged item (the chunk's head and tail, and
//    every decode token) stores its slots 2 bytes at a time.  Slots outside the chunk are never written and
//    never read: no read-modify-write, a neighbouring launch may own them;
//  * the arithmetic is written with __fmaf_rn / __fmul_rn: the result does not depend on -ffp-contract.  A
//    NaN or Inf in x1, x2, c or s reaches both outputs of its pair wherever IEEE says so and nothing else;
//  * idempotent: q is not rotated in place, the caches are never read, so a captured launch may be replayed.
//
// No bounds checks here by design: the host wrapper (ops/loadgen.py rope_append) validates shapes, strides
// and alignment, and on request ctx_lens, q_start, the touched block ids and that they are distinct.
// 40 VGPRs, no AGPRs, 8 KiB of LDS, nothing spilled, 8 waves per SIMD.  Measured on an MI355X with HIP events
// around single launches (profiles/r11_rope_append, 32 query heads over 8 KV heads): 23.4 us for 256 decode
// tokens (2,048 workgroups, 6.4 MB), 24.2 us for two 1,024-token chunks (528 workgroups, 51.4 MB: 2.1 TB/s) and
// 22.2 us for sixteen 128-token chunks (2.3 TB/s), beside 6.2 TB/s of the stream triad: latency-dominated.
#include "api.h"
#include "paged_attn.h"

namespace gs {
namespace {

typedef unsigned short u16;
typedef float f32x4a __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kHalf = kHeadDim / 2;                      // the rotate-half distance
constexpr int kRowLanes = 8;                             // lanes per q / K row: 16 bytes of each half
constexpr int kVLanes = kHeadDim / 8;                    // lanes per V row: 16 bytes each

// the V tile in LDS: element (row, d) -- 16-byte chunks swizzled by the row's group of 8
__device__ __forceinline__ int v_lds_index(int row, int d) {
  return row * kHeadDim + ((((d >> 3) ^ (((row >> 3) & 3) << 1))) << 3) + (d & 7);
}

__device__ __forceinline__ void rotate_store(bf16x8 x1, bf16x8 x2, const float (&c)[8], const float (&sn)[8],
                                             __bf16* dst) {
  bf16x8 y1, y2;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float a = (float)x1[e], b = (float)x2[e];
    y1[e] = (__bf16)__fmaf_rn(a, c[e], -__fmul_rn(b, sn[e]));
    y2[e] = (__bf16)__fmaf_rn(b, c[e], __fmul_rn(a, sn[e]));
  }
  *reinterpret_cast<bf16x8*>(dst) = y1;
  *reinterpret_cast<bf16x8*>(dst + kHalf) = y2;
}

__global__ void __launch_bounds__(kThreads) rope_append_kernel(
    const __bf16* __restrict__ qkv, const float* __restrict__ cos_sin, __bf16* __restrict__ k_cache,
    u16* __restrict__ v_cache, const int* __restrict__ block_table, const int* __restrict__ ctx_lens,
    const int* __restrict__ q_start, __bf16* __restrict__ q_out, int Hq, int Hkv, int nj, size_t ld_qkv,
    size_t ld_q_out, size_t ld_table) {
  __shared__ __attribute__((aligned(16))) u16 vt[kBlockTokens * kHeadDim];
  const int tid = threadIdx.x;
  // the grid is [sequence][KV head][j]
  const int j = blockIdx.x % nj;
  const int g = (blockIdx.x / nj) % Hkv, s = blockIdx.x / nj / Hkv;
  const int row0 = q_start[s];
  const int q_len = q_start[s + 1] - row0;
  if (q_len <= 0) return;
  const int ctx = ctx_lens[s];
  const int p0 = ctx - q_len;                            // position of chunk token 0
  const int jb = p0 / kBlockTokens + j;                  // the table column of this workgroup's block
  if (jb > (ctx - 1) / kBlockTokens) return;
  const int p_lo = max(p0, jb * kBlockTokens);           // the workgroup's positions [p_lo, p_hi)
  const int p_hi = min(ctx, (jb + 1) * kBlockTokens);
  const int n = p_hi - p_lo, slot0 = p_lo - jb * kBlockTokens;
  const int group = Hq / Hkv;
  const size_t blk = (size_t)block_table[(size_t)s * ld_table + jb];
  const size_t slab = (blk * Hkv + g) * ((size_t)kBlockTokens * kHeadDim);
  const __bf16* x0 = qkv + (size_t)(row0 + (p_lo - p0)) * ld_qkv;        // the workgroup's first qkv row

  // V: token i of the workgroup to row slot0 + i of the LDS tile
  {
    const int lane = tid % kVLanes;
    for (int i = tid / kVLanes; i < n; i += kThreads / kVLanes) {
      const bf16x8_bits v = *reinterpret_cast<const bf16x8_bits*>(
          x0 + (size_t)i * ld_qkv + (size_t)(Hq + Hkv + g) * kHeadDim + 8 * lane);
      *reinterpret_cast<bf16x8_bits*>(&vt[v_lds_index(slot0 + i, 8 * lane)]) = v;
    }
  }

  // q heads of the group and the K head: row r is token r / (group + 1), head r % (group + 1) (group: K)
  {
    const int lane = tid % kRowLanes;
    const int rows = n * (group + 1);
    for (int r = tid / kRowLanes; r < rows; r += kThreads / kRowLanes) {
      const int i = r / (group + 1), hh = r - i * (group + 1);
      const bool is_k = hh == group;
      const __bf16* src = x0 + (size_t)i * ld_qkv + (size_t)(is_k ? Hq + g : g * group + hh) * kHeadDim + 8 * lane;
      const bf16x8 x1 = *reinterpret_cast<const bf16x8*>(src);
      const bf16x8 x2 = *reinterpret_cast<const bf16x8*>(src + kHalf);
      const float* t = cos_sin + (size_t)(p_lo + i) * kHeadDim + 8 * lane;
      float c[8], sn[8];
#pragma unroll
      for (int w = 0; w < 2; ++w) {
        const f32x4a cv = *reinterpret_cast<const f32x4a*>(t + 4 * w);
        const f32x4a sv = *reinterpret_cast<const f32x4a*>(t + kHalf + 4 * w);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          c[4 * w + e] = cv[e];
          sn[4 * w + e] = sv[e];
        }
      }
      __bf16* dst = is_k ? k_cache + slab + (size_t)(slot0 + i) * kHeadDim + 8 * lane
                         : q_out + (size_t)(row0 + (p_lo - p0) + i) * ld_q_out + (size_t)(g * group + hh) * kHeadDim + 8 * lane;
      rotate_store(x1, x2, c, sn, dst);
    }
  }

  __syncthreads();

  // V out: item (d, v) is slots 8 v .. 8 v + 7 of row d of the slab
  u16* vdst = v_cache + slab;
  for (int it = tid; it < kHeadDim * (kBlockTokens / 8); it += kThreads) {
    const int d = it >> 2, v = it & 3;
    const int lo = max(8 * v, slot0), hi = min(8 * v + 8, slot0 + n);
    if (lo >= hi) continue;
    u16* out = vdst + (size_t)d * kBlockTokens;
    if (hi - lo == 8) {
      bf16x8_bits w;
#pragma unroll
      for (int e = 0; e < 8; ++e) w[e] = (short)vt[v_lds_index(8 * v + e, d)];
      *reinterpret_cast<bf16x8_bits*>(out + 8 * v) = w;
    } else {
      for (int t = lo; t < hi; ++t) out[t] = vt[v_lds_index(t, d)];
    }
  }
}

}  // namespace

int rope_append_workgroups(int S, int Hkv, int max_q_len) {
  if (S < 0 || Hkv <= 0 || max_q_len < 0) throw std::runtime_error("rope_append: negative or zero sizes");
  if (S == 0 || max_q_len == 0) return 0;
  const int64_t n = (int64_t)S * Hkv * (((int64_t)max_q_len + 30) / 32 + 1);
  if (n >= (int64_t)1 << 31) throw std::runtime_error("rope_append: more than 2^31 - 1 workgroups");
  return (int)n;
}

void rope_append_bf16(uintptr_t qkv, uintptr_t cos_sin, uintptr_t k_cache, uintptr_t v_cache, uintptr_t block_table,
                      uintptr_t ctx_lens, uintptr_t q_start, uintptr_t q_out, int S, int Hq, int Hkv, int max_q_len,
                      int max_pos, int64_t ld_qkv, int64_t ld_q_out, int64_t ld_table, uintptr_t stream) {
  check_paged_operands("rope_append", "token", qkv, k_cache, v_cache, block_table, ctx_lens, q_out, S, Hq, Hkv, ld_qkv,
                       ld_q_out, ld_table);
  if (ld_qkv < ((int64_t)Hq + 2 * (int64_t)Hkv) * kHeadDim)
    throw std::runtime_error("rope_append: the qkv token stride must be >= (Hq + 2 Hkv) * 128 elements");
  if (max_q_len < 0 || max_pos < 0) throw std::runtime_error("rope_append: negative max_q_len or max_pos");
  if (q_start % 4) throw std::runtime_error("rope_append: q_start must be 4-byte aligned");
  if (cos_sin % 16) throw std::runtime_error("rope_append: cos_sin must be 16-byte aligned");
  const int grid = rope_append_workgroups(S, Hkv, max_q_len);
  if (grid == 0) return;
  hipLaunchKernelGGL(rope_append_kernel, dim3(grid), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const __bf16*>(qkv), reinterpret_cast<const float*>(cos_sin),
                     reinterpret_cast<__bf16*>(k_cache), reinterpret_cast<u16*>(v_cache),
                     reinterpret_cast<const int*>(block_table), reinterpret_cast<const int*>(ctx_lens),
                     reinterpret_cast<const int*>(q_start), reinterpret_cast<__bf16*>(q_out), Hq, Hkv, grid / (S * Hkv),
                     (size_t)ld_qkv, (size_t)ld_q_out, (size_t)ld_table);
  HIP_CHECK(hipGetLastError());
}

}  // namespace gs
