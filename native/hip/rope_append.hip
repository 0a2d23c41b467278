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
// The cache format is a compile-time parameter of the one body (KvBf16 / KvFp8, paged_attn.h): rope_append_kernel
// and rope_append_kv8_kernel are its two instantiations.  Into an FP8 cache (THE FP8 KV FORMAT and its
// quantisation rule: api.h) the grid, the ownership rule, the "caches never read, replayable" contract and q_out
// -- bf16, the same arithmetic -- are the same; only the cache bytes differ, one fp32 scale per KV head:
//
//   K: y  = the fp32 result of the __fmaf_rn / __fmul_rn rotation, NOT first rounded to bf16
//      z  = __fdiv_rn(y, k_scale[g]);   k_cache[block, g, p % 32, d] = kv8_code(z)
//   V: z  = __fdiv_rn(float(v), v_scale[g]);   v_cache[block, g, d, p % 32] = kv8_code(z)
//
// A K row lane holds d = 8 l .. + 7 and d = 64 + 8 l .. + 7 and stores each as 8 bytes; the V tile goes through
// LDS as bf16 (8 KiB, the same swizzle) and is quantised on the way out: an item (d, v) wholly inside the chunk's
// slots is one 8-byte store of slots 8 v .. 8 v + 7 of row d, a ragged item stores its slots one byte at a time.
// Slots outside the chunk are never written and never read.
//
// No bounds checks here by design: the host wrapper (ops/loadgen.py rope_append) validates shapes, strides
// and alignment, and on request ctx_lens, q_start, the touched block ids, that they are distinct and the scales.
// 40 VGPRs (bf16) or 58 (FP8), no AGPRs, 8 KiB of LDS, nothing spilled, 8 waves per SIMD.  Measured (bf16) on an
// MI355X with HIP events around single launches (profiles/r11_rope_append, 32 query heads over 8 KV heads):
// 23.4 us for 256 decode tokens (2,048 workgroups, 6.4 MB), 24.2 us for two 1,024-token chunks (528 workgroups,
// 51.4 MB: 2.1 TB/s) and 22.2 us for sixteen 128-token chunks (2.3 TB/s), beside 6.2 TB/s of the stream triad:
// latency-dominated.
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

// the e4m3fn code of z by THE QUANTISATION RULE (api.h): the rounding idiom of quant_mx.hip's mx_code<false> on
// an fp32 input.  With ax = min(|z|, 512) (everything from 464 on saturates, and the clamp keeps the exponent
// arithmetic below in range for +-Inf), C = 2^(max(exponent(ax), -6) + 20) is the power of two whose fp32 ulp is
// e4m3's step at ax (2^-9 below 2^-6), so r = (ax + C) - C is ax rounded to that step, ties to even, in one fp32
// add; r = min(r, 448); the code is read off r's bits (normal) or r * 512 (subnormal), a NaN gives 0x7F, and z's
// sign bit is always carried.  Integer and power-of-two arithmetic only: with the one IEEE division in front of it,
// ops/loadgen.py quantize_kv8_reference agrees bit for bit.  v_cvt_pk_fp8_f32 is not used: its ties, saturation,
// NaN and subnormal behaviour against this rule have not been measured.
__device__ __forceinline__ uint32_t kv8_code(float z) {
  const uint32_t bits = __float_as_uint(z);
  const uint32_t mag = bits & 0x7FFFFFFFu;
  const float ax = fminf(__uint_as_float(mag), 512.f);   // a NaN becomes 512 here and is replaced below
  const uint32_t ex = __float_as_uint(ax) >> 23;
  const uint32_t ec = max(ex, 121u) + 20u;
  const float C = __uint_as_float(ec << 23);
  float r = __fsub_rn(__fadd_rn(ax, C), C);
  r = fminf(r, 448.f);
  const uint32_t normal = (__float_as_uint(r) >> 20) - (120u << 3);
  const uint32_t subnormal = (uint32_t)(int)__fmul_rn(r, 512.f);
  uint32_t code = r >= 0.015625f ? normal : subnormal;
  code = mag > 0x7F800000u ? 0x7Fu : code;
  return code | ((bits >> 31) << 7);
}

__device__ __forceinline__ u32x2 pack8(const uint32_t (&c)[8]) {
  return u32x2{c[0] | c[1] << 8 | c[2] << 16 | c[3] << 24, c[4] | c[5] << 8 | c[6] << 16 | c[7] << 24};
}

// The two halves of a rotated row (8 elements each), rounded to bf16: a q_out row, or the K row of a bf16 cache
__device__ __forceinline__ void store_rounded(__bf16* dst, const float (&y1)[8], const float (&y2)[8]) {
  bf16x8 r1, r2;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    r1[e] = (__bf16)y1[e];
    r2[e] = (__bf16)y2[e];
  }
  *reinterpret_cast<bf16x8*>(dst) = r1;
  *reinterpret_cast<bf16x8*>(dst + kHalf) = r2;
}

// The same halves as the K row of an FP8 cache: quantised from the fp32 values, NOT first rounded to bf16, each
// half's 8 codes one 8-byte store
__device__ __forceinline__ void store_quantised(uint8_t* dst, const float (&y1)[8], const float (&y2)[8], float scale) {
  uint32_t c1[8], c2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    c1[e] = kv8_code(__fdiv_rn(y1[e], scale));
    c2[e] = kv8_code(__fdiv_rn(y2[e], scale));
  }
  *reinterpret_cast<u32x2*>(dst) = pack8(c1);
  *reinterpret_cast<u32x2*>(dst + kHalf) = pack8(c2);
}

__device__ __forceinline__ float bf16_bits_to_float(u16 w) { return __uint_as_float((uint32_t)w << 16); }

// V values (bf16 bit patterns from the LDS tile) into the cache, 8 slots or one: overloads on the cache's element
// type.  bf16: bit for bit, 16 bytes or 2; FP8: kv8_code(__fdiv_rn(v, scale)), 8 bytes or 1.  `scale` is the FP8
// cache's v_scale[g] and is not looked at for bf16
__device__ __forceinline__ void store_v8(u16* dst, const u16 (&w)[8], float) {
  bf16x8_bits r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = (short)w[e];
  *reinterpret_cast<bf16x8_bits*>(dst) = r;
}

__device__ __forceinline__ void store_v8(uint8_t* dst, const u16 (&w)[8], float scale) {
  uint32_t c[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) c[e] = kv8_code(__fdiv_rn(bf16_bits_to_float(w[e]), scale));
  *reinterpret_cast<u32x2*>(dst) = pack8(c);
}

__device__ __forceinline__ void store_v1(u16* dst, u16 w, float) { *dst = w; }

__device__ __forceinline__ void store_v1(uint8_t* dst, u16 w, float scale) {
  *dst = (uint8_t)kv8_code(__fdiv_rn(bf16_bits_to_float(w), scale));
}

// The kernel's body for either format.  VElem is what the entry point's parameter list calls a V element: u16, the
// bit pattern of a bf16 (V is copied bit for bit), or uint8_t; k_scale / v_scale are read only where Fmt::kScales
template <class Fmt, class VElem>
__device__ __forceinline__ void rope_append_body(
    u16 (&vt)[kBlockTokens * kHeadDim], const __bf16* __restrict__ qkv, const float* __restrict__ cos_sin,
    typename Fmt::Elem* __restrict__ k_cache, VElem* __restrict__ v_cache, const float* __restrict__ k_scale,
    const float* __restrict__ v_scale, const int* __restrict__ block_table, const int* __restrict__ ctx_lens,
    const int* __restrict__ q_start, __bf16* __restrict__ q_out, int Hq, int Hkv, int nj, size_t ld_qkv,
    size_t ld_q_out, size_t ld_table) {
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
  const size_t slab = (blk * Hkv + g) * ((size_t)kBlockTokens * kHeadDim);      // elements
  const __bf16* x0 = qkv + (size_t)(row0 + (p_lo - p0)) * ld_qkv;        // the workgroup's first qkv row
  float ks = 0.f, vs = 0.f;
  if constexpr (Fmt::kScales) {
    ks = k_scale[g];
    vs = v_scale[g];
  }

  // V: token i of the workgroup to row slot0 + i of the LDS tile, bf16 in both formats
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
      // where the row goes: the K row to its slot of the cache, a q row to q_out.  One select, in front of the
      // rotation: behind it, or as two store paths, the bf16 kernel takes 42 to 54 VGPRs instead of 40
      char* dst = is_k ? reinterpret_cast<char*>(k_cache + slab + (size_t)(slot0 + i) * kHeadDim + 8 * lane)
                       : reinterpret_cast<char*>(q_out + (size_t)(row0 + (p_lo - p0) + i) * ld_q_out +
                                                 (size_t)(g * group + hh) * kHeadDim + 8 * lane);
      // the rotation, in fp32
      float y1[8], y2[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float a = (float)x1[e], b = (float)x2[e];
        y1[e] = __fmaf_rn(a, c[e], -__fmul_rn(b, sn[e]));
        y2[e] = __fmaf_rn(b, c[e], __fmul_rn(a, sn[e]));
      }
      // the K row of an FP8 cache is quantised; every q row, and the K row of a bf16 cache, is rounded once
      if (Fmt::kScales && is_k) store_quantised(reinterpret_cast<uint8_t*>(dst), y1, y2, ks);
      else store_rounded(reinterpret_cast<__bf16*>(dst), y1, y2);
    }
  }

  __syncthreads();

  // V out: item (d, v) is slots 8 v .. 8 v + 7 of row d of the slab
  VElem* vdst = v_cache + slab;
  for (int it = tid; it < kHeadDim * (kBlockTokens / 8); it += kThreads) {
    const int d = it >> 2, v = it & 3;
    const int lo = max(8 * v, slot0), hi = min(8 * v + 8, slot0 + n);
    if (lo >= hi) continue;
    VElem* out = vdst + (size_t)d * kBlockTokens;
    if (hi - lo == 8) {
      u16 w[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) w[e] = vt[v_lds_index(8 * v + e, d)];
      store_v8(out + 8 * v, w, vs);
    } else {
      for (int t = lo; t < hi; ++t) store_v1(out + t, vt[v_lds_index(t, d)], vs);
    }
  }
}

// The two entry points: kernel names and parameter lists are a contract (recorded traces are keyed by them)
__global__ void __launch_bounds__(kThreads) rope_append_kernel(
    const __bf16* __restrict__ qkv, const float* __restrict__ cos_sin, __bf16* __restrict__ k_cache,
    u16* __restrict__ v_cache, const int* __restrict__ block_table, const int* __restrict__ ctx_lens,
    const int* __restrict__ q_start, __bf16* __restrict__ q_out, int Hq, int Hkv, int nj, size_t ld_qkv,
    size_t ld_q_out, size_t ld_table) {
  __shared__ __attribute__((aligned(16))) u16 vt[kBlockTokens * kHeadDim];
  rope_append_body<KvBf16>(vt, qkv, cos_sin, k_cache, v_cache, nullptr, nullptr, block_table, ctx_lens, q_start, q_out,
                           Hq, Hkv, nj, ld_qkv, ld_q_out, ld_table);
}

__global__ void __launch_bounds__(kThreads) rope_append_kv8_kernel(
    const __bf16* __restrict__ qkv, const float* __restrict__ cos_sin, uint8_t* __restrict__ k_cache,
    uint8_t* __restrict__ v_cache, const float* __restrict__ k_scale, const float* __restrict__ v_scale,
    const int* __restrict__ block_table, const int* __restrict__ ctx_lens, const int* __restrict__ q_start,
    __bf16* __restrict__ q_out, int Hq, int Hkv, int nj, size_t ld_qkv, size_t ld_q_out, size_t ld_table) {
  __shared__ __attribute__((aligned(16))) u16 vt[kBlockTokens * kHeadDim];
  rope_append_body<KvFp8>(vt, qkv, cos_sin, k_cache, v_cache, k_scale, v_scale, block_table, ctx_lens, q_start, q_out,
                          Hq, Hkv, nj, ld_qkv, ld_q_out, ld_table);
}

// The launch function of a format: k_scale / v_scale are 0 for KvBf16
template <class Fmt>
void launch_rope_append(const std::string& name, uintptr_t qkv, uintptr_t cos_sin, uintptr_t k_cache, uintptr_t v_cache,
                        uintptr_t k_scale, uintptr_t v_scale, uintptr_t block_table, uintptr_t ctx_lens,
                        uintptr_t q_start, uintptr_t q_out, int S, int Hq, int Hkv, int max_q_len, int max_pos,
                        int64_t ld_qkv, int64_t ld_q_out, int64_t ld_table, uintptr_t stream) {
  check_paged_operands(name, "token", qkv, k_cache, v_cache, block_table, ctx_lens, q_out, S, Hq, Hkv, ld_qkv, ld_q_out,
                       ld_table);
  if (ld_qkv < ((int64_t)Hq + 2 * (int64_t)Hkv) * kHeadDim)
    throw std::runtime_error(name + ": the qkv token stride must be >= (Hq + 2 Hkv) * 128 elements");
  if (max_q_len < 0 || max_pos < 0) throw std::runtime_error(name + ": negative max_q_len or max_pos");
  if (q_start % 4) throw std::runtime_error(name + ": q_start must be 4-byte aligned");
  if (cos_sin % 16) throw std::runtime_error(name + ": cos_sin must be 16-byte aligned");
  if constexpr (Fmt::kScales) check_scales(name, k_scale, v_scale);
  const int grid = rope_append_workgroups(S, Hkv, max_q_len);
  if (grid == 0) return;
  const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if constexpr (Fmt::kScales)
    hipLaunchKernelGGL(rope_append_kv8_kernel, dim3(grid), dim3(kThreads), 0, st, reinterpret_cast<const __bf16*>(qkv),
                       reinterpret_cast<const float*>(cos_sin), reinterpret_cast<uint8_t*>(k_cache),
                       reinterpret_cast<uint8_t*>(v_cache), reinterpret_cast<const float*>(k_scale),
                       reinterpret_cast<const float*>(v_scale), reinterpret_cast<const int*>(block_table),
                       reinterpret_cast<const int*>(ctx_lens), reinterpret_cast<const int*>(q_start),
                       reinterpret_cast<__bf16*>(q_out), Hq, Hkv, grid / (S * Hkv), (size_t)ld_qkv, (size_t)ld_q_out,
                       (size_t)ld_table);
  else
    hipLaunchKernelGGL(rope_append_kernel, dim3(grid), dim3(kThreads), 0, st, reinterpret_cast<const __bf16*>(qkv),
                       reinterpret_cast<const float*>(cos_sin), reinterpret_cast<__bf16*>(k_cache),
                       reinterpret_cast<u16*>(v_cache), reinterpret_cast<const int*>(block_table),
                       reinterpret_cast<const int*>(ctx_lens), reinterpret_cast<const int*>(q_start),
                       reinterpret_cast<__bf16*>(q_out), Hq, Hkv, grid / (S * Hkv), (size_t)ld_qkv, (size_t)ld_q_out,
                       (size_t)ld_table);
  HIP_CHECK(hipGetLastError());
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
  launch_rope_append<KvBf16>("rope_append", qkv, cos_sin, k_cache, v_cache, 0, 0, block_table, ctx_lens, q_start, q_out,
                             S, Hq, Hkv, max_q_len, max_pos, ld_qkv, ld_q_out, ld_table, stream);
}

void rope_append_kv8(uintptr_t qkv, uintptr_t cos_sin, uintptr_t k_cache, uintptr_t v_cache, uintptr_t k_scale,
                     uintptr_t v_scale, uintptr_t block_table, uintptr_t ctx_lens, uintptr_t q_start, uintptr_t q_out,
                     int S, int Hq, int Hkv, int max_q_len, int max_pos, int64_t ld_qkv, int64_t ld_q_out,
                     int64_t ld_table, uintptr_t stream) {
  launch_rope_append<KvFp8>("rope_append_kv8", qkv, cos_sin, k_cache, v_cache, k_scale, v_scale, block_table, ctx_lens,
                            q_start, q_out, S, Hq, Hkv, max_q_len, max_pos, ld_qkv, ld_q_out, ld_table, stream);
}

}  // namespace gs
