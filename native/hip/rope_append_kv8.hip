// RoPE + paged-KV append into an FP8 cache (gfx950 / MI355X): rope_append.hip's kernel with the cache bytes
// quantised to OCP e4m3fn under one fp32 scale per KV head (THE FP8 KV FORMAT and its quantisation rule: api.h).
// The grid, the ownership rule (workgroup (s, g, j) owns the chunk's new slots of one (block, KV head) slab), the
// "caches never read, replayable" contract and q_out -- bf16, the same arithmetic -- are rope_append_kernel's; read
// its header.  The differences are the cache bytes:
//
//   K: y  = the fp32 result of the __fmaf_rn / __fmul_rn rotation, NOT first rounded to bf16
//      z  = __fdiv_rn(y, k_scale[g]);   k_cache[block, g, p % 32, d] = kv8_code(z)
//   V: z  = __fdiv_rn(float(v), v_scale[g]);   v_cache[block, g, d, p % 32] = kv8_code(z)
//
// kv8_code is the rounding idiom of quant_mx.hip's mx_code<false> on an fp32 input: with ax = min(|z|, 512)
// (everything from 464 on saturates, and the clamp keeps the exponent arithmetic below in range for +-Inf),
// C = 2^(max(exponent(ax), -6) + 20) is the power of two whose fp32 ulp is e4m3's step at ax (2^-9 below 2^-6), so
// r = (ax + C) - C is ax rounded to that step, ties to even, in one fp32 add; r = min(r, 448); the code is read off
// r's bits (normal) or r * 512 (subnormal), a NaN gives 0x7F, and z's sign bit is always carried.  Integer and
// power-of-two arithmetic and one IEEE division: ops/loadgen.py quantize_kv8_reference agrees bit for bit.
// v_cvt_pk_fp8_f32 is not used: its ties, saturation, NaN and subnormal behaviour against this rule have not been
// measured.
//
// Stores: a K row lane holds d = 8 l .. + 7 and d = 64 + 8 l .. + 7 and stores each as 8 bytes; the V tile goes
// through LDS as bf16 exactly as in rope_append.hip (8 KiB, the same swizzle) and is quantised on the way out: an
// item (d, v) wholly inside the chunk's slots is one 8-byte store of slots 8 v .. 8 v + 7 of row d, a ragged item
// stores its slots one byte at a time.  Slots outside the chunk are never written and never read.
//
// No bounds checks here by design: the host wrapper (ops/loadgen.py rope_append) validates shapes, strides and
// alignment, and on request ctx_lens, q_start, the touched block ids and the scales.
#include "api.h"
#include "paged_attn.h"

namespace gs {
namespace {

typedef unsigned short u16;
typedef float f32x4a __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int kThreads = 256;
constexpr int kHalf = kHeadDim / 2;                      // the rotate-half distance
constexpr int kRowLanes = 8;                             // lanes per q / K row: 16 bytes of each half
constexpr int kVLanes = kHeadDim / 8;                    // lanes per V row: 16 bytes each

// the V tile in LDS: element (row, d) -- 16-byte chunks swizzled by the row's group of 8
__device__ __forceinline__ int v_lds_index(int row, int d) {
  return row * kHeadDim + ((((d >> 3) ^ (((row >> 3) & 3) << 1))) << 3) + (d & 7);
}

// the e4m3fn code of z by THE QUANTISATION RULE (api.h)
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

__global__ void __launch_bounds__(kThreads) rope_append_kv8_kernel(
    const __bf16* __restrict__ qkv, const float* __restrict__ cos_sin, uint8_t* __restrict__ k_cache,
    uint8_t* __restrict__ v_cache, const float* __restrict__ k_scale, const float* __restrict__ v_scale,
    const int* __restrict__ block_table, const int* __restrict__ ctx_lens, const int* __restrict__ q_start,
    __bf16* __restrict__ q_out, int Hq, int Hkv, int nj, size_t ld_qkv, size_t ld_q_out, size_t ld_table) {
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
  const size_t slab = (blk * Hkv + g) * ((size_t)kBlockTokens * kHeadDim);      // bytes, and elements
  const __bf16* x0 = qkv + (size_t)(row0 + (p_lo - p0)) * ld_qkv;        // the workgroup's first qkv row
  const float ks = k_scale[g], vs = v_scale[g];

  // V: token i of the workgroup to row slot0 + i of the LDS tile, still bf16
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
      float y1[8], y2[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float a = (float)x1[e], b = (float)x2[e];
        y1[e] = __fmaf_rn(a, c[e], -__fmul_rn(b, sn[e]));
        y2[e] = __fmaf_rn(b, c[e], __fmul_rn(a, sn[e]));
      }
      if (is_k) {
        uint32_t c1[8], c2[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          c1[e] = kv8_code(__fdiv_rn(y1[e], ks));
          c2[e] = kv8_code(__fdiv_rn(y2[e], ks));
        }
        uint8_t* dst = k_cache + slab + (size_t)(slot0 + i) * kHeadDim + 8 * lane;
        *reinterpret_cast<u32x2*>(dst) = pack8(c1);
        *reinterpret_cast<u32x2*>(dst + kHalf) = pack8(c2);
      } else {
        bf16x8 o1, o2;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          o1[e] = (__bf16)y1[e];
          o2[e] = (__bf16)y2[e];
        }
        __bf16* dst = q_out + (size_t)(row0 + (p_lo - p0) + i) * ld_q_out + (size_t)(g * group + hh) * kHeadDim + 8 * lane;
        *reinterpret_cast<bf16x8*>(dst) = o1;
        *reinterpret_cast<bf16x8*>(dst + kHalf) = o2;
      }
    }
  }

  __syncthreads();

  // V out: item (d, v) is slots 8 v .. 8 v + 7 of row d of the slab
  uint8_t* vdst = v_cache + slab;
  for (int it = tid; it < kHeadDim * (kBlockTokens / 8); it += kThreads) {
    const int d = it >> 2, v = it & 3;
    const int lo = max(8 * v, slot0), hi = min(8 * v + 8, slot0 + n);
    if (lo >= hi) continue;
    uint8_t* out = vdst + (size_t)d * kBlockTokens;
    if (hi - lo == 8) {
      uint32_t w[8];
#pragma unroll
      for (int e = 0; e < 8; ++e)
        w[e] = kv8_code(__fdiv_rn(__uint_as_float((uint32_t)vt[v_lds_index(8 * v + e, d)] << 16), vs));
      *reinterpret_cast<u32x2*>(out + 8 * v) = pack8(w);
    } else {
      for (int t = lo; t < hi; ++t)
        out[t] = (uint8_t)kv8_code(__fdiv_rn(__uint_as_float((uint32_t)vt[v_lds_index(t, d)] << 16), vs));
    }
  }
}

}  // namespace

void rope_append_kv8(uintptr_t qkv, uintptr_t cos_sin, uintptr_t k_cache, uintptr_t v_cache, uintptr_t k_scale,
                     uintptr_t v_scale, uintptr_t block_table, uintptr_t ctx_lens, uintptr_t q_start, uintptr_t q_out,
                     int S, int Hq, int Hkv, int max_q_len, int max_pos, int64_t ld_qkv, int64_t ld_q_out,
                     int64_t ld_table, uintptr_t stream) {
  check_paged_operands("rope_append_kv8", "token", qkv, k_cache, v_cache, block_table, ctx_lens, q_out, S, Hq, Hkv,
                       ld_qkv, ld_q_out, ld_table);
  if (ld_qkv < ((int64_t)Hq + 2 * (int64_t)Hkv) * kHeadDim)
    throw std::runtime_error("rope_append_kv8: the qkv token stride must be >= (Hq + 2 Hkv) * 128 elements");
  if (max_q_len < 0 || max_pos < 0) throw std::runtime_error("rope_append_kv8: negative max_q_len or max_pos");
  if (q_start % 4) throw std::runtime_error("rope_append_kv8: q_start must be 4-byte aligned");
  if (cos_sin % 16) throw std::runtime_error("rope_append_kv8: cos_sin must be 16-byte aligned");
  if (!k_scale || !v_scale) throw std::runtime_error("rope_append_kv8: k_scale and v_scale are needed");
  if (k_scale % 4 || v_scale % 4) throw std::runtime_error("rope_append_kv8: k_scale / v_scale must be 4-byte aligned");
  const int grid = rope_append_workgroups(S, Hkv, max_q_len);
  if (grid == 0) return;
  hipLaunchKernelGGL(rope_append_kv8_kernel, dim3(grid), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const __bf16*>(qkv), reinterpret_cast<const float*>(cos_sin),
                     reinterpret_cast<uint8_t*>(k_cache), reinterpret_cast<uint8_t*>(v_cache),
                     reinterpret_cast<const float*>(k_scale), reinterpret_cast<const float*>(v_scale),
                     reinterpret_cast<const int*>(block_table), reinterpret_cast<const int*>(ctx_lens),
                     reinterpret_cast<const int*>(q_start), reinterpret_cast<__bf16*>(q_out), Hq, Hkv, grid / (S * Hkv),
                     (size_t)ld_qkv, (size_t)ld_q_out, (size_t)ld_table);
  HIP_CHECK(hipGetLastError());
}

}  // namespace gs
