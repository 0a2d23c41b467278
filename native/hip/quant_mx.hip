// MX quantiser (gfx950 / MI355X): bf16 activations to OCP Microscaling v1.0 blocks -- 32 elements of a row share
// one E8M0 scale byte, the elements are fp8 (e4m3fn, one per byte) or fp4 (e2m1, two per byte, element 2i in bits
// 3:0 of byte i).  The format and the rule are stated in api.h (quantize_mx_bf16); in short, per block:
//
//   e      = the largest biased exponent field (bits >> 7) & 0xFF of the 32 bf16 inputs
//   e==255 : scale byte 255, every element byte 0x00                 (an Inf or NaN in the block)
//   else   : scale byte b = max(e - emax, 0), emax = 8 (fp8) / 2 (fp4); element = v * 2^(127 - b) rounded to the
//            element format to nearest, ties to even, saturated at 448 / 6, the input's sign bit always carried
//
// Everything is integer or power-of-two arithmetic, so the CPU reference (ops/loadgen.py quantize_mx_reference)
// agrees bit for bit.  How an element is rounded, with M = 3 / 1 mantissa bits and smallest normal exponent
// emin = -6 / 0:
//
//   ax = |v| * 2^(127 - b)                    exact in fp32 (where it would be an fp32 subnormal it is far below
//                                             half the format's smallest step and rounds to zero either way)
//   C  = 2^(max(exponent(ax), emin) + 23 - M) the power of two whose fp32 ulp is the format's step at ax
//   r  = (ax + C) - C                         one fp32 add rounds ax to that step, nearest even; the subtraction
//                                             is exact.  r = min(r, 448 / 6)
//   code = r >= 2^emin ? (bits(r) >> (23 - M)) - ((126 + emin) << M) : int(r * 2^(M - emin))
//
// Built without -ffast-math; the add and the subtraction are __fadd_rn / __fsub_rn, which are never re-associated.
// v_cvt_scalef32_pk_fp8_bf16 / _fp4_bf16 are not used: whether they follow this rule on ties, saturation, signed
// zero and subnormal results has not been measured.
//
// Shape of the kernel: the work is flattened over (row, 16-byte chunk of 8 inputs); a block of 32 is four
// consecutive chunks, so FOUR LANES hold a block (D % 32 == 0: a lane group never straddles a row) and its
// exponent maximum is two butterfly steps (no LDS memory).  A workgroup of 256 threads covers 1,024 consecutive
// chunks, thread t taking t, t + 256, t + 512, t + 768: four 16-byte loads in flight before the first use, each
// load instruction of a wave one coalesced 1 KiB access.  A lane stores its 8 fp8 bytes as one 8-byte store, or
// its 8 fp4 nibbles as one 4-byte store, where q's rows allow it (base and row stride multiples of 8 / 4 bytes),
// else byte by byte; lane 0 of a group stores the block's scale byte (single bytes: the scale rows have no
// alignment rule; assembling four neighbours into a dword where the layout allows it is left out).  No atomics,
// no scratch.  The grid is ceil(T * D / 8192) (quantize_mx_workgroups); offsets are 64-bit.
//
// No bounds checks here by design: the host wrapper (ops/loadgen.py quantize_mx) validates shapes, strides,
// alignment and overlap.
// 46 VGPRs, no AGPRs, no LDS, nothing spilled, 8 waves per SIMD.  Measured on an MI355X as chains of launches
// replayed from one graph (profiles/r16_mx): 5.5 / 5.2 us (fp8 / fp4) for 256 x 4096, 26.2 / 24.6 us for 2048 x 14336
// and 50.2 / 47.7 us for 8192 x 8192 (from HBM: 4.05 / 3.56 TB/s, 0.67 / 0.59 of the stream triad's 6.04 TB/s in the
// same run).
#include "api.h"
#include "common.h"

namespace gs {
namespace {

typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int kThreads = 256;
constexpr int kChunks = 4;                               // 16-byte input chunks per thread
constexpr int kSpan = kThreads * kChunks;                // chunks per workgroup: 8192 inputs

// the element code (sign included) of the bf16 pattern h under the block's scale factor sc = 2^(127 - b)
template <bool FP4>
__device__ __forceinline__ uint32_t mx_code(uint32_t h, float sc) {
  constexpr int M = FP4 ? 1 : 3, EMIN = FP4 ? 0 : -6;
  const float ax = __fmul_rn(__uint_as_float((h & 0x7FFFu) << 16), sc);
  const uint32_t ex = __float_as_uint(ax) >> 23;
  const uint32_t ec = max(ex, (uint32_t)(EMIN + 127)) + (23 - M);
  const float C = __uint_as_float(ec << 23);
  float r = __fsub_rn(__fadd_rn(ax, C), C);
  r = fminf(r, FP4 ? 6.f : 448.f);
  const uint32_t normal = (__float_as_uint(r) >> (23 - M)) - ((126 + EMIN) << M);
  const uint32_t subnormal = (uint32_t)(int)__fmul_rn(r, FP4 ? 2.f : 512.f);
  const uint32_t code = r >= (FP4 ? 1.f : 0.015625f) ? normal : subnormal;
  return code | ((h >> 15) << (FP4 ? 3 : 7));
}

template <bool FP4, bool WIDE>
__global__ void __launch_bounds__(kThreads)
quantize_mx_kernel(const uint16_t* __restrict__ x, uint8_t* __restrict__ q, uint8_t* __restrict__ scales, int D,
                   int64_t total, size_t ld_x, size_t ld_q, size_t ld_s) {
  constexpr int EMAX = FP4 ? 2 : 8;
  const int per_row = D >> 3;                            // chunks of a row
  const int64_t first = (int64_t)blockIdx.x * kSpan + threadIdx.x;
  u16x8 v[kChunks];
#pragma unroll
  for (int k = 0; k < kChunks; ++k) {
    const int64_t chunk = first + k * kThreads;
    v[k] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (chunk < total) {
      const int64_t row = chunk / per_row;
      const int col = (int)(chunk - row * per_row);
      v[k] = *reinterpret_cast<const u16x8*>(x + (size_t)row * ld_x + (col << 3));
    }
  }
#pragma unroll
  for (int k = 0; k < kChunks; ++k) {
    const int64_t chunk = first + k * kThreads;
    int e = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) e = max(e, (int)(v[k][i] >> 7) & 0xFF);
    // the block's four lanes (a whole group is in range or out of it: total is a multiple of 4)
    e = max(e, __shfl_xor(e, 1));
    e = max(e, __shfl_xor(e, 2));
    const bool nonfinite = e == 255;
    const int b = nonfinite ? 255 : max(e - EMAX, 0);    // finite: at most 254 - emax
    const float sc = __uint_as_float((uint32_t)(254 - min(b, 253)) << 23);
    uint32_t c[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) c[i] = nonfinite ? 0u : mx_code<FP4>(v[k][i], sc);
    if (chunk < total) {
      const int64_t row = chunk / per_row;
      const int col = (int)(chunk - row * per_row);
      if constexpr (FP4) {
        uint8_t* dst = q + (size_t)row * ld_q + (col << 2);
        uint32_t w = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) w |= c[i] << (4 * i);
        if constexpr (WIDE) {
          *reinterpret_cast<uint32_t*>(dst) = w;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) dst[i] = (uint8_t)(w >> (8 * i));
        }
      } else {
        uint8_t* dst = q + (size_t)row * ld_q + (col << 3);
        if constexpr (WIDE) {
          *reinterpret_cast<u32x2*>(dst) = u32x2{c[0] | c[1] << 8 | c[2] << 16 | c[3] << 24,
                                                 c[4] | c[5] << 8 | c[6] << 16 | c[7] << 24};
        } else {
#pragma unroll
          for (int i = 0; i < 8; ++i) dst[i] = (uint8_t)c[i];
        }
      }
      if ((col & 3) == 0) scales[(size_t)row * ld_s + (col >> 2)] = (uint8_t)b;
    }
  }
}

}  // namespace

int quantize_mx_workgroups(int T, int D) {
  if (T < 0 || D <= 0 || D % 32) throw std::runtime_error("quantize_mx: T must be >= 0 and D a positive multiple of 32");
  const int64_t chunks = (int64_t)T * (D / 8);
  const int64_t n = (chunks + kSpan - 1) / kSpan;
  if (n >= (int64_t)1 << 31) throw std::runtime_error("quantize_mx: more than 2^31 - 1 workgroups");
  return (int)n;
}

void quantize_mx_bf16(uintptr_t x, uintptr_t q, uintptr_t scales, int T, int D, int64_t ld_x, int64_t ld_q,
                      int64_t ld_scales, int fmt, uintptr_t stream) {
  const int grid = quantize_mx_workgroups(T, D);
  if (fmt != kMxFp8 && fmt != kMxFp4) throw std::runtime_error("quantize_mx: fmt must be 0 (fp8) or 4 (fp4)");
  const bool fp4 = fmt == kMxFp4;
  if (!x || !q || !scales) throw std::runtime_error("quantize_mx: x, q and scales are needed");
  if (ld_x < D || ld_x % 8 || x % 16)
    throw std::runtime_error("quantize_mx: x needs 16-byte aligned rows (row stride >= D, a multiple of 8)");
  if (ld_q < (fp4 ? D / 2 : D) || ld_scales < D / 32)
    throw std::runtime_error("quantize_mx: q / scales row strides are shorter than their rows");
  if (grid == 0) return;
  const int width = fp4 ? 4 : 8;                         // bytes a lane stores at once where q's rows allow it
  const bool wide = q % width == 0 && ld_q % width == 0;
  const void* kernel = fp4 ? (wide ? (const void*)quantize_mx_kernel<true, true> : (const void*)quantize_mx_kernel<true, false>)
                           : (wide ? (const void*)quantize_mx_kernel<false, true> : (const void*)quantize_mx_kernel<false, false>);
  const uint16_t* xp = reinterpret_cast<const uint16_t*>(x);
  uint8_t* qp = reinterpret_cast<uint8_t*>(q);
  uint8_t* sp = reinterpret_cast<uint8_t*>(scales);
  int64_t total = (int64_t)T * (D / 8);
  size_t lx = (size_t)ld_x, lq = (size_t)ld_q, ls = (size_t)ld_scales;
  void* args[] = {&xp, &qp, &sp, &D, &total, &lx, &lq, &ls};
  HIP_CHECK(hipLaunchKernel(kernel, dim3(grid), dim3(kThreads), args, 0, reinterpret_cast<hipStream_t>(stream)));
}

}  // namespace gs
