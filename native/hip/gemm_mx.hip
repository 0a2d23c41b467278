// MX GEMM (gfx950 / MI355X): C[M,N] = act(A[M,K] . W[N,K]^T (+bias)) with both operands in OCP Microscaling blocks
// (api.h, quantize_mx_bf16: 32 elements of a row share one E8M0 scale byte), fp32 accumulate, bf16 out, on
// v_mfma_scale_f32_16x16x128_f8f6f4 with REAL block scales.  W is always fp4 (e2m1, two per byte); A is fp8
// (e4m3fn) or fp4 -- the instruction's format codes 0 and 4, which are also the `a_fmt` values of the entry point.
//
// The kernel is gemm_fp8_nt_kernel's (gemm_tiles.h): glds staging through stage_tile into two LDS stages, the
// 128 x 128 and 64 x 64 block tiles of four waves under the same fill rule (fp8_tile_128), the W fragment as the
// MFMA's first operand so that the epilogue is the D = C^T one (packed bf16x4 stores, fused bias + ReLU).  What
// differs:
//
//  * a K tile is 128 elements for either format: 128 bytes of an fp8 row (staged as the bf16 kernels' 64-deep
//    tile, as gemm_fp8 does) and 64 bytes of an fp4 row (staged as their 32-deep tile, 4 chunks of 16 bytes per
//    row, the same conflict-free XOR swizzle).  A 256-deep fp4 tile (one barrier per two MFMA k-steps) was not
//    built;
//  * the fragment map, MEASURED with one-hot operands and per-block scales (tests/test_gpu_gemm_mx_exact.py, the
//    scale map): the instruction's k axis is cut into four blocks of 32, and the scale of block b of a row comes
//    from the scale register of lane group b (lane = row + 16 b) -- whichever lane holds the block's data.  An fp4
//    operand keeps block fk whole in lane group fk = lane >> 4: k = 32 fk + j for element j, the low nibble of a
//    byte first (the upper four registers are not read for format 4).  An fp8 operand does NOT: registers 0-3 of
//    lane group fk hold k = 16 fk .. 16 fk + 15 and registers 4-7 hold k = 64 + 16 fk .. 64 + 16 fk + 15, so a block
//    is spread over the same register half of two lane groups.  gemm_fp8's map (chunks 2 fk, 2 fk + 1: 32
//    contiguous k per lane) is only right when both operands use it and every scale is equal; against an fp4
//    operand, or with real scales, the fp8 fragment has to be the 16-byte chunks fk and 4 + fk of the row's K tile
//    (lds_frag_fp8_mx).  The lane's scale byte is that of block fk for either format;
//  * the scales reach the lanes as per-lane byte loads straight from global memory: lane (row, fk) loads byte
//    [row, 4 t + fk] of its operand's scale matrix for K tile t, MI + NJ bytes per lane and tile (OPSEL 0: the
//    byte sits in bits 7:0 of the scale register).  The loads of tile t + 1 are issued BEFORE that tile's glds and
//    first used after the barrier that retires the glds, so they add no wait of their own.  Single bytes keep the
//    scale rows free of any alignment rule.
//
// Scale byte 255 (NaN) and byte 0 with non-zero elements are outside the contract (tests print what the hardware
// does); a block of zero elements with scale byte 0 contributes exactly 0.
// No bounds checks here by design: the host wrapper (ops/loadgen.py gemm_mx) validates.
// 128 x 128: 132 VGPRs and 32 KiB of LDS with fp4 activations, 162 and 48 KiB with fp8; 64 x 64: 52 / 70 VGPRs, 16 /
// 24 KiB; no AGPRs, nothing spilled, 3 (128 x 128) and 8 / 6 waves per SIMD.  Measured on an MI355X as chains of
// launches replayed from one graph, random operands (profiles/r16_mx): correct and UNTUNED -- at 8192^3 1,069 us
// (1,029 TF) with fp4 and 1,126 us (976 TF) with fp8 activations against gemm_fp8's 490 us (2,246 TF) and the bf16
// gemm's 728 us (1,510 TF) in the same run.  fp4 activations are only 1.05 to 1.13 times faster than fp8 ones, so
// the MFMA does not bound it; the scale bytes' scattered per-lane loads and the 128-deep tile are the suspects
// (scales through LDS or a dword per row and K tile, and a 256-deep fp4 tile, were not measured).
#include "api.h"
#include "gemm_tiles.h"

namespace gs {
namespace {

// one 16-byte chunk of an fp4 row as the 8-register operand (registers 4 .. 7 are not read for format 4)
__device__ __forceinline__ i32x8 lds_frag_fp4(const char* lds_tile, int row, int fk) {
  const i32x4 lo = __builtin_bit_cast(i32x4, lds_frag<32>(lds_tile, row, fk));
  return i32x8{lo[0], lo[1], lo[2], lo[3], 0, 0, 0, 0};
}

// the fp8 fragment of lane group fk in the instruction's own k order: chunks fk (k = 16 fk ..) and 4 + fk (k = 64 + 16 fk ..)
__device__ __forceinline__ i32x8 lds_frag_fp8_mx(const char* lds_tile, int row, int fk) {
  const i32x4 lo = __builtin_bit_cast(i32x4, lds_frag<BK>(lds_tile, row, fk));
  const i32x4 hi = __builtin_bit_cast(i32x4, lds_frag<BK>(lds_tile, row, 4 + fk));
  return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

template <int BM, int BN, int WGM, int WGN, int OCC, bool A4, bool RELU, bool BIAS>
__global__ void __launch_bounds__(WGM * WGN * 64, OCC)
gemm_mx_nt_kernel(const uint8_t* __restrict__ Aq, const uint8_t* __restrict__ As, const uint8_t* __restrict__ Wq,
                  const uint8_t* __restrict__ Ws, __bf16* __restrict__ C, const float* __restrict__ bias, int M, int N,
                  int K, int lda, int ldas, int ldw, int ldws, int ldc) {
  constexpr int NT = WGM * WGN * 64;
  constexpr int KTE = 128;                             // elements per K tile = one MFMA k-step
  constexpr int AKT = A4 ? 32 : 64, WKT = 32;          // the same tile in bf16-view elements (bytes / 2) per row
  constexpr int A_BYTES = BM * AKT * 2, B_BYTES = BN * WKT * 2;
  constexpr int WTM = BM / WGM, WTN = BN / WGN;
  constexpr int MI = WTM / 16, NJ = WTN / 16;
  constexpr int A_FMT = A4 ? kMxFp4 : kMxFp8;
  static_assert(A_BYTES / 16 % NT == 0 && B_BYTES / 16 % NT == 0, "stage split");
  __shared__ __attribute__((aligned(16))) char smem[2 * (A_BYTES + B_BYTES)];
  // bf16 views of the byte rows for the 16-byte glds staging (row strides halved)
  const __bf16* A = reinterpret_cast<const __bf16*>(Aq);
  const __bf16* Wt = reinterpret_cast<const __bf16*>(Wq);
  const int lda2 = lda / 2, ldw2 = ldw / 2;

  int tm, tn;
  tile_coords(blockIdx.x, gridDim.x, M / BM, N / BN, 0, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int lane = threadIdx.x & (kWave - 1);
  const int wm = wave / WGN, wn = wave % WGN;
  f32x4 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto tileA = [&](int buf) { return smem + buf * (A_BYTES + B_BYTES); };
  auto tileB = [&](int buf) { return smem + buf * (A_BYTES + B_BYTES) + A_BYTES; };
  const int frow = lane & 15;
  const int fk = lane >> 4;
  auto stage = [&](int t, int buf) {
    stage_tile<BM, NT, AKT>(A, lda2, m0, t * AKT, tileA(buf), wave, lane);
    stage_tile<BN, NT, WKT>(Wt, ldw2, n0, t * WKT, tileB(buf), wave, lane);
  };
  // this lane's scale bytes of K tile t: block 4 t + fk of its MI rows of A and its NJ rows of W
  const uint8_t* as_lane = As + (size_t)(m0 + wm * WTM + frow) * ldas + fk;
  const uint8_t* ws_lane = Ws + (size_t)(n0 + wn * WTN + frow) * ldws + fk;
  int sa[MI], sw[NJ], na[MI], nw[NJ];
  auto load_scales = [&](int t, int (&a)[MI], int (&w)[NJ]) {
#pragma unroll
    for (int i = 0; i < MI; ++i) a[i] = as_lane[(size_t)i * 16 * ldas + t * 4];
#pragma unroll
    for (int j = 0; j < NJ; ++j) w[j] = ws_lane[(size_t)j * 16 * ldws + t * 4];
  };
  auto compute = [&](const char* a_t, const char* b_t) {
    i32x8 af[MI], bf[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) bf[j] = lds_frag_fp4(b_t, wn * WTN + j * 16 + frow, fk);
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      if constexpr (A4) af[i] = lds_frag_fp4(a_t, wm * WTM + i * 16 + frow, fk);
      else af[i] = lds_frag_fp8_mx(a_t, wm * WTM + i * 16 + frow, fk);
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bf[j], af[i], acc[i][j], kMxFp4, A_FMT, 0, sw[j],
                                                                      0, sa[i]);
    __builtin_amdgcn_s_setprio(0);
  };
  const int nt = K / KTE;
  load_scales(0, sa, sw);
  stage(0, 0);
  __syncthreads();
  int buf = 0;
  for (int t = 0; t < nt; ++t) {
#pragma unroll
    for (int i = 0; i < MI; ++i) na[i] = 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) nw[j] = 0;
    if (t + 1 < nt) {
      load_scales(t + 1, na, nw);
      stage(t + 1, buf ^ 1);
    }
    compute(tileA(buf), tileB(buf));
    __syncthreads();
    buf ^= 1;
#pragma unroll
    for (int i = 0; i < MI; ++i) sa[i] = na[i];
#pragma unroll
    for (int j = 0; j < NJ; ++j) sw[j] = nw[j];
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int col = n0 + wn * WTN + j * 16 + fk * 4;
    f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
    if (BIAS) bv = *reinterpret_cast<const f32x4*>(bias + col);
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int row = m0 + wm * WTM + i * 16 + frow;
      f32x4 v = acc[i][j] + bv;
      bf16x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = act_bf16<RELU>(v[r]);
      *reinterpret_cast<bf16x4*>(C + (size_t)row * ldc + col) = o;
    }
  }
}

struct MxArgs {
  const uint8_t *A, *As, *W, *Ws;
  __bf16* C;
  const float* bias;
  int M, N, K, lda, ldas, ldw, ldws, ldc;
  bool relu;
  hipStream_t s;
};

template <int BM, int BN, bool A4, bool RELU, bool BIAS>
void launch_one(const MxArgs& g) {
  const dim3 grid((g.M / BM) * (g.N / BN)), block(256);
  hipLaunchKernelGGL((gemm_mx_nt_kernel<BM, BN, 2, 2, 2, A4, RELU, BIAS>), grid, block, 0, g.s, g.A, g.As, g.W, g.Ws, g.C,
                     g.bias, g.M, g.N, g.K, g.lda, g.ldas, g.ldw, g.ldws, g.ldc);
}

template <int BM, int BN, bool A4>
void launch_act(const MxArgs& g) {
  if (g.relu && g.bias) launch_one<BM, BN, A4, true, true>(g);
  else if (g.relu) launch_one<BM, BN, A4, true, false>(g);
  else if (g.bias) launch_one<BM, BN, A4, false, true>(g);
  else launch_one<BM, BN, A4, false, false>(g);
}

void check_mx_shape(int M, int N, int K, const char* who) {
  if (M <= 0 || N <= 0 || K <= 0 || M % 64 || N % 64 || K % 128)
    throw std::runtime_error(std::string(who) + ": M, N must be positive multiples of 64 and K of 128");
}

}  // namespace

int gemm_mx_workgroups(int M, int N, int K, int cu_budget) {
  check_mx_shape(M, N, K, "gemm_mx_workgroups");
  return fp8_tile_128(M, N, cu_budget) ? (M / 128) * (N / 128) : (M / 64) * (N / 64);
}

void gemm_mx_nt(uintptr_t a, uintptr_t a_scales, uintptr_t w, uintptr_t w_scales, uintptr_t c, uintptr_t bias, int M,
                int N, int K, int lda, int ld_a_scales, int ldw, int ld_w_scales, int ldc, int a_fmt, bool relu,
                uintptr_t stream, int cu_budget) {
  check_mx_shape(M, N, K, "gemm_mx");
  if (a_fmt != kMxFp8 && a_fmt != kMxFp4) throw std::runtime_error("gemm_mx: a_fmt must be 0 (fp8) or 4 (fp4)");
  const bool a4 = a_fmt == kMxFp4;
  if (!a || !a_scales || !w || !w_scales || !c) throw std::runtime_error("gemm_mx: a, w, their scales and c are needed");
  if (lda < (a4 ? K / 2 : K) || ldw < K / 2 || lda % 16 || ldw % 16 || a % 16 || w % 16)
    throw std::runtime_error("gemm_mx: element rows must be 16-byte aligned and at least a row long");
  if (ld_a_scales < K / 32 || ld_w_scales < K / 32) throw std::runtime_error("gemm_mx: scale row strides < K / 32");
  if (ldc < N || ldc % 4 || c % 8) throw std::runtime_error("gemm_mx: C rows must be 8-byte aligned");
  if (bias) check_align(reinterpret_cast<void*>(bias), "bias");
  const MxArgs g{reinterpret_cast<const uint8_t*>(a), reinterpret_cast<const uint8_t*>(a_scales),
                 reinterpret_cast<const uint8_t*>(w), reinterpret_cast<const uint8_t*>(w_scales),
                 reinterpret_cast<__bf16*>(c), reinterpret_cast<const float*>(bias), M, N, K, lda, ld_a_scales, ldw,
                 ld_w_scales, ldc, relu, reinterpret_cast<hipStream_t>(stream)};
  const bool big = fp8_tile_128(M, N, cu_budget);
  if (big && a4) launch_act<128, 128, true>(g);
  else if (big) launch_act<128, 128, false>(g);
  else if (a4) launch_act<64, 64, true>(g);
  else launch_act<64, 64, false>(g);
  HIP_CHECK(hipGetLastError());
}

}  // namespace gs
