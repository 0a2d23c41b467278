// Top-k / top-p token sampling (gfx950 / MI355X): the last step of a decode iteration, the choice of the next
// token from the LM head's logits.  One very long bf16 row per sequence in, an exact selection of its k largest
// elements, a short sorted softmax over the survivors, 4 bytes out.
//
// logits bf16 [S, V] (row stride ld_logits in elements, 64-bit row offsets), temperature fp32 [S], top_k int32 [S],
// top_p fp32 [S], u fp32 [S] (caller-supplied uniforms in [0, 1): there is no RNG in the kernel, so a replayed graph
// is idempotent), out int32 [S].  V is a multiple of 8 in [8, 131072].
//
// Row-level rules:
//  * Comparisons are on values: +0.0 == -0.0.
//  * A row that holds any NaN, or whose maximum is -Inf, gives token -1.  No other row is affected.
//  * A row whose maximum is +Inf gives the lowest index holding +Inf, in either mode.
//  * Greedy (temperature == 0 or top_k == 1): the token is the lowest index of the row maximum.  No exponential is
//    computed.  u and top_p are not read as numbers and may be NaN.
// Candidates:
//  * k = min(clamp(top_k, 1, 64), V).
//  * The candidates are the k largest logits.  Ties at the threshold value go to the lowest indices.
//  * They are ranked c_0 .. c_{k-1} by (value descending, index ascending).
//  * The kernel itself clamps top_k into [1, 64] (one v_med3): an out-of-range value cannot run past the LDS
//    candidate array.
// Weights:
//  * c = 1.44269504f / temperature is an IEEE division.
//  * a_j = (l_{c_j} - l_{c_0}) * c is one fp32 subtraction and one fp32 multiply.
//  * w_j is the hardware exp2 (v_exp_f32) of a_j, as in swiglu.hip and the attentions.
//  * Consequences: w_0 == 1 exactly; equal logits give exactly 1; a_j <= -150 (and -Inf) gives exactly 0.
// Cumulative sum:
//  * cum_j is the inclusive fp32 prefix sum of w in rank order.
//  * The association is unspecified but fixed (here: a 6-step wave scan, lane j adding the sum of the lanes
//    (j - 2s, j - s] to its own at step s = 1, 2, 4 .. 32).
//  * There are no float atomics, so two launches on the same inputs give identical tokens.
//  * Z = cum_{k-1}.
// Top-p:
//  * n is the smallest n >= 1 with cum_{n-1} >= top_p * Z (one fp32 multiply).
//  * top_p == 1 keeps all k.
// Pick:
//  * target = u * cum_{n-1}.
//  * The token is c_j for the smallest j < n with cum_j > target.
//  * If no such j exists, the token is c_{n-1}.
// Memory:
//  * Nothing outside the S x V window and the five [S] vectors is read.
//  * Only out[0..S) is written.
//
// Shape of the kernel (what was chosen and why):
//
//  * one 1,024-thread workgroup per row (sample_workgroups = S).  Thread t owns the 16-byte chunks t, t + 1024,
//    .. t + 15 * 1024 of the row -- those with 8 * chunk < V: "round" r is the chunks [1024 r, 1024 r + 1024), a
//    wave's load instruction one coalesced 1 KiB access.  Every logit byte is read once and then lives in
//    registers (64 VGPRs), two elements per register, for all passes;
//  * the registers hold not the bf16 codes but their 16-bit ORDER KEYS: key = code + 0x8000 for a code without
//    the sign bit, 0x10000 - code with it (four packed 16-bit operations per two elements, once).  The map is
//    monotonic in the value, has no hole, sends +0.0 and -0.0 to the same key 0x8000, -Inf to 0x0080 and +Inf
//    to 0xFF80; exactly the NaNs lie outside [0x0080, 0xFF80].  The chunks past the row's end are filled with
//    the key of -Inf: they rank below or equal to every element and, on a tie, behind it (their index is >= V),
//    and k <= V, so none is ever a candidate.  The value of a candidate is rebuilt from its key;
//  * pass 1: packed 16-bit maximum and minimum of the thread's keys, a wave butterfly and the 16 wave
//    partials through LDS (integers: any order gives the same) -- the row maximum and the NaN flag;
//  * the selection is exact because there are only 65,536 keys.  An LDS histogram counts the elements by
//    their key distance from the maximum's key, a window of distances at a time: [0, 16), [16, 64), [64, 128),
//    [128, 256), then 256 more per step (narrow windows first: a window a whole binade wide already holds a
//    percent of a normally distributed row, and every element inside a window costs an LDS atomic).  Wave 0
//    scans each window's bins on top of the count above the window, and the walk stops in the window where
//    the cumulative count reaches k: that bin is the threshold key T, with
//    `above` elements over it and k - above ties to admit.  The register scan of a window tests two elements
//    with one packed maximum against the window's lower edge, so a pass costs two instructions per register
//    unless an element is inside; only those touch LDS, with integer atomics (order-independent).  For
//    logits like a language model's the top 64 lie within half a binade (64 codes) of the maximum and the walk
//    takes two or three windows; a row whose top values are spread over the whole range takes up to 259, each
//    a pass over the registers and two barriers (the "staircase" figure below);
//  * compaction: the elements over T, and the ties where all of T's elements are admitted, are appended to a
//    64-entry LDS array of (key, index) words through an LDS counter -- in any order, the ranking below is a
//    total order.  Where T has more elements than ties to admit, they are ranked by index first: the tie
//    count of every (round, wave) -- 512 consecutive indices -- goes into the 256 bins, wave 0 turns them into
//    exclusive prefix counts, and a wave whose prefix is below the tie count ranks its own ties with a wave
//    scan over its lanes and the order of the elements inside a chunk;
//  * wave 0 ranks the k words by counting, for each, the words larger than it ((key << 17) | (131071 -
//    index): value descending, index ascending), rebuilds the logits, and computes weights, scan, cut and pick;
//    lane 0 writes the token.  A greedy row, and a row whose maximum is +Inf, runs the same selection with
//    k = 1 and writes c_0;
//  * built without -ffast-math: the division is v_div_scale / v_div_fmas / v_div_fixup.
//
// No bounds checks here by design beyond the top_k clamp: the host wrapper (ops/loadgen.py sample_tokens)
// validates shapes, strides, alignment and overlap.
// 96 VGPRs (64 of them the row), no AGPRs, 104 SGPRs (74 more kept in VGPR lanes: the unrolled scans nest many
// exec masks), 2,136 bytes of LDS, no scratch; the registers would allow 5 waves per SIMD, the 1,024-thread
// workgroup puts 4 there: one workgroup per CU.
// Measured on an MI355X as chains of launches replayed from one graph (profiles/r14_sample; temperature 0.8,
// top_k 50, top_p 0.9, logits bf16(1.5 * randn), V = 128,256): 24.1 us for 8 rows (8 workgroups on 256 CUs) and
// 30.0 us for 256 rows (one per CU, 64 MB from the Infinity Cache: 2.19 TB/s), 23.1 us for 256 greedy rows, against
// 9.7 us for one greedy row of 8 logits -- the cost of the passes alone; 355.8 us for 4,096 rows (1 GiB, from HBM):
// 2.95 TB/s, 0.50 of the stream triad's 5.92 TB/s on a 1 GiB working set in the same run, and 1 / 7.4 of the time of
// torch.topk(50) + softmax + cumsum on the same logits (1 / 7.1 at 256 rows, 1 / 2.9 at 8).  The kernel is bound
// by its passes over the registers, not by memory: a workgroup loads, then computes, and a CU holds one
// workgroup, so nothing overlaps the two.  The fallback: 256 staircase rows (the top 64 values 3 binades apart
// from one another, across zero: about 135 windows) take 383.6 us, and one row of 8 logits sampled with k = 8 -- the
// candidates on both sides of zero -- 318.8 us: the walk does not skip empty windows.  With [64, 256) as one
// window the 256 rows took 32.5 us: about one row in eight has a maximum so far out that the top 50 reach past
// the first 64 codes, and a window that wide holds 13 % of the row.  Not measured: other workgroup sizes and
// chunk counts per thread, other window sequences, a trained model's logits, co-run groups.
#include "api.h"
#include "paged_attn.h"

namespace gs {
namespace {

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / kWave;
constexpr int kRounds = 16;                              // 16-byte chunks of a row per thread
constexpr int kMaxV = 8 * kThreads * kRounds;            // 131072
constexpr int kMaxK = 64;                                // candidates: one wave ranks and scans them
constexpr int kBins = 256;                               // histogram bins: a window of key distances, or (round, wave)
constexpr uint32_t kKeyNegInf = 0x0080, kKeyPosInf = 0xFF80;
constexpr uint32_t kIdxMask = kMaxV - 1;
static_assert(kRounds * kWaves == kBins, "one bin per (round, wave)");

// the order keys of two packed bf16 codes
__device__ __forceinline__ uint32_t to_keys(uint32_t w) {
  const u16x2 m = __builtin_bit_cast(u16x2, (i16x2)(__builtin_bit_cast(i16x2, w) >> 15));      // 0xFFFF where negative
  const u16x2 x = __builtin_bit_cast(u16x2, w) ^ (m | u16x2{0x8000, 0x8000});
  return __builtin_bit_cast(uint32_t, (u16x2)(x - m));
}

__device__ __forceinline__ uint32_t pk_max(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}

__device__ __forceinline__ uint32_t pk_min(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}

__device__ __forceinline__ float key_value(uint32_t key) {
  const uint32_t code = key >= 0x8000u ? key - 0x8000u : (0x10000u - key) & 0xFFFFu;
  return __uint_as_float(code << 16);
}

// f(key, index) for every element of the thread whose key is > floor_key (floor_key in [0, 0xFFFF])
template <class F>
__device__ __forceinline__ void for_keys_above(const uint32_t (&kv)[kRounds][4], int tid, uint32_t floor_key, F&& f) {
  const uint32_t f2 = floor_key | floor_key << 16;
#pragma unroll
  for (int r = 0; r < kRounds; ++r)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t v = kv[r][q];
      if (pk_max(v, f2) != f2) {
        asm volatile("" : "+v"(v));                      // keeps the unpacking inside the branch, out of the caller's loop
        const int idx = ((r * kThreads + tid) << 3) + 2 * q;
        const uint32_t lo = v & 0xFFFFu, hi = v >> 16;
        if (lo > floor_key) f(lo, idx);
        if (hi > floor_key) f(hi, idx + 1);
      }
    }
}

// the elements of round r's chunk with key == T counted; those with key > T handed to f where kAppend
template <bool kAppend, class F>
__device__ __forceinline__ int count_ties(const uint32_t (&v)[4], int idx0, uint32_t T, F&& f) {
  const uint32_t fl = T - 1, f2 = fl | fl << 16;
  int c = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (pk_max(v[q], f2) != f2) {
      const uint32_t lo = v[q] & 0xFFFFu, hi = v[q] >> 16;
      c += (lo == T) + (hi == T);
      if (kAppend) {
        if (lo > T) f(lo, idx0 + 2 * q);
        if (hi > T) f(hi, idx0 + 2 * q + 1);
      }
    }
  return c;
}

__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t x, int lane) {
#pragma unroll
  for (int s = 1; s < kWave; s <<= 1) {
    const uint32_t t = __shfl_up(x, s, kWave);
    if (lane >= s) x += t;
  }
  return x;
}

__global__ void __launch_bounds__(kThreads) sample_topk_kernel(
    const __bf16* __restrict__ logits, const float* __restrict__ u, const float* __restrict__ temperature,
    const int* __restrict__ top_k, const float* __restrict__ top_p, int* __restrict__ out, int V, size_t ld_logits) {
  __shared__ uint32_t part[kWaves];
  __shared__ uint32_t hist[kBins];
  __shared__ unsigned long long cand[kMaxK], sorted[kMaxK];
  __shared__ uint32_t ncand, res_total, res_d, res_above, res_cnt;

  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const size_t row = blockIdx.x;
  const int nchunks = V >> 3;
  const __bf16* lr = logits + row * ld_logits;

  // the row, as keys
  uint32_t kv[kRounds][4];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int chunk = tid + r * kThreads;
    u32x4 w = {0xFF80FF80u, 0xFF80FF80u, 0xFF80FF80u, 0xFF80FF80u};        // -Inf past the row's end
    if (chunk < nchunks) w = *reinterpret_cast<const u32x4*>(lr + 8 * (size_t)chunk);
#pragma unroll
    for (int q = 0; q < 4; ++q) kv[r][q] = to_keys(w[q]);
  }
  if (tid < kBins) hist[tid] = 0;
  if (tid == 0) ncand = 0;

  // pass 1: the largest and the smallest key of the row
  uint32_t mx = kv[0][0], mn = kv[0][0];
#pragma unroll
  for (int r = 0; r < kRounds; ++r)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      mx = pk_max(mx, kv[r][q]);
      mn = pk_min(mn, kv[r][q]);
    }
  mx = max(mx & 0xFFFFu, mx >> 16);
  mn = min(mn & 0xFFFFu, mn >> 16);
  uint32_t both = mx << 16 | (0xFFFFu - mn);
#pragma unroll
  for (int m = kWave / 2; m > 0; m >>= 1) {
    const uint32_t o = __shfl_xor(both, m, kWave);
    both = max(both & 0xFFFF0000u, o & 0xFFFF0000u) | max(both & 0xFFFFu, o & 0xFFFFu);
  }
  if (lane == 0) part[wave] = both;
  __syncthreads();
  mx = 0;
  mn = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) {
    mx = max(mx, part[i] >> 16);
    mn = max(mn, part[i] & 0xFFFFu);
  }
  const int maxkey = (int)mx;
  const uint32_t minkey = 0xFFFFu - mn;
  if (maxkey > (int)kKeyPosInf || minkey < kKeyNegInf || maxkey == (int)kKeyNegInf) {      // a NaN, or all -Inf
    if (tid == 0) out[row] = -1;
    return;
  }

  const float temp = temperature[row];
  int k = __builtin_amdgcn_readfirstlane(min(max(top_k[row], 1), kMaxK));
  const bool greedy = temp == 0.f || k == 1 || maxkey == (int)kKeyPosInf;
  if (greedy) k = 1;
  k = min(k, V);

  // the threshold key: windows of key distances from the maximum, until the cumulative count reaches k
  int lo = 0, hi = 16;
  uint32_t carry = 0;                                    // elements above the window
  for (;;) {
    const int fl = max(maxkey - hi, 0);                  // key > maxkey - hi: distance < hi
    for_keys_above(kv, tid, (uint32_t)fl, [&](uint32_t key, int) {
      const int d = maxkey - (int)key;
      if (d >= lo) atomicAdd(&hist[d - lo], 1u);
    });
    __syncthreads();
    if (wave == 0) {
      uint32_t b[4], local = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        b[i] = hist[4 * lane + i];
        hist[4 * lane + i] = 0;
        local += b[i];
      }
      const uint32_t incl = wave_inclusive_sum(local, lane);
      const uint32_t total = __shfl(incl, kWave - 1, kWave);
      uint32_t before = carry + incl - local;
      if (before < (uint32_t)k && before + local >= (uint32_t)k) {          // one lane at the most
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (before < (uint32_t)k && before + b[i] >= (uint32_t)k) {
            res_d = lo + 4 * lane + i;
            res_above = before;
            res_cnt = b[i];
          }
          before += b[i];
        }
      }
      if (lane == 0) res_total = carry + total;
    }
    __syncthreads();
    carry = res_total;
    if (carry >= (uint32_t)k) break;
    lo = hi;
    hi = hi == 16 ? 64 : hi == 64 ? 128 : hi == 128 ? 256 : hi + 256;
  }
  const uint32_t T = (uint32_t)maxkey - res_d;
  const int ties = k - (int)res_above;
  auto append = [&](uint32_t key, int idx) {
    const uint32_t slot = atomicAdd(&ncand, 1u);
    cand[slot] = (unsigned long long)key << 17 | (kIdxMask - (uint32_t)idx);
  };

  if (res_cnt == (uint32_t)ties) {
    for_keys_above(kv, tid, T - 1, append);              // every element at T is a candidate
  } else {
    // more elements at T than places: the lowest indices.  Bin (r, wave) counts 512 consecutive indices
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
      const int c = count_ties<true>(kv[r], (r * kThreads + tid) << 3, T, append);
      if (c) atomicAdd(&hist[r * kWaves + wave], (uint32_t)c);
    }
    __syncthreads();
    if (wave == 0) {
      uint32_t b[4], local = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        b[i] = hist[4 * lane + i];
        local += b[i];
      }
      uint32_t before = wave_inclusive_sum(local, lane) - local;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        hist[4 * lane + i] = before;
        before += b[i];
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
      const int off = __builtin_amdgcn_readfirstlane((int)hist[r * kWaves + wave]);
      if (off < ties) {
        const int idx0 = (r * kThreads + tid) << 3;
        const int c = count_ties<false>(kv[r], idx0, T, append);
        if (__ballot(c > 0)) {
          int rank = off + (int)(wave_inclusive_sum((uint32_t)c, lane)) - c;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if ((kv[r][q] & 0xFFFFu) == T && rank++ < ties) append(T, idx0 + 2 * q);
            if ((kv[r][q] >> 16) == T && rank++ < ties) append(T, idx0 + 2 * q + 1);
          }
        }
      }
    }
  }
  __syncthreads();

  // wave 0: rank the k candidates by (key descending, index ascending)
  if (wave == 0 && lane < k) {
    const unsigned long long mine = cand[lane];
    int rank = 0;
    for (int i = 0; i < k; ++i) rank += cand[i] > mine;
    sorted[rank] = mine;
  }
  __syncthreads();
  if (wave != 0) return;
  const unsigned long long p = lane < k ? sorted[lane] : 0ull;
  const int idx = (int)(kIdxMask - ((uint32_t)p & kIdxMask));
  if (greedy) {
    if (lane == 0) out[row] = idx;
    return;
  }
  const float l = key_value((uint32_t)(p >> 17));
  const float c = 1.44269504f / temp;
  const float a = __fmul_rn(__fsub_rn(l, __shfl(l, 0, kWave)), c);
  float cum = lane < k ? __builtin_amdgcn_exp2f(a) : 0.f;
#pragma unroll
  for (int s = 1; s < kWave; s <<= 1) {
    const float t = __shfl_up(cum, s, kWave);
    if (lane >= s) cum = __fadd_rn(cum, t);
  }
  const float Z = __shfl(cum, k - 1, kWave);
  const float cut = __fmul_rn(top_p[row], Z);
  const unsigned long long kept = __ballot(lane < k && cum >= cut);
  const int n = kept ? __ffsll(kept) : k;
  const float target = __fmul_rn(u[row], __shfl(cum, n - 1, kWave));
  const unsigned long long over = __ballot(lane < n && cum > target);
  const int pick = over ? __ffsll(over) - 1 : n - 1;
  const int token = __shfl(idx, pick, kWave);
  if (lane == 0) out[row] = token;
}

}  // namespace

int sample_workgroups(int S) {
  if (S < 0) throw std::runtime_error("sample_topk: negative S");
  return S;
}

void sample_topk_bf16(uintptr_t logits, uintptr_t u, uintptr_t temperature, uintptr_t top_k, uintptr_t top_p,
                      uintptr_t out, int S, int V, int64_t ld_logits, uintptr_t stream) {
  if (S < 0) throw std::runtime_error("sample_topk: negative S");
  if (V < 8 || V > kMaxV || V % 8) throw std::runtime_error("sample_topk: V must be a multiple of 8 in [8, 131072]");
  if (ld_logits < V || ld_logits % 8)
    throw std::runtime_error("sample_topk: the row stride must be >= V and a multiple of 8 elements");
  if (!logits || !u || !temperature || !top_k || !top_p || !out)
    throw std::runtime_error("sample_topk: logits, u, temperature, top_k, top_p and out are needed");
  if (logits % 16) throw std::runtime_error("sample_topk: logits must be 16-byte aligned");
  if (u % 4 || temperature % 4 || top_k % 4 || top_p % 4 || out % 4)
    throw std::runtime_error("sample_topk: u / temperature / top_k / top_p / out must be 4-byte aligned");
  const int grid = sample_workgroups(S);
  if (grid == 0) return;
  hipLaunchKernelGGL(sample_topk_kernel, dim3(grid), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const __bf16*>(logits), reinterpret_cast<const float*>(u),
                     reinterpret_cast<const float*>(temperature), reinterpret_cast<const int*>(top_k),
                     reinterpret_cast<const float*>(top_p), reinterpret_cast<int*>(out), V, (size_t)ld_logits);
  HIP_CHECK(hipGetLastError());
}

}  // namespace gs
