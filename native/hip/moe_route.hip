// MoE routing (gfx950 / MI355X): one op, two launches -- the per-token top-k + softmax of the router's logits, and
// the "align" step that sorts the T * k (token, choice) slots by expert into the tile-aligned layout the grouped
// expert GEMM (moe_gemm.hip) and the combine (moe_combine.hip) share.
//
// (a) moe_topk_kernel: one wave per token, four tokens per 256-thread workgroup.  Lane l holds the logits
//     l, l + 64, l + 128, l + 192 of its row (E <= 256) as 25-bit integers ((order key + 1) << 8) | (255 - index):
//     the order key is the bf16 code made monotonic (-0 folded into +0 first: comparisons are on values), so the
//     integer maximum is the largest value and, among equal values, the lowest index.  k <= 8 rounds of a per-lane
//     maximum and a 6-step wave butterfly pick the k winners in rank order; a winner is struck out (0 is below
//     every real entry), so the ids are k distinct values in [0, E) whatever the data -- a NaN is just a key.
//     Weights: e_j = exp2((l_j - l_0) * 1.44269504f) -- one fp32 subtract, one fp32 multiply, v_exp_f32 --, a
//     sum over j = 0 .. k - 1 in that order, an IEEE division.  No float atomics, nothing order-dependent.
// (b) moe_align_kernel: ONE workgroup of 1,024 threads (T * k <= 32,768 slots: their expert ids are 32 KiB of LDS
//     bytes).  With n = T * k, c_e the slots of expert e and off[e + 1] - off[e] = 64 * ceil(c_e / 64):
//       sorted_ids[off[e] + r] = the r-th slot of expert e in ascending slot order (stable), r < c_e; n elsewhere
//       tile_expert[i]         = the expert of rows [64 i, 64 i + 64); -1 past off[E] / 64
//       expert_offsets[e]      = off[e], e = 0 .. E
//       slot_pos[s]            = the row of sorted_ids that holds s
//     Wave w takes the w-th contiguous run of 64-slot groups.  Pass 1 counts (wave, expert) pairs with LDS integer
//     atomics (a count does not depend on their order); thread e then turns its column of counts into the first row
//     of every (wave, expert) pair and writes expert e's offsets, tile experts and pad rows; pass 2 walks each wave's
//     groups in order, ranks the lanes of one expert inside a group with ballots, and writes.  Every element of all
//     four arrays is written exactly once per launch, so they may hold anything before and a replay gives the same.
//
// No bounds checks on the operands by design: the host wrapper (ops/loadgen.py moe_route) validates them.  The ids the
// align step reads are clamped into [0, E), so no data can make it index out of range.
// moe_topk_kernel: 20 VGPRs, no LDS, no scratch; moe_align_kernel: 44 VGPRs, 52,240 bytes of LDS, no scratch.
// Measured on an MI355X (profiles/r15_moe; both launches, replayed from a graph): 18.7 us for 256 tokens x 128 experts x
// top-8, 83.4 us for 2,048 tokens (16,384 slots through the one align workgroup).
#include "api.h"
#include "common.h"

namespace gs {
namespace {

constexpr int kTopkThreads = 256;
constexpr int kTokensPerWorkgroup = kTopkThreads / kWave;
constexpr int kAlignThreads = 1024;
constexpr int kAlignWaves = kAlignThreads / kWave;
constexpr int kMaxExperts = 256, kMaxTopK = 8, kMaxSlots = 32768, kBlockM = 64;

__device__ __forceinline__ unsigned order_entry(unsigned b, int idx) {
  if (b == 0x8000u) b = 0;                                           // -0 == +0
  const unsigned key = (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u);
  return ((key + 1) << 8) | (unsigned)(255 - idx);
}

__device__ __forceinline__ float entry_value(unsigned entry) {
  const unsigned key = (entry >> 8) - 1;
  const unsigned b = (key & 0x8000u) ? (key & 0x7FFFu) : (~key & 0xFFFFu);
  return __uint_as_float(b << 16);
}

__global__ void __launch_bounds__(kTopkThreads) moe_topk_kernel(const unsigned short* __restrict__ logits, size_t ld, int T,
                                                                int E, int k, int* __restrict__ topk_ids,
                                                                float* __restrict__ topk_w) {
  const int lane = threadIdx.x & (kWave - 1);
  const int t = blockIdx.x * kTokensPerWorkgroup + (int)(threadIdx.x / kWave);
  if (t >= T) return;                                                // wave-uniform; the kernel has no barrier
  const unsigned short* row = logits + (size_t)t * ld;
  unsigned c[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = lane + kWave * i;
    c[i] = idx < E ? order_entry(row[idx], idx) : 0u;
  }
  int my_id = 0;
  float my_l = 0.f, l0 = 0.f;
  for (int j = 0; j < k; ++j) {
    unsigned m = max(max(c[0], c[1]), max(c[2], c[3]));
#pragma unroll
    for (int o = kWave / 2; o; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (c[i] == m) c[i] = 0u;                                      // the index is part of the entry: one lane, one slot
    const float v = entry_value(m);
    if (j == 0) l0 = v;
    if (lane == j) {
      my_id = 255 - (int)(m & 255u);
      my_l = v;
    }
  }
  const float e = __builtin_amdgcn_exp2f(__fmul_rn(__fsub_rn(my_l, l0), 1.44269504f));
  float s = __shfl(e, 0);
  for (int j = 1; j < k; ++j) s = __fadd_rn(s, __shfl(e, j));
  if (lane < k) {
    topk_ids[t * k + lane] = my_id;
    topk_w[t * k + lane] = __fdiv_rn(e, s);
  }
}

__global__ void __launch_bounds__(kAlignThreads) moe_align_kernel(const int* __restrict__ topk_ids, int n, int E,
                                                                  int max_tiles, int* __restrict__ sorted_ids,
                                                                  int* __restrict__ tile_expert,
                                                                  int* __restrict__ expert_offsets,
                                                                  int* __restrict__ slot_pos) {
  __shared__ unsigned char eid[kMaxSlots];
  __shared__ int cnt[kAlignWaves][kMaxExperts];          // counts, then the next free row of each (wave, expert)
  __shared__ int total[kMaxExperts], padded[kMaxExperts], off[kMaxExperts + 1];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  for (int i = tid; i < kAlignWaves * kMaxExperts; i += kAlignThreads) (&cnt[0][0])[i] = 0;
  __syncthreads();
  const int groups = (n + kWave - 1) / kWave, per_wave = (groups + kAlignWaves - 1) / kAlignWaves;
  const int g0 = min(wave * per_wave, groups), g1 = min(g0 + per_wave, groups);
  for (int g = g0; g < g1; ++g) {
    const int s = g * kWave + lane;
    if (s < n) {
      const int e = min(max(topk_ids[s], 0), E - 1);
      eid[s] = (unsigned char)e;
      atomicAdd(&cnt[wave][e], 1);
    }
  }
  __syncthreads();
  if (tid < E) {
    int run = 0;
    for (int w = 0; w < kAlignWaves; ++w) {
      const int c = cnt[w][tid];
      cnt[w][tid] = run;
      run += c;
    }
    total[tid] = run;
    padded[tid] = (run + kBlockM - 1) / kBlockM * kBlockM;
  }
  __syncthreads();
  if (tid < E) {
    int o = 0;
    for (int e = 0; e < tid; ++e) o += padded[e];
    const int end = o + padded[tid];
    off[tid] = o;
    expert_offsets[tid] = o;
    if (tid == E - 1) {
      off[E] = end;
      expert_offsets[E] = end;
    }
    for (int w = 0; w < kAlignWaves; ++w) cnt[w][tid] += o;
    for (int r = o + total[tid]; r < end; ++r) sorted_ids[r] = n;
    for (int i = o / kBlockM; i < end / kBlockM; ++i) tile_expert[i] = tid;
  }
  __syncthreads();
  const int end = off[E];
  for (int r = end + tid; r < max_tiles * kBlockM; r += kAlignThreads) sorted_ids[r] = n;
  for (int i = end / kBlockM + tid; i < max_tiles; i += kAlignThreads) tile_expert[i] = -1;
  for (int g = g0; g < g1; ++g) {
    const int s = g * kWave + lane;
    const bool valid = s < n;
    const int e = valid ? (int)eid[s] : -1;
    int rank = 0, mine = 0;
    unsigned long long todo = __ballot(valid);
    while (todo) {                                                   // one round per distinct expert of the group
      const int leader = __ffsll((long long)todo) - 1;
      const int el = __shfl(e, leader);
      const unsigned long long same = __ballot(e == el);
      if (e == el) {
        rank = __popcll(same & ((1ull << lane) - 1ull));
        mine = __popcll(same);
      }
      todo &= ~same;
    }
    if (valid) {
      const int pos = cnt[wave][e] + rank;
      sorted_ids[pos] = s;
      slot_pos[s] = pos;
    }
    if (valid && rank == 0) cnt[wave][e] += mine;                    // after every lane's read above (one wave, in order)
  }
}

}  // namespace

int moe_max_tiles(int T, int k, int E) {
  if (T < 0 || k < 1 || k > kMaxTopK || E < 1 || E > kMaxExperts)
    throw std::runtime_error("moe: T must be >= 0, top_k in [1, 8] and E in [1, 256]");
  const int64_t n = (int64_t)T * k;
  if (n > kMaxSlots) throw std::runtime_error("moe: more than 32768 (token, choice) slots");
  const int64_t by_pad = (n + (int64_t)(kBlockM - 1) * E) / kBlockM;
  return (int)(n < by_pad ? n : by_pad);
}

int moe_route_workgroups(int T) {
  if (T < 0) throw std::runtime_error("moe_route: T must be >= 0");
  return (T + kTokensPerWorkgroup - 1) / kTokensPerWorkgroup;
}

void moe_route_bf16(uintptr_t logits, uintptr_t topk_ids, uintptr_t topk_w, uintptr_t sorted_ids, uintptr_t tile_expert,
                    uintptr_t expert_offsets, uintptr_t slot_pos, int T, int E, int k, int64_t ld_logits,
                    uintptr_t stream) {
  const int max_tiles = moe_max_tiles(T, k, E);
  if (E < 8 || E % 8 || k > E) throw std::runtime_error("moe_route: E must be a multiple of 8 in [8, 256] and top_k <= E");
  if (ld_logits < E || ld_logits % 8) throw std::runtime_error("moe_route: the logits row stride must be >= E and a multiple of 8");
  if (logits % 16) throw std::runtime_error("moe_route: logits must be 16-byte aligned");
  if (!expert_offsets || expert_offsets % 4) throw std::runtime_error("moe_route: expert_offsets is needed, 4-byte aligned");
  if (T > 0 && (!logits || !topk_ids || !topk_w || !sorted_ids || !tile_expert || !slot_pos))
    throw std::runtime_error("moe_route: every operand is needed");
  if (topk_ids % 4 || topk_w % 4 || sorted_ids % 4 || tile_expert % 4 || slot_pos % 4)
    throw std::runtime_error("moe_route: the int32 / fp32 operands must be 4-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (T > 0) {
    hipLaunchKernelGGL(moe_topk_kernel, dim3(moe_route_workgroups(T)), dim3(kTopkThreads), 0, st,
                       reinterpret_cast<const unsigned short*>(logits), (size_t)ld_logits, T, E, k,
                       reinterpret_cast<int*>(topk_ids), reinterpret_cast<float*>(topk_w));
    HIP_CHECK(hipGetLastError());
  }
  // T == 0: nothing is read; the E + 1 offsets (all 0) are the whole layout
  hipLaunchKernelGGL(moe_align_kernel, dim3(1), dim3(kAlignThreads), 0, st, reinterpret_cast<const int*>(topk_ids), T * k, E,
                     max_tiles, reinterpret_cast<int*>(sorted_ids), reinterpret_cast<int*>(tile_expert),
                     reinterpret_cast<int*>(expert_offsets), reinterpret_cast<int*>(slot_pos));
  HIP_CHECK(hipGetLastError());
}

}  // namespace gs
