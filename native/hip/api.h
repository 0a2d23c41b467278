// Declarations shared by the HIP sources and the pybind11 bindings.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace gs {
struct DevInfo {
  int index = 0;
  std::string name, arch, uuid, rocr_uuid, pci;
  int cus = 0, clock_khz = 0, mem_clock_khz = 0, warp = 0, l2_bytes = 0, max_threads = 0;
  size_t lds_per_block = 0, total_mem = 0, free_mem = 0;
  size_t heap_limit = 0, fifo_limit = 0, stack_limit = 0;
  int pci_bus = 0, pci_device = 0, pci_domain = 0;
};
int device_count();
std::vector<DevInfo> query_all();
uintptr_t create_masked_stream(const std::vector<uint32_t>& mask);
uintptr_t create_stream(int priority);
void destroy_stream(uintptr_t s);
std::vector<uint32_t> get_stream_mask(uintptr_t s);
std::vector<uint32_t> probe_xcd(uintptr_t stream, int n);
void gemm_bf16_nt(uintptr_t a, uintptr_t bt, uintptr_t c, uintptr_t bias, int M, int N, int K, int lda, int ldb,
                  int ldc, bool relu, uintptr_t stream, int cu_budget, uintptr_t workspace = 0,
                  size_t workspace_floats = 0);
int pick_split_k(int M, int N, int K, int cu_budget);
size_t splitk_workspace_floats(int M, int N, int K, int cu_budget);
void gemm_fp8_nt(uintptr_t a, uintptr_t bt, uintptr_t c, uintptr_t bias, int M, int N, int K, int lda, int ldb,
                 int ldc, bool relu, uintptr_t stream, int cu_budget);
void stream_triad(uintptr_t a, uintptr_t b, uintptr_t c, float s, size_t n_floats, int blocks, uintptr_t stream);
// out[b, :] = bf16(sum of table[idx[j], :] over j in [offsets[b], offsets[b+1])) -- native/hip/gather.hip;
// strides in elements, blocks > 0 caps the grid (the workgroups then walk the bags grid-stride)
void embedding_bag_bf16(uintptr_t table, uintptr_t idx, uintptr_t offsets, uintptr_t out, int B, int D,
                        int64_t ld_table, int64_t ld_out, int blocks, uintptr_t stream);
// workgroups of that launch
int embedding_bag_workgroups(int B, int blocks);
// out[s, h, :] = bf16(softmax(scale * q[s, h, :] . K^T) . V) over the ctx_lens[s] tokens block_table[s, :]
// names -- native/hip/decode_attn.hip; k_cache [NB, Hkv, 32, 128], v_cache [NB, Hkv, 128, 32], q / out
// [S, Hq, 128] with sequence strides ld_q / ld_out, block_table rows ld_table apart (strides in elements)
void paged_decode_bf16(uintptr_t q, uintptr_t k_cache, uintptr_t v_cache, uintptr_t block_table, uintptr_t ctx_lens,
                       uintptr_t out, int S, int Hq, int Hkv, int64_t ld_q, int64_t ld_out, int64_t ld_table,
                       float scale, uintptr_t stream);
// workgroups of that launch: one per (sequence, KV head)
int paged_decode_workgroups(int S, int Hkv);
// The same attention as a split-KV launch pair for a few long sequences (decode_attn.hip tells the partition
// rule): kv_splits in [2, 32] workgroups per (sequence, KV head) write fp32 partials to `workspace` (16-byte
// aligned, paged_decode_split_workspace_floats elements, one launch in flight per workspace), a merge kernel
// on the same stream combines them into out
void paged_decode_split_bf16(uintptr_t q, uintptr_t k_cache, uintptr_t v_cache, uintptr_t block_table,
                             uintptr_t ctx_lens, uintptr_t workspace, uintptr_t out, int S, int Hq, int Hkv,
                             int kv_splits, int64_t ld_q, int64_t ld_out, int64_t ld_table, float scale,
                             uintptr_t stream);
// workgroups of the split kernel: one per (sequence, KV head, split)
int paged_decode_split_workgroups(int S, int Hkv, int kv_splits);
// fp32 elements of the workspace: 132 (128 accumulators, maximum, normaliser, 2 unused) per (sequence, head, split)
size_t paged_decode_split_workspace_floats(int S, int Hq, int kv_splits);
// Chunked-prefill (append) attention over the same cache -- native/hip/prefill_attn.hip: q / out [Tq, Hq, 128] packed
// over sequences with token strides ld_q / ld_out, the chunk of sequence s being rows q_start[s] .. q_start[s + 1] - 1
// (q_start int32 [S + 1]); query i of the chunk has position ctx_lens[s] - q_len[s] + i and attends tokens [0, position].
// max_q_len bounds every q_len (it sizes the grid); S == 0 or max_q_len == 0 launches nothing
void paged_prefill_bf16(uintptr_t q, uintptr_t k_cache, uintptr_t v_cache, uintptr_t block_table, uintptr_t ctx_lens,
                        uintptr_t q_start, uintptr_t out, int S, int Hq, int Hkv, int max_q_len, int64_t ld_q,
                        int64_t ld_out, int64_t ld_table, float scale, uintptr_t stream);
// workgroups of that launch: one per (sequence, KV head, tile of 128 (chunk token, head of the group) columns)
int paged_prefill_workgroups(int S, int Hq, int Hkv, int max_q_len);
// RoPE + append into the same cache -- native/hip/rope_append.hip: qkv [Tq, Hq + 2 Hkv, 128] (q heads, K heads, V heads;
// token stride ld_qkv), packed over the sequences by q_start like the prefill's q; row q_start[s] + i is token
// p = ctx_lens[s] - q_len[s] + i of s and goes to slot p % 32 of block block_table[s, p / 32]: q and K rotated
// (rotate-half pairing, cos_sin fp32 [max_pos, 128]: 64 cosines then 64 sines per position) to q_out [Tq, Hq, 128]
// (token stride ld_q_out) and k_cache, V copied bit for bit to v_cache.  The caches are never read
void rope_append_bf16(uintptr_t qkv, uintptr_t cos_sin, uintptr_t k_cache, uintptr_t v_cache, uintptr_t block_table,
                      uintptr_t ctx_lens, uintptr_t q_start, uintptr_t q_out, int S, int Hq, int Hkv, int max_q_len,
                      int max_pos, int64_t ld_qkv, int64_t ld_q_out, int64_t ld_table, uintptr_t stream);
// workgroups of that launch: one per (sequence, KV head, cache block a chunk of max_q_len tokens can touch):
// S * Hkv * ((max_q_len + 30) / 32 + 1), 0 where S == 0 or max_q_len == 0
int rope_append_workgroups(int S, int Hkv, int max_q_len);
// Residual add + RMSNorm -- native/hip/rmsnorm.hip: x, residual, res_out, y bf16 [T, D] with row strides (in elements),
// weight bf16 [D], D a multiple of 8 in [8, 8192].  res_out = bf16(x + residual); y = bf16((hb * r) * weight) with
// hb = fp32(res_out) and r = 1 / sqrt(mean(hb^2) + eps).  residual == 0: none -- hb = fp32(x), res_out (0 too) is not
// written.  res_out may be exactly residual; nothing else may overlap an output
void add_rmsnorm_bf16(uintptr_t x, uintptr_t residual /*0: none*/, uintptr_t weight, uintptr_t res_out, uintptr_t y,
                      int T, int D, int64_t ld_x, int64_t ld_res, int64_t ld_res_out, int64_t ld_y, float eps,
                      uintptr_t stream);
// workgroups of that launch: one per row
int add_rmsnorm_workgroups(int T);
// SwiGLU -- native/hip/swiglu.hip: gate_up bf16 [T, 2F] (gate columns [0, F), up columns [F, 2F)), out bf16 [T, F],
// F a multiple of 8, row strides in elements: out = bf16(g / (1 + exp2(-g * log2e)) * u)
void swiglu_bf16(uintptr_t gate_up, uintptr_t out, int T, int F, int64_t ld_in, int64_t ld_out, uintptr_t stream);
// workgroups of that launch: one per 1,024 16-byte output chunks of the flattened (row, chunk) space,
// ceil(T * F / 8192)
int swiglu_workgroups(int T, int F);
// Top-k / top-p token sampling -- native/hip/sample.hip: logits bf16 [S, V] (row stride ld_logits in elements), V a
// multiple of 8 in [8, 131072]; u, temperature, top_p fp32 [S], top_k int32 [S], out int32 [S].  Per row: the
// k = min(clamp(top_k, 1, 64), V) largest logits (ties to the lowest indices) ranked by (value descending, index
// ascending), weights exp2((l - l_max) * (1.44269504f / temperature)), a cut at top_p of their sum and the pick at u
// of what is kept; temperature == 0 or top_k == 1 is the lowest index of the maximum; a NaN in the row, or a
// maximum of -Inf, gives -1.  u holds the caller's uniforms in [0, 1): the kernel has no RNG
void sample_topk_bf16(uintptr_t logits, uintptr_t u, uintptr_t temperature, uintptr_t top_k, uintptr_t top_p,
                      uintptr_t out, int S, int V, int64_t ld_logits, uintptr_t stream);
// workgroups of that launch: one per row
int sample_workgroups(int S);
// Mixture-of-experts MLP -- native/hip/moe_route.hip, moe_gemm.hip, moe_combine.hip.  They share one layout of the
// n = T * k (token, choice) slots, s = t * k + j: sorted_ids int32 [64 * moe_max_tiles] (expert e owns rows
// [off[e], off[e + 1]), a multiple of 64; its slots first, ascending; n elsewhere), tile_expert int32 [moe_max_tiles]
// (-1: unused), expert_offsets int32 [E + 1] (off), slot_pos int32 [n] (the row that holds slot s).
// the least upper bound on the used 64-row tiles: min(T k, (T k + 63 E) / 64); T k <= 32768, k <= 8, E <= 256
int moe_max_tiles(int T, int k, int E);
// Routing: logits bf16 [T, E] (row stride ld_logits; E a multiple of 8 in [8, 256], k <= min(8, E)).  Launch 1: the k
// largest logits per token by (value descending, index ascending) to topk_ids int32 [T, k], and topk_w fp32 [T, k] =
// e_j / sum e with e_j = exp2((l_j - l_0) * 1.44269504f).  Launch 2 (one workgroup): the four layout arrays, every
// element written.  T == 0 reads nothing and writes the E + 1 offsets
void moe_route_bf16(uintptr_t logits, uintptr_t topk_ids, uintptr_t topk_w, uintptr_t sorted_ids, uintptr_t tile_expert,
                    uintptr_t expert_offsets, uintptr_t slot_pos, int T, int E, int k, int64_t ld_logits,
                    uintptr_t stream);
// workgroups of the top-k launch: one wave per token, ceil(T / 4) (the align launch is one workgroup)
int moe_route_workgroups(int T);
// Grouped expert GEMM: out[i, :] = bf16(a[src(i), :] . w[tile_expert[i / 64]]^T) for the rows of used tiles; w bf16
// [E, N, K] (row stride ldw, expert stride expert_stride), N and K multiples of 64; src(i) = sorted_ids[i] / gather_div,
// or i with gather_div == 0; a pad row (sorted_ids[i] >= n_slots) is written as +0.0, unused tiles are not touched
void moe_gemm_bf16(uintptr_t a, uintptr_t w, uintptr_t sorted_ids, uintptr_t tile_expert, uintptr_t out, int max_tiles,
                   int n_slots, int gather_div, int N, int K, int64_t lda, int64_t ldw, int64_t expert_stride,
                   int64_t ldc, uintptr_t stream);
// workgroups of that launch: moe_max_tiles(T, k, E) * (N / BN), BN = 128 where N % 128 == 0, else 64
int moe_gemm_workgroups(int T, int k, int E, int N);
// Combine: out[t, :] = bf16(sum_j topk_w[t, j] * y[slot_pos[t k + j], :]), fma in the order j = 0 .. k - 1; y bf16
// [P_max, D], out bf16 [T, D], D a multiple of 8
void moe_combine_bf16(uintptr_t y, uintptr_t slot_pos, uintptr_t topk_w, uintptr_t out, int T, int D, int k, int64_t ld_y,
                      int64_t ld_out, uintptr_t stream);
// workgroups of that launch: one thread per 16-byte output chunk, ceil(T * D / 2048)
int moe_combine_workgroups(int T, int D);
// MX operands -- native/hip/quant_mx.hip, gemm_mx.hip.  THE FORMAT (OCP Microscaling v1.0, block size 32 along the
// row): a matrix [rows, K], K a multiple of 32, is a pair (elements, scales).  scales: uint8 [rows, K / 32], one E8M0
// byte per (row, block), value 2^(b - 127), b = 255 is NaN.  elements, by format code (the MFMA's cbsz / blgp codes):
//   kMxFp4 = 4  e2m1 (sign, 2 exponent bits, 1 mantissa bit: magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6), two per byte,
//               element 2i in bits 3:0 of byte i: uint8 [rows, K / 2]
//   kMxFp8 = 0  OCP e4m3fn, one per byte: [rows, K]
// All row strides are in elements of the array they belong to (bytes, here).  THE QUANTISATION RULE, per block of 32
// bf16 inputs: e = the largest biased exponent field (bits >> 7) & 0xFF; emax = 2 (fp4) / 8 (fp8).  e == 255 (an Inf
// or NaN in the block): scale byte 255 and every element byte of the block 0x00.  Otherwise the scale byte is
// b = max(e - emax, 0) (at most 252; an all-zero or subnormal-amax block gets 0) and an element is v * 2^(127 - b),
// rounded to the element format to nearest, ties to even, saturated at the largest finite magnitude (6 / 448), the
// input's sign bit always carried (-0.0, and a negative value that rounds to zero, give 0x8 / 0x80).
constexpr int kMxFp8 = 0, kMxFp4 = 4;
// x bf16 [T, D] (D a multiple of 32, 16-byte aligned rows) -> q and scales of format fmt, every scale byte written;
// no overlap; T == 0 launches nothing
void quantize_mx_bf16(uintptr_t x, uintptr_t q, uintptr_t scales, int T, int D, int64_t ld_x, int64_t ld_q,
                      int64_t ld_scales, int fmt, uintptr_t stream);
// workgroups of that launch: one per 1,024 16-byte input chunks of the flattened (row, chunk) space, ceil(T * D / 8192)
int quantize_mx_workgroups(int T, int D);
// c[m, n] = act(sum_k a[m, k] w[n, k] + bias[n]), bf16 out: a of format a_fmt (kMxFp8 or kMxFp4), w always kMxFp4;
// M, N multiples of 64, K of 128; element rows 16-byte aligned; bias fp32, relu and cu_budget as gemm_fp8_nt
void gemm_mx_nt(uintptr_t a, uintptr_t a_scales, uintptr_t w, uintptr_t w_scales, uintptr_t c, uintptr_t bias, int M,
                int N, int K, int lda, int ld_a_scales, int ldw, int ld_w_scales, int ldc, int a_fmt, bool relu,
                uintptr_t stream, int cu_budget);
// workgroups of that launch: gemm_fp8_nt's tiles and fill rule (fp8_tile_128)
int gemm_mx_workgroups(int M, int N, int K, int cu_budget);
// the fill rule of gemm_fp8_nt and gemm_mx_nt (gemm.hip): 128 x 128 tiles, else 64 x 64
bool fp8_tile_128(int M, int N, int cu_budget);
// FP8 paged-KV cache -- native/hip/rope_append.hip, decode_attn_kv8.hip.  THE FP8 KV FORMAT: k_cache uint8
// [NB, Hkv, 32, 128] and v_cache uint8 [NB, Hkv, 128, 32], the logical layout of the bf16 caches with one OCP e4m3fn
// byte per element; k_scale and v_scale fp32 [Hkv] (4-byte aligned).  A stored byte c of KV head g stands for
// e4m3fn(c) * scale[g].  THE QUANTISATION RULE for an fp32 value z (the writer computes z = value / scale[g], an IEEE
// fp32 division): a NaN gives 0x7F | sign << 7; otherwise |z| is rounded to the nearest e4m3fn magnitude, ties to even
// (the subnormal step is 2^-9 below 2^-6), anything that rounds above 448, +-Inf included, saturates to 0x7E (448);
// z's sign bit is always carried (-0.0, and a negative value that rounds to zero, give 0x80).  e4m3fn -> bf16 is exact
// for all 254 non-NaN codes, so the readers dequantise in registers and keep the bf16 MFMAs.
// rope_append_bf16 into such a cache: q_out as there; K is quantised from the fp32 rotation result (not first rounded
// to bf16) divided by k_scale[g], V from float(v) / v_scale[g]
void rope_append_kv8(uintptr_t qkv, uintptr_t cos_sin, uintptr_t k_cache, uintptr_t v_cache, uintptr_t k_scale,
                     uintptr_t v_scale, uintptr_t block_table, uintptr_t ctx_lens, uintptr_t q_start, uintptr_t q_out,
                     int S, int Hq, int Hkv, int max_q_len, int max_pos, int64_t ld_qkv, int64_t ld_q_out,
                     int64_t ld_table, uintptr_t stream);
// paged_decode_bf16 / paged_decode_split_bf16 over such a cache: scores = mfma_sum * (scale * k_scale[g]), the two
// scalars multiplied once in fp32; out = bf16((acc / lsum) * v_scale[g]).  The split kernel's partials are unscaled by
// v_scale (the merge applies it); workgroups, workspace rows and the partition rule are the bf16 functions'
void paged_decode_kv8(uintptr_t q, uintptr_t k_cache, uintptr_t v_cache, uintptr_t k_scale, uintptr_t v_scale,
                      uintptr_t block_table, uintptr_t ctx_lens, uintptr_t out, int S, int Hq, int Hkv, int64_t ld_q,
                      int64_t ld_out, int64_t ld_table, float scale, uintptr_t stream);
void paged_decode_split_kv8(uintptr_t q, uintptr_t k_cache, uintptr_t v_cache, uintptr_t k_scale, uintptr_t v_scale,
                            uintptr_t block_table, uintptr_t ctx_lens, uintptr_t workspace, uintptr_t out, int S,
                            int Hq, int Hkv, int kv_splits, int64_t ld_q, int64_t ld_out, int64_t ld_table,
                            float scale, uintptr_t stream);
// paged_prefill_bf16 over such a cache -- native/hip/prefill_attn_kv8.hip: the same two scale rules, the division
// before v_scale; workgroups are paged_prefill_workgroups'; S == 0 or max_q_len == 0 launches nothing
void paged_prefill_kv8(uintptr_t q, uintptr_t k_cache, uintptr_t v_cache, uintptr_t k_scale, uintptr_t v_scale,
                       uintptr_t block_table, uintptr_t ctx_lens, uintptr_t q_start, uintptr_t out, int S, int Hq,
                       int Hkv, int max_q_len, int64_t ld_q, int64_t ld_out, int64_t ld_table, float scale,
                       uintptr_t stream);
// The launch knobs, each described once: name, min, max, default, kind.  Python gets set_<name> for every
// row, knobs(), knob_defaults() and reset_knobs() (bindings.cpp); C++ reads knob(k_<name>).  An ON_OFF knob
// takes any integer as on / off, a RANGE knob raises outside min..max.  What the values select is told where
// they are read (gemm.hip, triad.hip).
#define GS_KNOBS(X)                    \
  X(gemm_tile, 0, 16, 0, RANGE)        \
  X(gemm_policy, 0, 13, 10, RANGE)     \
  X(split_k, -1, 8, 0, RANGE)          \
  X(w4_probe, 0, 3, 0, RANGE)          \
  X(w4_prio, 0, 1, 0, ON_OFF)          \
  X(wide_epilogue, 0, 1, 1, ON_OFF)    \
  X(xcd_blocks, 0, 1, 1, ON_OFF)       \
  X(lone_plain_order, 0, 1, 1, ON_OFF) \
  X(xcd_group, 1, 64, 4, RANGE)        \
  X(triad_variant, 0, 10, 6, RANGE)
#define GS_KNOB_ID(name, lo, hi, def, kind) k_##name,
enum Knob { GS_KNOBS(GS_KNOB_ID) kNumKnobs };
enum KnobKind { RANGE, ON_OFF };
struct KnobInfo { const char* name; int min, max, def; KnobKind kind; };
extern const KnobInfo kKnobs[kNumKnobs];
extern int g_knob[kNumKnobs];
inline int knob(Knob k) { return g_knob[k]; }
void set_knob(Knob k, int value);
void reset_knobs();
void xcd_probe(uintptr_t out, int blocks, uintptr_t stream);
int pick_xcd_map(int tiles_m, int tiles_n);
int pick_gemm_tile(int M, int N, int cu_budget);
// What gemm_bf16_nt launches for a call, decided on the host alone: the launches in order (a policy-9 GEMM is
// several row slices [m0, m0 + m), a split-K GEMM the sliced kernel then splitk_reduce as tile 0) and the
// split factor.  wide_ok: the wide epilogue may run (the wide_epilogue knob is on and C rows are 16-byte
// aligned); workspace: the caller passes a split-K workspace.
struct GemmLaunch { int tile; const void* kernel; int grid, block, xmap, m0, m; };
struct GemmPlan { int split = 1; std::vector<GemmLaunch> launches; };
GemmPlan plan_gemm(int M, int N, int K, int cu_budget, bool relu, bool bias, bool wide_ok, bool workspace);
// workgroups of the GEMM launch this shape / CU budget gets (the kernel's CU footprint)
int gemm_workgroups(int M, int N, int K, int cu_budget, bool fp8, bool split_workspace);
std::vector<int> peer_access_matrix();
double peer_copy_gbps(int src, int dst, size_t bytes, int iters);
}  // namespace gs
