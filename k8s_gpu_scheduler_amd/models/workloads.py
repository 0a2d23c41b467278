"""Synthetic pod workloads (the "model families" the scheduler places).

The reference characterises 18 MLPerf-style inference workloads -- {onnx, tensorflow} x
{mobilenet, resnet50, ssd_mobilenet} x batch {1024, 2048, 4096} -- only through their
measured throughput per GPU share (reference
pkg/recommender/recommender/configurations_train.ods) and pairwise interference
(interference_train.ods).  There are no model binaries to run here, so each workload is
re-created as a kernel mix with the same *character* on MI355X, built from the native
load kernels (ops.loadgen):

  resnet50       compute-bound: a chain of bf16 MFMA GEMMs (+bias+ReLU fused)
  mobilenet      memory-bound: HBM triad passes (depthwise-like) + one small GEMM
  ssd_mobilenet  mixed: GEMMs and HBM streaming in similar proportion

The batch suffix scales the GEMM M dimension and the streamed bytes; the framework prefix
selects a different layer shape (onnx: 2048-wide, tensorflow: 1536/2560-wide).  One
*iteration* ("query batch") runs the op list once; a pod's throughput is iterations/s,
its SLO a minimum iterations/s -- the same semantics as the reference's SLO env
(SURVEY.md §2.7.1).

A third kernel character exists outside the catalog (EXTRA): "gather", the bf16 embedding-bag
(ops.loadgen.embedding_bag) -- memory-bound like the triad, but random table rows instead of a
stream, no MFMA work, and a rate that depends on where the rows sit (L2 > Infinity Cache > HBM).
A fourth is "attn", decode attention over a paged KV cache (ops.loadgen.paged_decode_attention):
HBM-bound too, but its traffic is 8 KiB cache slabs named by a block table, its two products run on
the matrix cores, and it has a softmax (transcendentals, cross-lane reductions) in the loop.
A fifth kernel character is "prefill", chunked-prefill attention over the same cache
(ops.loadgen.paged_prefill_attention): many new tokens per sequence attending causally, so every
cache slab is reused by all of them and the op is MFMA-bound -- but unlike a GEMM's, each of its
MFMAs sits behind exps, cross-lane maxima and a rescale of the accumulators.
A sixth is "attn_split", the decode attention of a FEW LONG sequences (LONG_CONTEXT): HBM-bound like
"attn", but S * Hkv workgroups would leave most CUs idle, so each (sequence, KV head) is split over
`splits` workgroups whose fp32 partials a second kernel merges -- CU-hungry only when split.
A seventh kernel character is "rope_append" (LLM_LAYER), the rotary embedding of q and K and the append
of the new K / V to the paged cache (ops.loadgen.rope_append): the one WRITER of that cache -- small,
latency-dominated and write-scattering (256-byte K rows and, for V, 2-byte-granular columns of the
transposed [128, 32] slabs, at block-table-named places), no MFMA work, no transcendentals (the caller
supplies the cos / sin table), and it sits between two GEMM-sized neighbours.
An eighth is "add_rmsnorm" (LLM_BLOCK), the residual add + RMSNorm in front of a decoder block's projections
(ops.loadgen.add_rmsnorm): a row reduction followed by a second pass over the same row, kept in registers --
two bf16 streams in, two out, a cross-lane and cross-wave sum per row, no MFMA work.
A ninth is "swiglu" (LLM_BLOCK), silu(gate) * up between the fused gate / up projection and the down projection
(ops.loadgen.swiglu): an element-wise stream like the triad, but bf16, pairing column j with column F + j of the
same row, and with a transcendental and an IEEE division -- about 20 VALU operations -- per 6 bytes.
A tenth is "sample" (LLM_HEAD), top-k / top-p token sampling from the LM head's logits (ops.loadgen.sample_tokens):
one very long row per sequence (128,256 bf16 logits = 250 KiB) read once into the registers of one workgroup, an
exact selection of its k largest elements through an LDS histogram of 16-bit order keys, a short sorted softmax
over the survivors and a 4-byte result -- integer compares and LDS atomics, no MFMA work, one exponential per
candidate.
An eleventh is "moe_route" (LLM_MOE), the router of a mixture-of-experts MLP (ops.loadgen.moe_route): a tiny top-k
softmax over E <= 256 logits per token -- one wave per token, integer compares, k exponentials -- and a counting sort
of the T * k (token, choice) slots by expert in ONE workgroup, latency-bound and all but invisible to the CUs.
A twelfth is "moe_gemm" (LLM_MOE), the grouped expert GEMM (ops.loadgen.moe_gemm): MFMA work like "gemm", but over
ragged, data-dependent groups of token rows, one weight matrix per 64-row tile.  At decode batch sizes every expert's
weights are streamed for about 16 rows each, so it is bound by HBM weight traffic, not by the matrix cores; the grid is
sized for the worst routing and the fraction of its workgroups that do work is decided on the device by the router.
A thirteenth is "moe_combine" (LLM_MOE), the weighted scatter-back of the experts' outputs to token order
(ops.loadgen.moe_combine): k indexed 16-byte-chunked row reads and k fused multiply-adds per output chunk -- a gather
like the embedding bag's, but weighted, over rows the same step just wrote, no MFMA work.
A fourteenth is "quant_mx" (LLM_MX), the quantiser of bf16 activations to block-scaled MX operands
(ops.loadgen.quantize_mx): a stream like the SwiGLU's, 2 bytes in and 1 or 1/2 and a scale byte per 32 out, with a
four-lane exponent maximum per block and integer / power-of-two arithmetic only, no MFMA work.
A fifteenth is "gemm_mx" (LLM_MX), fp8 or fp4 activations on MXFP4 weights with one scale per 32 elements
(ops.loadgen.gemm_mx): MFMA work at two or four times the bf16 rate on a quarter of the weight bytes -- at decode
sizes bound by weight streaming like "moe_gemm", at prefill sizes by the matrix cores.
A sixteenth to eighteenth are "rope_append_kv8", "attn_kv8" and "attn_split_kv8" (LLM_KV8): the append and the two decode
attentions over an FP8 (OCP e4m3fn) paged cache with one fp32 scale per KV head (ops.loadgen.rope_append and
paged_decode_attention_kv8) -- the attentions stream HALF the cache bytes of "attn" / "attn_split"
for the same flops, at the cost of a byte -> bf16 conversion in front of every MFMA operand, and hold twice the
sequences per GiB; the append rounds every K and V element with an IEEE division and a few integer operations.
A nineteenth is "prefill_kv8" (LLM_KV8_PREFILL), chunked-prefill attention over that FP8 cache
(ops.loadgen.paged_prefill_attention_kv8): "prefill"'s MFMA work behind a byte -> bf16 conversion of every K and V
fragment, over half the cache bytes -- the conversion sits beside the MFMAs that bound the kernel, not behind HBM.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple


ATTN_HEAD_DIM = 128               # the attention kernels' head dim ...
ATTN_BLOCK_TOKENS = 32            # ... and KV-cache block size (native/hip/decode_attn.hip, prefill_attn.hip)
ATTN_MAX_KV_SPLITS = 32           # the split-KV decode attention: most workgroups per (sequence, KV head) ...
ATTN_PARTIAL_FLOATS = 132         # ... and fp32 per (sequence, head, split) in its workspace: O, m, l, 2 unused
MOE_BLOCK_M = 64                  # rows of a tile of the MoE kernels' sorted layout (native/hip/moe_gemm.hip) ...
MOE_MAX_EXPERTS = 256             # ... the most experts ...
MOE_MAX_TOP_K = 8                 # ... the most choices per token ...
MOE_MAX_SLOTS = 32768             # ... and the most (token, choice) slots T * k of one routing (native/hip/moe_route.hip)


MX_BLOCK = 32                     # elements of a row that share one scale byte of an MX operand (native/hip/quant_mx.hip)
_MX_ELEMENT_BYTES = {"fp8": 1.0, "fp4": 0.5}


def moe_max_tiles(T: int, k: int, E: int) -> int:
    """The 64-row tiles the sorted MoE layout can need for T tokens, top-k k and E experts: the least upper bound on
    sum_e ceil(c_e / 64) over all expert counts c_e >= 0 with sum c_e = T * k -- every slot its own tile, or every
    expert with 63 rows of padding: min(T k, (T k + 63 E) // 64).  The layout's arrays and the grouped GEMM's grid
    are sized by it on the host -- a pure-Python copy of moe_max_tiles (native/hip/moe_route.hip), pinned against it
    in tests/test_moe_cpu.py."""
    n = T * k
    return min(n, (n + (MOE_BLOCK_M - 1) * E) // MOE_BLOCK_M)


@dataclass(frozen=True)
class Op:
    kind: str              # "gemm" (bf16) | "gemm8" (fp8 e4m3, bf16 out) | "triad" | "gather" (bf16 embedding bag)
    #                        | "attn" (bf16 paged-KV decode attention, head dim 128, blocks of 32 tokens)
    #                        | "prefill" (bf16 paged-KV chunked-prefill attention over the same cache)
    #                        | "attn_split" ("attn" as a split-KV launch pair: `splits` workgroups per (sequence, KV head))
    #                        | "rope_append" (bf16 RoPE of q and K and the append of the new K / V to the same cache)
    #                        | "add_rmsnorm" (bf16 residual add + RMSNorm of M rows of N elements, always with a residual)
    #                        | "swiglu" (bf16 silu(gate) * up: M rows of 2 N in, M rows of N out)
    #                        | "sample" (top-k / top-p token sampling: M rows of N bf16 logits in, M int32 tokens out)
    #                        | "moe_route" (MoE routing: top-k softmax of M tokens' N expert logits, the sorted tile layout)
    #                        | "moe_gemm" (bf16 grouped expert GEMM: the M * q routed rows times [N, K] weights of `rows` experts)
    #                        | "moe_combine" (bf16 weighted sum of each token's K expert output rows of N elements)
    #                        | "rope_append_kv8", "attn_kv8", "attn_split_kv8" ("rope_append", "attn", "attn_split" over an FP8
    #                          e4m3fn cache with one fp32 scale per KV head; the fields of their bf16 kinds)
    #                        | "prefill_kv8" ("prefill" over such a cache; the fields of "prefill")
    #                        | "quant_mx" (bf16 -> MX blocks of format `fmt`: M rows of N elements)
    #                        | "gemm_mx" (MX GEMM, bf16 out: activations of format `fmt` on fp4 weights)
    M: int = 0             # gather: bags; attn, attn_split, prefill, rope_append: sequences; add_rmsnorm, swiglu, sample: rows;
    #                        moe_route, moe_gemm, moe_combine: T, the tokens
    N: int = 0             # gather: D, the row length; attn, attn_split, prefill, rope_append: query heads;
    #                        add_rmsnorm: D, the row length; swiglu: F, the output row length; sample: V, the vocabulary;
    #                        moe_route: E, the experts; moe_gemm: the output width; moe_combine: D, the row length
    K: int = 0             # gather: pooling factor (rows per bag); attn, attn_split, prefill, rope_append: context tokens
    #                        per sequence (rope_append: the chunk included); sample: the top-k (1 .. 64);
    #                        moe_route, moe_combine: k, the top-k (1 .. 8); moe_gemm: the reduction length
    relu: bool = True
    n_floats: int = 0      # triad
    rows: int = 0          # gather: rows of the table; attn, attn_split, prefill, rope_append: KV heads;
    #                        moe_gemm, moe_combine: E, the experts
    q: int = 0             # prefill, rope_append: chunk tokens per sequence (the last q of the K context tokens; 1: decode);
    #                        moe_gemm: k, the top-k
    splits: int = 0        # attn_split: kv_splits, workgroups per (sequence, KV head)
    gather: bool = False   # moe_gemm: A is the [T, K] token rows read through the permutation (the first projection);
    #                        False: A is the sorted [P_max, K] intermediate read in place (the down projection)
    fmt: str = ""          # quant_mx: the MX element format written, "fp8" or "fp4"; gemm_mx: the activations' format
    #                        (the weights are always "fp4")

    @property
    def is_gemm(self) -> bool:
        return self.kind in ("gemm", "gemm8")

    @property
    def on_mfma(self) -> bool:
        """MFMA work in the roofline: costed max(flops term, bytes term), its flops on the MFMA side."""
        return self.is_gemm or self.kind in ("prefill", "prefill_kv8", "moe_gemm", "gemm_mx")

    @property
    def flops(self) -> float:
        if self.kind == "gather":
            return 1.0 * self.M * self.K * self.N                 # one add per gathered element
        if self.kind in ("attn", "attn_split", "attn_kv8", "attn_split_kv8"):      # q . K^T and P . V, a multiply-add each
            return 4.0 * self.M * self.N * self.K * ATTN_HEAD_DIM
        if self.kind in ("prefill", "prefill_kv8"):               # the same per (query, token at or below it) pair:
            pairs = self.q * (self.K - self.q) + self.q * (self.q + 1) / 2        # the prefix, then the causal triangle
            return 4.0 * ATTN_HEAD_DIM * self.M * self.N * pairs
        if self.kind in ("rope_append", "rope_append_kv8"):       # two multiplies and one add per rotated element of q and K
            return 3.0 * ATTN_HEAD_DIM * (self.N + self.rows) * self.M * self.q
        if self.kind == "add_rmsnorm":                            # the add, the square and its sum, the two multiplies
            return 5.0 * self.M * self.N
        if self.kind == "swiglu":                                 # two multiplies, the exp as one, an add, a division, a multiply
            return 6.0 * self.M * self.N
        if self.kind == "sample":                                 # the maximum's compare and the selection's compare per logit
            return 2.0 * self.M * self.N
        if self.kind == "moe_route":                              # a compare per logit in each of the k selection rounds
            return 1.0 * self.M * self.N * self.K
        if self.kind == "moe_gemm":                               # the T * k useful rows (pad rows and unused tiles are not work)
            return 2.0 * self.M * self.q * self.N * self.K
        if self.kind == "moe_combine":                            # a multiply-add per (token, choice, element)
            return 2.0 * self.M * self.K * self.N
        if self.kind == "quant_mx":                               # per element: the exponent compare of the block maximum, the
            return 5.0 * self.M * self.N                          # scaling multiply, the rounding add and subtract, the clamp
        if self.kind == "gemm_mx":
            return 2.0 * self.M * self.N * self.K
        return 2.0 * self.M * self.N * self.K if self.is_gemm else 2.0 * self.n_floats

    @property
    def bytes(self) -> float:
        if self.kind == "gemm":
            return 2.0 * (self.M * self.K + self.N * self.K + self.M * self.N)
        if self.kind == "gemm8":
            return 1.0 * (self.M * self.K + self.N * self.K) + 2.0 * self.M * self.N
        if self.kind == "gather":                                 # rows read, indices, offsets, output
            return 2.0 * self.M * self.K * self.N + 4.0 * self.M * self.K + 4.0 * (self.M + 1) + 2.0 * self.M * self.N
        if self.kind in ("attn", "attn_split", "attn_kv8", "attn_split_kv8"):      # K and V, q and out, block table, ctx_lens
            kv8 = self.kind.endswith("_kv8")                      # 1-byte K / V elements and the two [Hkv] fp32 scale vectors
            b = ((2.0 if kv8 else 4.0) * self.M * self.rows * self.K * ATTN_HEAD_DIM + 4.0 * self.M * self.N * ATTN_HEAD_DIM
                 + 4.0 * self.M * self.K / ATTN_BLOCK_TOKENS + 4.0 * self.M + (8.0 * self.rows if kv8 else 0.0))
            if self.kind.startswith("attn_split"):                # the fp32 workspace, written and read once
                b += 2 * 4.0 * decode_split_workspace_floats(self.M, self.N, self.splits)
            return b
        if self.kind in ("prefill", "prefill_kv8"):               # K and V read once, q and out, table, ctx_lens, q_start
            kv8 = self.kind == "prefill_kv8"                      # 1-byte K / V elements and the two [Hkv] fp32 scale vectors
            return ((2.0 if kv8 else 4.0) * self.M * self.rows * self.K * ATTN_HEAD_DIM
                    + 4.0 * self.M * self.q * self.N * ATTN_HEAD_DIM
                    + 4.0 * self.M * self.K / ATTN_BLOCK_TOKENS + 4.0 * self.M + 4.0 * (self.M + 1)
                    + (8.0 * self.rows if kv8 else 0.0))
        if self.kind in ("rope_append", "rope_append_kv8"):
            kv8 = self.kind == "rope_append_kv8"                  # 1-byte K / V elements and the two [Hkv] fp32 scale vectors
            tokens = self.M * self.q
            # table entries (K - q) // 32 .. (K - 1) // 32 of each sequence
            touched = (self.K - 1) // ATTN_BLOCK_TOKENS - (self.K - self.q) // ATTN_BLOCK_TOKENS + 1 if self.q else 0
            return (2.0 * tokens * (self.N + 2 * self.rows) * ATTN_HEAD_DIM        # qkv read
                    + 2.0 * tokens * self.N * ATTN_HEAD_DIM                        # q_out written
                    + (1.0 if kv8 else 2.0) * tokens * 2 * self.rows * ATTN_HEAD_DIM      # K and V written
                    + 4.0 * ATTN_HEAD_DIM * tokens                                 # one 512-byte cos / sin row per token
                    + 4.0 * self.M + 4.0 * (self.M + 1) + 4.0 * self.M * touched   # ctx_lens, q_start, the touched table entries
                    + (8.0 * self.rows if kv8 else 0.0))
        if self.kind == "add_rmsnorm":                            # x and residual read, residual_out and y written, the weight
            return 8.0 * self.M * self.N + 2.0 * self.N
        if self.kind == "swiglu":                                 # gate and up read, out written
            return 6.0 * self.M * self.N
        if self.kind == "sample":                                 # the logits once, four parameter words and the token per row
            return 2.0 * self.M * self.N + 20.0 * self.M
        if self.kind == "moe_route":                              # the logits; ids written and read, weights and slot_pos
            tiles = moe_max_tiles(self.M, self.K, self.N)         # written; the layout's other three arrays written
            return (2.0 * self.M * self.N + 16.0 * self.M * self.K + 4.0 * MOE_BLOCK_M * tiles + 4.0 * tiles
                    + 4.0 * (self.N + 1))
        if self.kind == "moe_gemm":                               # the weights of the experts that can be hit, once; the
            slots = self.M * self.q                               # T * k useful rows of A and of out
            return 2.0 * min(self.rows, slots) * self.N * self.K + 2.0 * slots * self.K + 2.0 * slots * self.N
        if self.kind == "moe_combine":                            # k rows of y per token, out, slot_pos and the weights
            return 2.0 * self.M * self.K * self.N + 2.0 * self.M * self.N + 8.0 * self.M * self.K
        if self.kind == "quant_mx":                               # bf16 in, elements and one scale byte per 32 out
            return (2.0 + _MX_ELEMENT_BYTES[self.fmt] + 1.0 / MX_BLOCK) * self.M * self.N
        if self.kind == "gemm_mx":                                # elements and scales of both operands, bf16 out
            return ((_MX_ELEMENT_BYTES[self.fmt] + 1.0 / MX_BLOCK) * self.M * self.K
                    + (_MX_ELEMENT_BYTES["fp4"] + 1.0 / MX_BLOCK) * self.N * self.K + 2.0 * self.M * self.N)
        return 12.0 * self.n_floats

    def mfma_rate(self) -> float:
        """MFMA throughput relative to bf16 (the fp8 MFMA does twice the work per clock, the fp4 one four times; fp8
        activations on fp4 weights are costed at the wider operand's rate: the mixed rate has not been measured
        apart from the GEMM's, profiles/r16_mx/README.md)."""
        if self.kind == "gemm_mx":
            return 4.0 if self.fmt == "fp4" else 2.0
        return 2.0 if self.kind == "gemm8" else 1.0

    def workgroups(self, cu_budget: int) -> Optional[int]:
        """Workgroups of the op's launch under the default kernel policy (GEMM tiles picked for
        `cu_budget` CUs, 0 = the whole chip); None: the stream kernel's grid (one 1024-thread workgroup per 2048 float4, at most
        8192: 2048 to 8192 for the catalog's arrays) fills any chip."""
        if self.is_gemm:
            return default_gemm_workgroups(self.M, self.N, self.K, cu_budget, self.kind == "gemm8")
        if self.kind == "gather":
            return default_gather_workgroups(self.M)
        if self.kind in ("attn", "attn_kv8"):
            return default_attn_workgroups(self.M, self.rows)
        if self.kind in ("prefill", "prefill_kv8"):
            return default_prefill_workgroups(self.M, self.N, self.rows, self.q)
        if self.kind in ("attn_split", "attn_split_kv8"):
            return default_attn_split_workgroups(self.M, self.rows, self.splits)
        if self.kind in ("rope_append", "rope_append_kv8"):
            return default_rope_append_workgroups(self.M, self.rows, self.q)
        if self.kind == "add_rmsnorm":
            return default_add_rmsnorm_workgroups(self.M)
        if self.kind == "swiglu":
            return default_swiglu_workgroups(self.M, self.N)
        if self.kind == "sample":
            return default_sample_workgroups(self.M)
        if self.kind == "moe_route":
            return default_moe_route_workgroups(self.M)
        if self.kind == "moe_gemm":
            return default_moe_gemm_workgroups(self.M, self.q, self.rows, self.N)
        if self.kind == "moe_combine":
            return default_moe_combine_workgroups(self.M, self.N)
        if self.kind == "quant_mx":
            return default_quantize_mx_workgroups(self.M, self.N)
        if self.kind == "gemm_mx":
            return default_gemm_mx_workgroups(self.M, self.N, self.K, cu_budget)
        return None


@dataclass(frozen=True)
class Workload:
    name: str
    family: str                  # resnet50 | mobilenet | ssd_mobilenet
    framework: str               # onnx | tensorflow
    batch: int
    ops: Tuple[Op, ...]
    hbm_gib: float               # declared footprint (request)

    @property
    def flops(self) -> float:
        return sum(o.flops for o in self.ops)

    @property
    def bytes(self) -> float:
        return sum(o.bytes for o in self.ops)

    @property
    def intensity(self) -> float:
        return self.flops / max(self.bytes, 1.0)


def _mk(framework: str, family: str, batch: int) -> Workload:
    wide = 2048 if framework == "onnx" else 2560
    narrow = 1024 if framework == "onnx" else 1536
    m = batch                                         # 1024 / 2048 / 4096
    if family == "resnet50":
        ops = (Op("gemm", m, wide, wide), Op("gemm", m, wide, wide), Op("gemm", m, wide, wide))
        hbm = 8.0
    elif family == "mobilenet":
        ops = (Op("triad", n_floats=m * 16384), Op("triad", n_floats=m * 16384),
               Op("gemm", m, narrow, narrow))
        hbm = 4.0
    else:  # ssd_mobilenet
        ops = (Op("gemm", m, wide, narrow), Op("triad", n_floats=m * 16384), Op("gemm", m, narrow, wide))
        hbm = 6.0
    return Workload(f"{framework}_{family}_{batch}", family, framework, batch, ops, hbm * (batch / 1024) ** 0.5)


FRAMEWORKS = ("onnx", "tensorflow")
FAMILIES = ("mobilenet", "resnet50", "ssd_mobilenet")
BATCHES = (1024, 2048, 4096)

CATALOG: Dict[str, Workload] = {}
for _fw in FRAMEWORKS:
    for _fa in FAMILIES:
        for _b in BATCHES:
            _w = _mk(_fw, _fa, _b)
            CATALOG[_w.name] = _w
NAMES: List[str] = sorted(CATALOG)
INDEX: Dict[str, int] = {n: i for i, n in enumerate(NAMES)}

# Workloads OUTSIDE the reference's 18 (no configuration / interference rows, no co-run rows
# in data/corun_mi355x.json): kernel mixes the catalog does not have, runnable by the executor
# and the pod entrypoint, and what the co-run model's cold start is checked on
# (models.coldstart, tools/corun_extra_groups.py -> profiles/r05_coldstart/):
#   fp8_llm_2048     three fp8 GEMMs 2048 x 4096 x 4096 (LLM-projection-like, MFMA-bound on
#                    the block-scaled fp8 MFMA the catalog never uses)
#   triad_only_2048  three HBM stream passes, no GEMM at all
#   dlrm_2048        DLRM-like: 26 embedding lookups per sample (2048 x 26 bags of 32 random
#                    256-byte rows from a 1 GiB table -- four times the Infinity Cache, so the rows
#                    come from HBM), then two bf16 GEMMs (the top MLP over the 26 x 128 pooled
#                    features).  The gather is a third kernel character (indexed rows); no co-run
#                    groups are measured with it yet
#   llm_decode_256   one Llama-8B-like decoder layer in the decode phase at batch 256: the fused QKV
#                    projection (256 x 6144 x 4096), decode attention of 32 query heads over 8 KV
#                    heads (groups of 4) with 1,024 tokens of context per sequence, the output
#                    projection (256 x 4096 x 4096).  The paged KV cache is exactly 1 GiB (256 x 32
#                    blocks x 8 heads x 2 x 8 KiB) -- four times the Infinity Cache, like the DLRM
#                    table -- so it streams from HBM, through a shuffled block table.  The attention
#                    is a fourth kernel character; no co-run groups are measured with it yet
EXTRA: Dict[str, Workload] = {
    "fp8_llm_2048": Workload("fp8_llm_2048", "llm_fp8", "hip", 2048, (Op("gemm8", 2048, 4096, 4096),) * 3, 1.0),
    "triad_only_2048": Workload("triad_only_2048", "stream", "hip", 2048,
                                (Op("triad", n_floats=2048 * 16384),) * 3, 1.0),
    "dlrm_2048": Workload("dlrm_2048", "dlrm", "hip", 2048,
                          (Op("gather", 2048 * 26, 128, 32, rows=4 * 1024 * 1024),
                           Op("gemm", 2048, 1024, 3328), Op("gemm", 2048, 1024, 1024)), 1.25),
    "llm_decode_256": Workload("llm_decode_256", "llm_decode", "hip", 256,
                               (Op("gemm", 256, 6144, 4096), Op("attn", 256, 32, 1024, rows=8),
                                Op("gemm", 256, 4096, 4096)), 1.25),
}


# Workloads whose op kind the pinned tables of test_op_kinds_cpu.py do not list yet (they move to
# EXTRA together with those tables):
#   llm_prefill_2048  one Llama-8B-like decoder layer in the prefill phase: two sequences that each
#                     append a 1,024-token chunk to 3,072 cached tokens -- the fused QKV projection
#                     of the 2,048 new tokens (2048 x 6144 x 4096), chunked-prefill attention of 32
#                     query heads over 8 KV heads with 4,096 tokens of context, the output projection
#                     (2048 x 4096 x 4096).  The paged KV cache is 32 MiB and stays in the Infinity
#                     Cache: the attention is MFMA-bound, its 1.2e11 flops level with the two GEMMs'
#                     1.7e11.  The prefill is a fifth kernel character; no co-run groups are
#                     measured with it yet
STAGED: Dict[str, Workload] = {
    "llm_prefill_2048": Workload("llm_prefill_2048", "llm_prefill", "hip", 2048,
                                 (Op("gemm", 2048, 6144, 4096), Op("prefill", 2, 32, 4096, rows=8, q=1024),
                                  Op("gemm", 2048, 4096, 4096)), 0.25),
}


# Workloads of the "attn_split" kind, which those pinned tables do not list either (they merge into
# EXTRA with STAGED, when test_op_kinds_cpu.py's tables are next rewritten):
#   llm_decode_long_8  one Llama-8B-like decoder layer decoding 8 sequences with 32,768 tokens of
#                      context each -- small-batch, long-context serving.  The 8 new tokens ride in
#                      the GEMMs' minimum 64-row tile (rows 8 .. 63 are padding): the fused QKV
#                      projection (64 x 6144 x 4096), split-KV decode attention of 32 query heads
#                      over 8 KV heads, the output projection (64 x 4096 x 4096).  The paged KV cache
#                      is exactly 1 GiB (8 x 1,024 blocks x 8 heads x 2 x 8 KiB), as llm_decode_256's,
#                      and streams from HBM -- but unsplit its grid is 64 workgroups on 256 CUs.
#                      splits = 4 (256 workgroups, one per CU) is the fastest count of the sweep in
#                      profiles/r10_decode_split/rates.json for (8 sequences, 32,768 tokens, groups
#                      of 4): 181 us against 413 us unsplit.  No co-run groups are measured with it yet
LONG_CONTEXT: Dict[str, Workload] = {
    "llm_decode_long_8": Workload("llm_decode_long_8", "llm_decode_long", "hip", 8,
                                  (Op("gemm", 64, 6144, 4096), Op("attn_split", 8, 32, 32768, rows=8, splits=4),
                                   Op("gemm", 64, 4096, 4096)), 1.25),
}


# Workloads of the "rope_append" kind, which those pinned tables do not list either: a decoder layer's
# attention half with the step between the QKV projection and the attention in it -- the fused QKV
# projection, RoPE of q and K and the append of the new K / V to the paged cache, the attention, the
# output projection.  Each op keeps its own operands, as everywhere in the executor: the append writes
# one cache and the attention reads another of the same shape.
#   llm_layer_decode_256    llm_decode_256 with the append of the 256 new tokens (one per sequence, each
#                           into slot 31 of its sequence's last block): 2,048 workgroups that each
#                           rotate five 256-byte rows and scatter 128 2-byte V elements.  Two 1 GiB caches
#   llm_layer_prefill_2048  llm_prefill_2048 with the append of the two 1,024-token chunks: 528 workgroups,
#                           512 of them with a whole (block, KV head) slab of K and V to write.  Two 32 MiB
#                           caches
# The append is a seventh kernel character; no co-run groups are measured with it yet
LLM_LAYER: Dict[str, Workload] = {
    "llm_layer_decode_256": Workload("llm_layer_decode_256", "llm_layer_decode", "hip", 256,
                                     (Op("gemm", 256, 6144, 4096), Op("rope_append", 256, 32, 1024, rows=8, q=1),
                                      Op("attn", 256, 32, 1024, rows=8), Op("gemm", 256, 4096, 4096)), 2.25),
    "llm_layer_prefill_2048": Workload("llm_layer_prefill_2048", "llm_layer_prefill", "hip", 2048,
                                       (Op("gemm", 2048, 6144, 4096), Op("rope_append", 2, 32, 4096, rows=8, q=1024),
                                        Op("prefill", 2, 32, 4096, rows=8, q=1024), Op("gemm", 2048, 4096, 4096)), 0.5),
}


# Workloads of the "add_rmsnorm" and "swiglu" kinds, which those pinned tables do not list either: a WHOLE
# Llama-8B-like decoder block (hidden 4096, 32 query heads over 8 KV heads, MLP width 14336) -- residual add +
# RMSNorm, the fused QKV projection, RoPE + append, the attention, the output projection, residual add + RMSNorm,
# the fused gate / up projection (N = 2 x 14336), SwiGLU, the down projection.  The MLP is the block's dominant
# GEMM work.  No GEMM has a ReLU, as in the model.  Each op keeps its own operands, as everywhere in the executor.
#   llm_block_decode_256    llm_layer_decode_256 with both norms and the MLP: the norms are 256 workgroups
#                           of one 8 KiB row each, the SwiGLU 448 workgroups over 256 x 14336 outputs -- all
#                           three latency-dominated beside GEMMs that stream 48 to 224 MiB of weights.  Two
#                           1 GiB caches and 0.5 GiB of weights and activations
#   llm_block_prefill_2048  llm_layer_prefill_2048 with both norms and the MLP: 2,048 rows, the SwiGLU 3,584
#                           workgroups reading 112 MiB and writing 56 MiB
# The norm and the activation are the eighth and ninth kernel characters; no co-run groups are measured with
# them yet
_BLOCK_D, _BLOCK_F = 4096, 14336


def _llm_block(rows: int, append: Op, attention: Op) -> Tuple[Op, ...]:
    return (Op("add_rmsnorm", rows, _BLOCK_D), Op("gemm", rows, 6144, _BLOCK_D, relu=False), append, attention,
            Op("gemm", rows, _BLOCK_D, 4096, relu=False), Op("add_rmsnorm", rows, _BLOCK_D),
            Op("gemm", rows, 2 * _BLOCK_F, _BLOCK_D, relu=False), Op("swiglu", rows, _BLOCK_F),
            Op("gemm", rows, _BLOCK_D, _BLOCK_F, relu=False))


LLM_BLOCK: Dict[str, Workload] = {
    "llm_block_decode_256": Workload("llm_block_decode_256", "llm_block_decode", "hip", 256,
                                     _llm_block(256, Op("rope_append", 256, 32, 1024, rows=8, q=1),
                                                Op("attn", 256, 32, 1024, rows=8)), 2.5),
    "llm_block_prefill_2048": Workload("llm_block_prefill_2048", "llm_block_prefill", "hip", 2048,
                                       _llm_block(2048, Op("rope_append", 2, 32, 4096, rows=8, q=1024),
                                                  Op("prefill", 2, 32, 4096, rows=8, q=1024)), 1.25),
}


# Workloads of the "sample" kind, which those pinned tables do not list either: the TAIL of a decode step for
# Llama-3's vocabulary of 128,256 tokens -- the final residual add + RMSNorm, the LM-head projection onto the
# vocabulary (no ReLU, 1 GiB of bf16 weights streamed for a few rows: HBM-bound, 501 column tiles of 256 or
# 1,002 of 128), top-k / top-p sampling of the next token from the logits (top_k = 50).  Each op keeps its own
# operands, as everywhere in the executor.
#   llm_head_decode_256  behind llm_block_decode_256: 256 rows, so the sampler is 256 workgroups, one per CU,
#                        reading 64 MB of logits
#   llm_head_decode_8    behind llm_decode_long_8: the 8 new tokens ride in the GEMMs' minimum 64-row tile (the
#                        norm and the projection run 64 rows, 56 of them padding), and the sampler takes the 8
#                        real rows: 8 workgroups on 256 CUs.  That is the case a split-row launch (several
#                        workgroups per row and a merge, like the split-KV attention) would address; it is out
#                        of scope here
# The sampler is a tenth kernel character; no co-run groups are measured with it yet
_HEAD_D, _HEAD_V, _HEAD_TOP_K = 4096, 128256, 50


def _llm_head(rows: int, seqs: int) -> Tuple[Op, ...]:
    return (Op("add_rmsnorm", rows, _HEAD_D), Op("gemm", rows, _HEAD_V, _HEAD_D, relu=False),
            Op("sample", seqs, _HEAD_V, _HEAD_TOP_K))


LLM_HEAD: Dict[str, Workload] = {
    "llm_head_decode_256": Workload("llm_head_decode_256", "llm_head_decode", "hip", 256, _llm_head(256, 256), 1.25),
    "llm_head_decode_8": Workload("llm_head_decode_8", "llm_head_decode_few", "hip", 8, _llm_head(64, 8), 1.0),
}


# Workloads of the "moe_route", "moe_gemm" and "moe_combine" kinds, which those pinned tables do not list either: the
# MLP half of a mixture-of-experts decoder block, Qwen3-30B-A3B-like (hidden 2048, 128 experts, top-8, expert width
# 768) -- residual add + RMSNorm, the router projection (T x 128 x 2048, no ReLU), top-8 routing and the sort into
# 64-row tiles, the experts' fused gate / up projection (to 2 x 768, A gathered through the permutation), SwiGLU over
# the P_max rows of the sorted layout, the experts' down projection (to 2048, read in place), the weighted combine
# back to token order.  1.125 GiB of expert weights.  Each op keeps its own operands, as everywhere in the executor:
# the routing of the GEMMs' and the combine's operands is computed once on the CPU from random logits.
#   llm_moe_decode_256    256 tokens: 2,048 slots over 128 experts, 16 rows per expert on average -- every expert's
#                         weights (1.2 GB) are streamed for a tile that is three quarters padding.  P_max = 10,112 rows
#                         in 158 tiles, of which the routing uses about 128
#   llm_moe_prefill_2048  2,048 tokens: 16,384 slots, 128 rows per expert on average; P_max = 24,448 rows in 382 tiles,
#                         about 320 of them used.  The same weights now meet eight times the rows
# The three are the eleventh to thirteenth kernel characters; no co-run groups are measured with them yet
_MOE_D, _MOE_E, _MOE_TOP_K, _MOE_F = 2048, 128, 8, 768


def _llm_moe(tokens: int) -> Tuple[Op, ...]:
    p_max = MOE_BLOCK_M * moe_max_tiles(tokens, _MOE_TOP_K, _MOE_E)
    return (Op("add_rmsnorm", tokens, _MOE_D), Op("gemm", tokens, _MOE_E, _MOE_D, relu=False),
            Op("moe_route", tokens, _MOE_E, _MOE_TOP_K),
            Op("moe_gemm", tokens, 2 * _MOE_F, _MOE_D, rows=_MOE_E, q=_MOE_TOP_K, gather=True),
            Op("swiglu", p_max, _MOE_F),
            Op("moe_gemm", tokens, _MOE_D, _MOE_F, rows=_MOE_E, q=_MOE_TOP_K),
            Op("moe_combine", tokens, _MOE_D, _MOE_TOP_K, rows=_MOE_E))


LLM_MOE: Dict[str, Workload] = {
    "llm_moe_decode_256": Workload("llm_moe_decode_256", "llm_moe_decode", "hip", 256, _llm_moe(256), 1.5),
    "llm_moe_prefill_2048": Workload("llm_moe_prefill_2048", "llm_moe_prefill", "hip", 2048, _llm_moe(2048), 1.75),
}


# Workloads of the "quant_mx" and "gemm_mx" kinds, which those pinned tables do not list either: the decoder block of
# LLM_BLOCK served QUANTISED -- every projection Op("gemm", r, N, K) of _llm_block becomes Op("quant_mx", r, K, fmt=f),
# the activations' quantisation to MX blocks, followed by Op("gemm_mx", r, N, K, fmt=f) on MXFP4 weights (0.27 of the
# bf16 bytes: 17 instead of 64 bytes per 32 elements).  The projections are, as there, 6144 x 4096 (QKV), 4096 x 4096
# (output), 28672 x 4096 (gate / up) and 4096 x 14336 (down); norms, append, attention and SwiGLU stay bf16.  Each op
# keeps its own operands, as everywhere in the executor.
#   llm_mx_block_decode_256    f = "fp8": 256 rows of fp8 activations on fp4 weights -- the weight-bound case: the
#                              GEMMs stream 12.8 to 59.5 MB of weights (bf16: 48 to 224 MiB) for 256 rows, the
#                              quantisers are 128 or 448 workgroups.  The executor allocates two 1 GiB caches,
#                              0.11 GiB of MX weights and 0.09 GiB of activations: 2.19 GiB, declared 2.25
#   llm_mx_block_prefill_2048  f = "fp4": 2,048 rows, fp4 on fp4 -- the compute-bound case at four times the bf16 MFMA
#                              rate; the quantisers read 16 or 56 MiB.  Two 32 MiB caches, the same weights and
#                              0.68 GiB of activations: 0.85 GiB, declared 1.0
# The quantiser and the MX GEMM are the fourteenth and fifteenth kernel characters; no co-run groups are measured
# with them yet
def _llm_mx_block(rows: int, f: str, append: Op, attention: Op) -> Tuple[Op, ...]:
    ops: List[Op] = []
    for o in _llm_block(rows, append, attention):
        if o.kind == "gemm":
            ops += [Op("quant_mx", o.M, o.K, fmt=f), Op("gemm_mx", o.M, o.N, o.K, relu=False, fmt=f)]
        else:
            ops.append(o)
    return tuple(ops)


LLM_MX: Dict[str, Workload] = {
    "llm_mx_block_decode_256": Workload("llm_mx_block_decode_256", "llm_mx_block_decode", "hip", 256,
                                        _llm_mx_block(256, "fp8", Op("rope_append", 256, 32, 1024, rows=8, q=1),
                                                      Op("attn", 256, 32, 1024, rows=8)), 2.25),
    "llm_mx_block_prefill_2048": Workload("llm_mx_block_prefill_2048", "llm_mx_block_prefill", "hip", 2048,
                                          _llm_mx_block(2048, "fp4", Op("rope_append", 2, 32, 4096, rows=8, q=1024),
                                                        Op("prefill", 2, 32, 4096, rows=8, q=1024)), 1.0),
}


# Workloads of the "rope_append_kv8", "attn_kv8" and "attn_split_kv8" kinds, which those pinned tables do not list either:
# the attention half of a decoder layer served from an FP8 (e4m3fn) paged KV cache with one fp32 scale per KV head.  Each
# op keeps its own operands, as everywhere in the executor: the append writes one cache and the attention reads another.
#   llm_kv8_layer_decode_256  llm_layer_decode_256 with the two kv8 kinds: the append quantises 256 x 8 K rows and V
#                             columns into slot 31 of their blocks, the attention streams 512 MiB instead of 1 GiB.  The
#                             executor allocates two 512 MiB caches (K + V each) and 0.10 GiB of GEMM and qkv operands:
#                             1.10 GiB, declared 1.25
#   llm_kv8_decode_long_8     llm_decode_long_8 with the append of the 8 new tokens in front of the split-KV attention
#                             (splits = 4, as there): 64 x 6144 x 4096, rope_append_kv8, attn_split_kv8, 64 x 4096 x 4096.
#                             Two 512 MiB caches and 0.10 GiB of other operands (the 16 MiB rope table among them):
#                             1.10 GiB, declared 1.25
# They are the sixteenth to eighteenth kernel characters; no co-run groups are measured with them yet
LLM_KV8: Dict[str, Workload] = {
    "llm_kv8_layer_decode_256": Workload("llm_kv8_layer_decode_256", "llm_kv8_layer_decode", "hip", 256,
                                         (Op("gemm", 256, 6144, 4096), Op("rope_append_kv8", 256, 32, 1024, rows=8, q=1),
                                          Op("attn_kv8", 256, 32, 1024, rows=8), Op("gemm", 256, 4096, 4096)), 1.25),
    "llm_kv8_decode_long_8": Workload("llm_kv8_decode_long_8", "llm_kv8_decode_long", "hip", 8,
                                      (Op("gemm", 64, 6144, 4096), Op("rope_append_kv8", 8, 32, 32768, rows=8, q=1),
                                       Op("attn_split_kv8", 8, 32, 32768, rows=8, splits=4),
                                       Op("gemm", 64, 4096, 4096)), 1.25),
}


# Workloads of the "prefill_kv8" kind, which those pinned tables do not list either (a table of its own: LLM_KV8 is
# pinned to its two entries): the prefill side of a stack that keeps its KV cache in FP8.  Each op keeps its own
# operands, as everywhere in the executor: the append writes one cache and the attention reads another.
#   llm_kv8_layer_prefill_2048  llm_layer_prefill_2048 with the two kv8 kinds: two sequences that each append a
#                               1,024-token chunk to 3,072 cached tokens.  Each op's K + V are 16 MiB and stay in the
#                               Infinity Cache: the compute-bound case, where the conversion cost shows undiluted.
#                               The executor allocates 0.252 GiB (0.22 of it the GEMMs' and qkv's), declared 0.5
#   llm_kv8_chunk_prefill_64    continuous batching / long-prefix chunks: 64 sequences that each append a 32-token
#                               chunk to 8,160 cached tokens.  128 columns per (sequence, KV head): one workgroup
#                               each, 512 workgroups.  Each op's K + V are 1 GiB (bf16: 2 GiB) and stream from HBM;
#                               about 256 flops per cache byte (bf16: 128), near the machine balance.  The executor
#                               allocates 2.22 GiB, declared 2.25
# The FP8 prefill is the nineteenth kernel character; no co-run groups are measured with it yet
LLM_KV8_PREFILL: Dict[str, Workload] = {
    "llm_kv8_layer_prefill_2048": Workload("llm_kv8_layer_prefill_2048", "llm_kv8_layer_prefill", "hip", 2048,
                                           (Op("gemm", 2048, 6144, 4096), Op("rope_append_kv8", 2, 32, 4096, rows=8, q=1024),
                                            Op("prefill_kv8", 2, 32, 4096, rows=8, q=1024), Op("gemm", 2048, 4096, 4096)),
                                           0.5),
    "llm_kv8_chunk_prefill_64": Workload("llm_kv8_chunk_prefill_64", "llm_kv8_chunk_prefill", "hip", 64,
                                         (Op("gemm", 2048, 6144, 4096), Op("rope_append_kv8", 64, 32, 8192, rows=8, q=32),
                                          Op("prefill_kv8", 64, 32, 8192, rows=8, q=32), Op("gemm", 2048, 4096, 4096)),
                                         2.25),
}

_TABLES = (CATALOG, EXTRA, STAGED, LONG_CONTEXT, LLM_LAYER, LLM_BLOCK, LLM_HEAD, LLM_MOE, LLM_MX, LLM_KV8, LLM_KV8_PREFILL)


def get(name: str) -> Workload:
    """A catalog, extra, staged, long-context, LLM-layer, LLM-block, LLM-head, LLM-MoE, LLM-MX, LLM-KV8 or
    LLM-KV8-prefill workload by exact name."""
    for table in _TABLES:
        w = table.get(name)
        if w is not None:
            return w
    raise KeyError(name)


def workload_for_pod(pod_name: str) -> Workload:
    """Same matching rule as the recommender: first catalog name that is a substring of
    the pod name with '-' -> '_' (reference recom_server.py:67-71); the extra workloads after
    the catalog, the staged ones after those, then the long-context ones, the LLM-layer ones, the LLM-block
    ones, the LLM-head ones, the LLM-MoE ones, the LLM-MX ones, the LLM-KV8 ones, the LLM-KV8-prefill ones last."""
    nm = pod_name.replace("-", "_")
    for table in _TABLES:
        for n in sorted(table, key=len, reverse=True):
            if n in nm:
                return table[n]
    raise KeyError(pod_name)


def roofline_split(pod_name: str, tflops: float = 1.0e3, tbps: float = 6.0) -> Optional[Tuple[float, float]]:
    """(MFMA-bound s, HBM-bound s) of one iteration of the pod's workload alone on a whole
    GPU (GEMMs at `tflops`, stream passes at `tbps`); None for a pod outside the catalog.
    The GPU plugin's complementarity term reads this (extras "roofline")."""
    try:
        w = workload_for_pod(pod_name)
    except KeyError:
        return None
    m = sum(o.flops / o.mfma_rate() for o in w.ops if o.on_mfma) / (tflops * 1e12)
    h = sum(o.bytes for o in w.ops if not o.on_mfma) / (tbps * 1e12)
    return m, h


# ---------------------------------------------------------------- analytic predictions
CUS = 256                          # MI355X compute units
POD_CU_BUDGET = 64                 # a bench pod's GEMM tile budget (2 CU-slice units x 32 CUs)


# block tile (BM, BN) of the native GEMM kernels: the rows of the kTiles table (native/hip/gemm.hip)
# the default policy can pick
_TILE = {1: (128, 128), 2: (64, 128), 3: (64, 64), 4: (256, 256), 10: (256, 256)}


def default_gemm_workgroups(M: int, N: int, K: int, cu_budget: int = 0, fp8: bool = False) -> int:
    """Workgroups the native GEMM launches for this shape under the DEFAULT kernel policy
    (policy 10, or 1: the same grids -- tile 14 launches tile 10's; no forced tile, split-K off)
    -- a pure-Python copy of pick_gemm_tile /
    resolve_gemm_tile / fp8_tile_128 (native/hip/gemm.hip), so the CU-fill feature needs no
    HIP build and never reads the process-wide tile settings.  Pinned against the
    native picker in tests/test_gemm_policy_picker.py."""
    alone = cu_budget <= 0 or cu_budget >= CUS
    budget = CUS if alone else cu_budget
    if fp8:
        need = 2 * CUS if alone else cu_budget
        big = M % 128 == 0 and N % 128 == 0 and (M // 128) * (N // 128) >= need
        return (M // 128) * (N // 128) if big else (M // 64) * (N // 64)
    per_cu = 2 if alone else 1
    if M % 256 == 0 and N % 256 == 0 and (M // 256) * (N // 256) >= budget:
        t = 10
    elif (M // 128) * (N // 128) >= per_cu * budget:
        t = 1
    elif (M // 64) * (N // 128) >= per_cu * budget and N % 128 == 0:
        t = 2
    else:
        t = 3
    if t == 10 and K < 128:
        t = 4
    bm, bn = _TILE[t]
    if M % bm or N % bn:
        bm, bn = _TILE[3]
    return (M // bm) * (N // bn)


GATHER_BAGS_PER_WORKGROUP = 4      # one wave per bag, 256-thread workgroups (native/hip/gather.hip)


def default_gather_workgroups(B: int, blocks: int = 0) -> int:
    """Workgroups the native embedding-bag launch gets for B bags (blocks > 0 caps the grid) -- a
    pure-Python copy of embedding_bag_workgroups (native/hip/gather.hip), pinned against it in
    tests/test_gather_cpu.py."""
    need = -(-B // GATHER_BAGS_PER_WORKGROUP)
    return blocks if 0 < blocks < need else need


def default_attn_workgroups(S: int, Hkv: int) -> int:
    """Workgroups the native decode-attention launch gets: one per (sequence, KV head) -- a
    pure-Python copy of paged_decode_workgroups (native/hip/decode_attn.hip), pinned against it in
    tests/test_decode_attn_cpu.py."""
    return S * Hkv


def default_attn_split_workgroups(S: int, Hkv: int, kv_splits: int) -> int:
    """Workgroups of the split-KV decode attention's first launch: one per (sequence, KV head, split)
    -- a pure-Python copy of paged_decode_split_workgroups (native/hip/decode_attn.hip), pinned
    against it in tests/test_decode_split_cpu.py.  (The merge launch is ceil(S * Hq / 16).)"""
    return S * Hkv * kv_splits


def decode_split_workspace_floats(S: int, Hq: int, kv_splits: int) -> int:
    """fp32 elements of the split-KV decode attention's workspace: ATTN_PARTIAL_FLOATS per (sequence,
    head, split) -- a pure-Python copy of paged_decode_split_workspace_floats, pinned like the above."""
    return S * Hq * kv_splits * ATTN_PARTIAL_FLOATS


def decode_split_range(ctx: int, kv_splits: int, p: int) -> Tuple[int, int]:
    """The cache blocks [lo, hi) of a sequence of ctx tokens that split p of kv_splits takes -- THE
    partition rule of the split-KV decode attention (native/hip/decode_attn.hip), part of its
    contract: with nblk = ceil(ctx / 32) and bps = ceil(nblk / kv_splits), split p takes
    [p * bps, min(nblk, (p + 1) * bps)) and is empty (lo == hi) where p * bps >= nblk."""
    nblk = -(-ctx // ATTN_BLOCK_TOKENS)
    bps = -(-nblk // kv_splits)
    return min(p * bps, nblk), min((p + 1) * bps, nblk)


PREFILL_COLUMNS = 128              # (chunk token, head of the group) columns per workgroup (native/hip/prefill_attn.hip)


def default_prefill_workgroups(S: int, Hq: int, Hkv: int, max_q_len: int) -> int:
    """Workgroups the native prefill-attention launch gets: one per (sequence, KV head, tile of 128
    columns), a column being a (chunk token, head of the KV head's group) pair and the tiles counted
    for max_q_len tokens -- a pure-Python copy of paged_prefill_workgroups
    (native/hip/prefill_attn.hip), pinned against it in tests/test_prefill_attn_cpu.py."""
    return S * Hkv * -(-max_q_len * (Hq // Hkv) // PREFILL_COLUMNS)


def default_rope_append_workgroups(S: int, Hkv: int, max_q_len: int) -> int:
    """Workgroups the native RoPE + append launch gets: one per (sequence, KV head, cache block a chunk
    of max_q_len tokens can touch -- one that starts in slot 31 touches 1 + ceil((max_q_len - 1) / 32)),
    none where S == 0 or max_q_len == 0 -- a pure-Python copy of rope_append_workgroups
    (native/hip/rope_append.hip), pinned against it in tests/test_gpu_rope_append_exact.py."""
    if S == 0 or max_q_len == 0:
        return 0
    return S * Hkv * ((max_q_len + 30) // ATTN_BLOCK_TOKENS + 1)


def default_add_rmsnorm_workgroups(T: int) -> int:
    """Workgroups the native add + RMSNorm launch gets: one per row -- a pure-Python copy of
    add_rmsnorm_workgroups (native/hip/rmsnorm.hip), pinned against it in tests/test_norm_act_cpu.py."""
    return T


SWIGLU_CHUNKS_PER_WORKGROUP = 1024     # 16-byte output chunks per workgroup: 256 threads x 4 (native/hip/swiglu.hip)


def default_swiglu_workgroups(T: int, F: int) -> int:
    """Workgroups the native SwiGLU launch gets: the work is flattened over (row, 16-byte chunk of 8
    outputs) and a workgroup takes 1,024 consecutive chunks, so ceil(T * F / 8192) -- a pure-Python copy of
    swiglu_workgroups (native/hip/swiglu.hip), pinned against it in tests/test_norm_act_cpu.py."""
    return -(-(T * (F // 8)) // SWIGLU_CHUNKS_PER_WORKGROUP)


def default_sample_workgroups(S: int) -> int:
    """Workgroups the native token-sampling launch gets: one per row of logits -- a pure-Python copy of
    sample_workgroups (native/hip/sample.hip), pinned against it in tests/test_sample_cpu.py."""
    return S


MOE_ROUTE_TOKENS_PER_WORKGROUP = 4     # one wave per token, 256-thread workgroups (native/hip/moe_route.hip)
MOE_COMBINE_CHUNKS_PER_WORKGROUP = 256  # one 16-byte output chunk per thread (native/hip/moe_combine.hip)


def default_moe_route_workgroups(T: int) -> int:
    """Workgroups of the routing's top-k launch: one wave per token, ceil(T / 4) (its second launch, the align
    step, is always ONE workgroup) -- a pure-Python copy of moe_route_workgroups (native/hip/moe_route.hip), pinned
    against it in tests/test_moe_cpu.py."""
    return -(-T // MOE_ROUTE_TOKENS_PER_WORKGROUP)


def default_moe_gemm_workgroups(T: int, k: int, E: int, N: int) -> int:
    """Workgroups the grouped expert GEMM launches: moe_max_tiles(T, k, E) row tiles times N / BN column tiles,
    BN = 128 where N % 128 == 0 and 64 otherwise -- sized for the worst routing; the workgroups of unused tiles
    exit at once -- a pure-Python copy of moe_gemm_workgroups (native/hip/moe_gemm.hip), pinned like the above."""
    return moe_max_tiles(T, k, E) * (N // (128 if N % 128 == 0 else 64))


def default_moe_combine_workgroups(T: int, D: int) -> int:
    """Workgroups of the MoE combine: the work flattened over (token, 16-byte chunk of 8 outputs), 256 chunks per
    workgroup, ceil(T * D / 2048) -- a pure-Python copy of moe_combine_workgroups (native/hip/moe_combine.hip),
    pinned like the above."""
    return -(-(T * (D // 8)) // MOE_COMBINE_CHUNKS_PER_WORKGROUP)


QUANT_MX_CHUNKS_PER_WORKGROUP = 1024    # 16-byte input chunks per workgroup: 256 threads x 4 (native/hip/quant_mx.hip)


def default_quantize_mx_workgroups(T: int, D: int) -> int:
    """Workgroups the native MX quantiser launches: the work flattened over (row, 16-byte chunk of 8 inputs), 1,024
    chunks per workgroup, ceil(T * D / 8192) -- a pure-Python copy of quantize_mx_workgroups (native/hip/quant_mx.hip),
    pinned against it in tests/test_mx_cpu.py."""
    return -(-(T * (D // 8)) // QUANT_MX_CHUNKS_PER_WORKGROUP)


def default_gemm_mx_workgroups(M: int, N: int, K: int, cu_budget: int = 0) -> int:
    """Workgroups the native MX GEMM launches: gemm_fp8's tiles under gemm_fp8's fill rule -- a pure-Python copy of
    gemm_mx_workgroups (native/hip/gemm_mx.hip), pinned against it in tests/test_mx_cpu.py."""
    return default_gemm_workgroups(M, N, K, cu_budget, fp8=True)


def cu_fill(w: Workload, cu_budget: int = POD_CU_BUDGET) -> Optional[float]:
    """Fraction of the chip's CUs the workload's kernels occupy, weighted by their (roofline)
    time: min(1, workgroups / CUs) per kernel -- GEMM workgroups as the native tile picker
    launches them for `cu_budget` under the default policy (default_gemm_workgroups), gather
    workgroups as default_gather_workgroups and attention workgroups as default_attn_workgroups,
    default_attn_split_workgroups, default_prefill_workgroups and default_rope_append_workgroups count
    them, the norm's one workgroup per row (default_add_rmsnorm_workgroups) and the SwiGLU's one per 8,192
    outputs (default_swiglu_workgroups), the sampler's one per row of logits (default_sample_workgroups), the MoE
    kernels' as default_moe_route_workgroups, default_moe_gemm_workgroups and default_moe_combine_workgroups count
    them, the stream kernels' grids fill the chip.  A pod that leaves CUs idle alone leaves
    co-runners room; one that fills the chip alone presses on and suffers from every co-runner
    (models.coldstart)."""
    t = f = 0.0
    for o in w.ops:
        dt = roofline_seconds(Workload(w.name, w.family, w.framework, w.batch, (o,), 0.0), 1.0)
        wg = o.workgroups(cu_budget)
        t += dt
        f += dt * (1.0 if wg is None else min(1.0, wg / CUS))
    return f / t if t > 0 else None


def roofline_seconds(w: Workload, share: float, peak_tflops: float = 1100.0, hbm_tbps: float = 5.5,
                     share_bw_exp: float = 0.6) -> float:
    """Per-iteration time on a `share` of the GPU's XCDs.  Compute scales linearly with
    the share; a CU subset can still pull a super-linear fraction of HBM bandwidth
    (share**share_bw_exp).  Defaults are measured MI355X rates of the native kernels
    (gemm ~1.1 PF on a whole chip, triad ~5.5 TB/s); `profile_workloads` replaces this
    with measurements."""
    t = 0.0
    for o in w.ops:
        if o.on_mfma:
            t += max(o.flops / (peak_tflops * o.mfma_rate() * 1e12 * share),
                     o.bytes / (hbm_tbps * 1e12 * share ** share_bw_exp))
        else:
            t += o.bytes / (hbm_tbps * 1e12 * share ** share_bw_exp)
    return t


def analytic_tables(model: str = "MI355X", parts=(1, 2, 4, 8)) -> Tuple[List[str], List[str], List[List[float]],
                                                                         List[str], List[List[float]]]:
    """(conf_index, conf_cols, conf_values, intf_cols, intf_values) -- configuration
    throughput (iterations/s) per partition share and pairwise interference (throughput
    lost when co-located on the same GPU: HBM contention between memory-heavy kernels),
    in the reference's matrix layout."""
    idx = list(NAMES)
    cols = [f"{p}P_{model}" for p in parts]
    conf = [[1.0 / roofline_seconds(CATALOG[n], 1.0 / p) for p in parts] for n in idx]
    intf_vals = []
    for n in idx:
        a = CATALOG[n]
        base = 1.0 / roofline_seconds(a, 0.25)
        mem_a = min(1.0, 1.0 / max(a.intensity / 100.0, 1e-3))
        row = []
        for m in idx:
            b = CATALOG[m]
            mem_b = min(1.0, 1.0 / max(b.intensity / 100.0, 1e-3))
            row.append(base * 0.25 * mem_a * mem_b)
        intf_vals.append(row)
    return idx, cols, conf, list(idx), intf_vals
