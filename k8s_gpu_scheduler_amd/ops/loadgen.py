"""Torch-facing wrappers for the HIP load kernels (native/hip/gemm.hip and its gemm_*.h kernel
headers, native/hip/triad.hip, native/hip/gather.hip, native/hip/decode_attn.hip,
native/hip/prefill_attn.hip, native/hip/rope_append.hip, native/hip/rmsnorm.hip, native/hip/swiglu.hip,
native/hip/sample.hip, native/hip/moe_route.hip, native/hip/moe_gemm.hip, native/hip/moe_combine.hip,
native/hip/decode_attn_kv8.hip, native/hip/prefill_attn_kv8.hip; rope_append.hip writes FP8 caches as well).

`gemm(a, bt)` computes act(a @ bt.T + bias) in bf16 on MFMA, `gemm_fp8` the same with OCP
e4m3fn operands on the block-scaled fp8 MFMA; `triad(a, b, c, s)` streams HBM;
`embedding_bag(table, idx, offsets)` gathers indexed table rows and sums them per bag (random-row
HBM / cache traffic, no MFMA); `paged_decode_attention(q, k_cache, v_cache, block_table, ctx_lens)`
is LLM decode attention over a paged KV cache (block-table-indexed HBM traffic, MFMA products, a
softmax in the loop; `kv_splits=` spreads a few long sequences over the chip); `paged_prefill_attention(q, k_cache, v_cache, block_table, ctx_lens, q_start)`
is chunked-prefill (append) attention over the same cache: many new tokens per sequence attending
causally (MFMA-bound, the softmax inside the matrix loop); `rope_append(qkv, cos_sin, k_cache, v_cache,
block_table, ctx_lens, q_start)` rotates q and K (RoPE) and appends the new K / V to that cache (small,
latency-dominated, write-scattering); `add_rmsnorm(x, weight, residual)` is the residual add + RMSNorm in
front of a decoder block's projections (a row reduction and a second pass over the same row, two bf16
streams in and two out) and `swiglu(gate_up)` the activation between its fused gate / up and down
projections (an element-wise bf16 stream with an exponential and an IEEE division per element);
`sample_tokens(logits, u, temperature, top_k, top_p)` picks the next token of every sequence from the LM
head's logits (top-k / top-p sampling: one very long row per sequence, an exact selection, a short sorted
softmax, a 4-byte result; the caller supplies the uniforms); `moe_route(logits, top_k)`, `moe_gemm(a, w, sorted_ids,
tile_expert, n_slots, gather_div=)` and `moe_combine(y, slot_pos, topk_w)` are the MLP of a mixture-of-experts block
-- a top-k softmax and a counting sort of the (token, choice) slots by expert into 64-row tiles, a grouped GEMM with
one weight matrix per tile (HBM-bound on the weights at decode sizes) and the weighted sum back to token order --
and `moe_mlp` chains them around `swiglu`; `quantize_mx(x, fmt)` turns bf16 activations into block-scaled MX
operands (a memory-bound stream with a four-lane exponent maximum per block) and `gemm_mx(a_q, a_scales, w_q,
w_scales, a_fmt)` multiplies fp8 or fp4 activations with fp4 weights on the block-scaled MFMA with real block
scales (native/hip/quant_mx.hip, native/hip/gemm_mx.hip).  Shapes are validated on the host before launch (the kernels
have no bounds checks by design).  On a GPU box the native module is mandatory: there is no PyTorch fallback
path here (tests compare against torch fp32 / fp64 references instead).

Operands may be views into larger allocations (row slices, column slices, padded rows).  The
host checks enforce, and tests/test_gpu_kernels_exact.py, test_gpu_gather_exact.py,
test_gpu_decode_attn_exact.py, test_gpu_prefill_attn_exact.py and test_gpu_corun_exact.py (the same inputs beside another stream's
kernels) rely on:

  * A, Bt: K-contiguous rows, the first element 16-byte aligned, the leading dimension (row
    stride in elements) >= K and a multiple of 8 for bf16, of 16 for fp8 -- every row then
    starts on a 16-byte boundary, which the 16-byte global->LDS loads need;
  * C: N-contiguous rows, ldc >= N, rows 8-byte aligned (ldc a multiple of 4, the first
    element 8-byte aligned).  With 16-byte aligned rows (ldc a multiple of 8, the first element
    16-byte aligned) the bf16 kernels take the wide 16-byte-store epilogue, otherwise the 8-byte
    one.  The 4-wave kernels (tiles 14-16) only have the wide epilogue: forced (set_gemm_tile) on
    a C that is not 16-byte aligned they raise, chosen by a policy they give way to the 8-phase /
    128 x 128 kernels;
  * bias: a contiguous fp32 vector of length N, 16-byte aligned;
  * triad: three contiguous fp32 arrays of equal length, a multiple of 4, each 16-byte aligned;
  * embedding_bag: table bf16 R x D and out bf16 B x D with D-contiguous rows, D a power of two
    in [64, 2048], row strides >= D and multiples of 8, the first elements 16-byte aligned (every
    row then is, which the 16-byte row loads and stores need); idx int32 (1-D of length L with
    offsets, or 2-D [B, P] without: fixed pooling) and offsets int32 of length B + 1 (CSR bags:
    non-decreasing, offsets[0] >= 0, offsets[B] <= L), both contiguous, 4-byte aligned.  The
    kernel trusts the indices: check_indices=True verifies the offsets and 0 <= idx[j] < R for the
    j in [offsets[0], offsets[B]) -- the entries the bags name; the others are never read as
    indices -- on the device first (one sync); a caller that passes False guarantees them itself;
  * paged_decode_attention: q and out bf16 [S, Hq, 128] with contiguous [Hq, 128] slabs, a sequence
    stride >= Hq * 128 and a multiple of 8, the first element 16-byte aligned; k_cache bf16
    [NB, Hkv, 32, 128] (a token's row d-contiguous) and v_cache bf16 [NB, Hkv, 128, 32]
    (token-contiguous: the transposed V layout of paged-attention servers), both contiguous and
    16-byte aligned; Hq / Hkv in {1, 2, 4, 8, 16}; block_table int32 [S, max_blocks] with
    contiguous rows a stride >= max_blocks apart, ctx_lens int32 [S] contiguous, both 4-byte
    aligned.  Token t of sequence s is slot t % 32 of block block_table[s, t // 32].  The kernel
    trusts ctx_lens and the block ids: check=True verifies 0 <= ctx <= 32 * max_blocks and
    0 <= id < NB for the ceil(ctx / 32) leading entries of each row -- the ones the sequence names;
    the others are never read as block ids -- on the device first (one sync); a caller that passes
    False guarantees them itself;
  * paged_prefill_attention: the caches, block_table and ctx_lens as for the decode attention; q and
    out bf16 [Tq, Hq, 128], packed over the S sequences, with contiguous [Hq, 128] slabs, a token
    stride >= Hq * 128 and a multiple of 8, the first element 16-byte aligned; q_start int32 [S + 1],
    contiguous, CSR like the gather's offsets: the chunk of sequence s is rows q_start[s] ..
    q_start[s + 1] - 1, q_len[s] of them, non-decreasing with q_start[0] >= 0 and q_start[S] <= Tq.
    ctx_lens[s] counts all tokens of s in the cache, the chunk's own included (a server appends the
    chunk's K / V before it attends); query i of s has position p = ctx_lens[s] - q_len[s] + i and
    attends tokens [0, p], causal with the diagonal included.  q_len[s] <= ctx_lens[s];
    q_len[s] == 0 is legal and writes nothing.  max_q_len bounds every q_len (it sizes the grid;
    the workgroups past a sequence's chunk exit at once).  The kernel trusts all of it: check=True
    verifies ctx_lens and the named block ids as above, q_start, q_len <= ctx_lens and
    q_len <= max_q_len on the device first (one sync, which also computes a max_q_len of None);
    check=False needs max_q_len and never syncs.  With every q_len == 1 this is the decode
    attention;
  * rope_append (native/hip/rope_append.hip), the writer of that cache: the caches, block_table,
    ctx_lens, q_start and max_q_len as for the prefill attention, the group rule Hq / Hkv in
    {1, 2, 4, 8, 16} included; qkv bf16 [Tq, Hq + 2 * Hkv, 128] -- the Hq query heads, then the Hkv K
    heads, then the Hkv V heads: the output of a fused QKV projection -- with contiguous
    [Hq + 2 * Hkv, 128] slabs, a token stride >= that slab and a multiple of 8, the first element
    16-byte aligned; q_out bf16 [Tq, Hq, 128] under the rules of the attentions' out, its storage range
    disjoint from qkv's (q is not rotated in place); cos_sin fp32 [max_pos, 128], contiguous and
    16-byte aligned, row p holding 64 cosines and then 64 sines (rope_table computes them in float64
    on the CPU; the kernel has no transcendentals).  Row q_start[s] + i is token
    p = ctx_lens[s] - q_len[s] + i of s and goes to slot p % 32 of block block_table[s, p // 32]:
    rotated K to k_cache[block, g, slot, :], V to v_cache[block, g, :, slot], rotated q to q_out.
    The kernel trusts all of it: check=True verifies ctx_lens (also against max_pos), q_start,
    q_len <= ctx_lens, q_len <= max_q_len and, of the block table, the entries the chunks touch --
    (ctx - q_len) // 32 .. (ctx - 1) // 32 of each sequence with q_len > 0 -- within [0, NB) and
    pairwise distinct over the launch (two sequences appending into one block is a silent race), on
    the device first (one sync); check=False needs max_q_len and never syncs.  The grid rule --
    S * Hkv * ((max_q_len + 30) // 32 + 1) workgroups, workgroup (s, g, j) taking the chunk's tokens in
    the j-th block the chunk touches, for KV head g -- is part of the contract
    (models.workloads.default_rope_append_workgroups);
  * add_rmsnorm (native/hip/rmsnorm.hip): x, residual, residual_out and out bf16 [T, D], each 2-D with
    contiguous rows, a row stride >= D and a multiple of 8, the first element 16-byte aligned (every
    16-byte chunk of a row then is); D a multiple of 8 in [8, 8192] (a thread keeps at most four chunks
    of its row in registers), T < 2^31; weight bf16 [D], contiguous and 16-byte aligned; eps finite and
    >= 0, rounded to fp32 once on the host.  residual_out needs a residual.  residual_out may be exactly
    residual (same data_ptr, shape and strides: the in-place update of the residual stream; a replayed
    graph is then not idempotent -- every replay adds x again); any other overlap of the storage ranges
    of out with x, weight, residual or residual_out, or of residual_out with x, weight or residual,
    raises.  One workgroup per row (models.workloads.default_add_rmsnorm_workgroups);
  * swiglu (native/hip/swiglu.hip): gate_up bf16 [T, 2F] -- gate columns [0, F), up columns [F, 2F): the
    output of a fused gate / up projection -- and out bf16 [T, F] under the same row rules; F a positive
    multiple of 8, T < 2^31 and T * F / 8 < 2^31 * 1024; out's storage range disjoint from gate_up's.  The
    grid rule -- the work flattened over (row, 16-byte chunk of 8 outputs), a workgroup taking 1,024
    consecutive chunks (8,192 outputs), thread t the chunks t, t + 256, t + 512, t + 768 of them:
    ceil(T * F / 8192) workgroups -- is part of the contract (models.workloads.default_swiglu_workgroups);
  * sample_tokens (native/hip/sample.hip): logits bf16 [S, V], 2-D with contiguous rows, a row stride >= V and
    a multiple of 8, the first element 16-byte aligned; V a multiple of 8 in [8, 131072] (a thread keeps at
    most 16 chunks of its row in registers), S < 2^31; u, temperature and top_p fp32 [S], top_k int32 [S],
    each 1-D and contiguous; out int32 [S], contiguous, its storage range disjoint from every input's.  The
    kernel trusts the parameters, except that it clamps top_k into [1, 64] itself: check=True verifies
    1 <= top_k <= 64, temperature finite and >= 0 and, on the rows that are not greedy (temperature == 0 or
    top_k == 1), 0 < top_p <= 1 and 0 <= u < 1, on the device first (one sync); check=False never syncs.
    One workgroup per row (models.workloads.default_sample_workgroups);
  * the MoE layout (native/hip/moe_route.hip), shared by moe_route, moe_gemm and moe_combine -- the
    moe_align_block_size scheme of paged-attention servers.  T tokens, E experts, top-k k; n = T * k slots, slot
    s = t * k + j being token t's j-th choice; moe_max_tiles(T, k, E) = min(n, (n + 63 E) // 64), the least upper
    bound on sum_e ceil(c_e / 64) over the expert counts c_e; P_max = 64 * moe_max_tiles.  Four int32 arrays:
      - sorted_ids [P_max]: experts in ascending order; expert e owns the rows [off[e], off[e + 1]) with
        off[e + 1] - off[e] = 64 * ceil(c_e / 64); its c_e slots come first, in ascending slot order (stable:
        deterministic, no run-to-run variation); the sentinel n fills the rest of its last tile and every row from
        off[E] to P_max;
      - tile_expert [moe_max_tiles]: the expert of each 64-row tile, -1 for the unused trailing tiles;
      - expert_offsets [E + 1]: off;
      - slot_pos [n]: the row of sorted_ids that holds slot s (the inverse map).
    Every element of all four is written by every moe_route launch: they may hold anything before, and a replay
    gives the same.  moe_align_reference(topk_ids, E) builds them in pure torch on the CPU;
  * moe_route: logits bf16 [T, E], 2-D with contiguous rows, a row stride >= E and a multiple of 8, the first
    element 16-byte aligned; E a multiple of 8 in [8, 256], 1 <= top_k <= min(8, E), T * top_k <= 32768.  topk_ids
    int32 [T, k] and topk_w fp32 [T, k], contiguous; the four layout arrays, 1-D, contiguous, of exactly the sizes
    above; all six made when None, pairwise disjoint and disjoint from logits.  Two launches: one wave per token
    (models.workloads.default_moe_route_workgroups), then ONE workgroup for the layout.  T == 0 reads nothing and
    writes the E + 1 offsets (all 0; moe_max_tiles == 0, so the other arrays are empty);
  * moe_gemm: a bf16 [R, K] and out bf16 [P_max, N] under the row rules of add_rmsnorm's operands (contiguous rows,
    a leading dimension >= the row and a multiple of 8, 16-byte aligned); w bf16 [E, N, K] with K-contiguous rows,
    a row stride >= K and an expert stride that are multiples of 8 (the expert stride is otherwise arbitrary: 0
    shares one matrix among the experts), 16-byte aligned; N and K positive multiples of 64; sorted_ids int32
    [P_max] and tile_expert int32 [P_max / 64], contiguous; out disjoint from every input.  Output row i of a used
    tile is a[src(i)] . w[tile_expert[i // 64]]^T with src(i) = sorted_ids[i] // gather_div for gather_div = k >= 1
    (the first projection: token rows through the permutation) and src(i) = i for gather_div = 0 (the down
    projection: the sorted intermediate in place).  The kernel trusts the layout: check=True verifies tile_expert
    within [-1, E), sorted_ids within [0, n_slots] and every source row of a used tile < R on the device first (one
    sync); check=False never syncs.  The grid -- P_max / 64 row tiles times N / BN column tiles, BN = 128 where
    N % 128 == 0, else 64 (models.workloads.default_moe_gemm_workgroups) -- is fixed on the host;
  * moe_combine: y bf16 [P_max, D] and out bf16 [T, D] under the same row rules, D a positive multiple of 8; topk_w
    fp32 [T, k] and slot_pos int32 [T * k], contiguous, 1 <= k <= 8; out disjoint from every input.  The kernel
    trusts slot_pos (moe_route wrote it): every entry names a row of y.  One thread per 16-byte output chunk
    (models.workloads.default_moe_combine_workgroups);
  * THE MX FORMAT (quantize_mx, gemm_mx and their references; OCP Microscaling v1.0, block size 32 along the row,
    K): a matrix [rows, K] is a pair (elements, scales).
      - Scale: one E8M0 byte per (row, block), value 2^(b - 127); b = 255 is NaN.  uint8 [rows, K / 32], row stride in
        elements.
      - "fp4": e2m1 -- sign, 2 exponent bits, 1 mantissa bit; magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6.  Two per byte,
        element 2i in bits 3:0 of byte i: uint8 [rows, K / 2].  (The nibble order inside a block cannot change a dot
        product of two fp4 operands as long as both use it; it is fixed so that bytes are comparable, and it is the
        order in which the MFMA pairs fp4 elements with the bytes of an fp8 operand.)
      - "fp8": OCP e4m3fn, one per byte: FP8 [rows, K].
    The quantisation rule is integer and power-of-two arithmetic only, so the device and quantize_mx_reference agree
    bit for bit.  Per block: e is the largest biased exponent field (bits >> 7) & 0xFF of the 32 bf16 inputs; emax
    is 2 for fp4 and 8 for fp8.  e == 255 (an Inf or NaN in the block): scale byte 255, all element bytes of the
    block 0x00.  Otherwise the scale byte is b = max(e - emax, 0), never above 253 (an all-zero and a
    subnormal-amax block get b = 0), and an element is v * 2^(127 - b), exact in fp32, rounded to the element format
    to nearest, ties to even, saturated at the largest finite magnitude (6 or 448); the input's sign bit is always
    carried, so -0.0 and a negative value that rounds to zero give 0x8 or 0x80.  The rule is idempotent;
  * quantize_mx (native/hip/quant_mx.hip): x under add_rmsnorm's row rules with D a positive multiple of 32; q and
    scales with contiguous rows and any row stride >= the row, pairwise disjoint and disjoint from x.  The grid rule
    -- the work flattened over (row, 16-byte chunk of 8 inputs), 1,024 chunks per workgroup: ceil(T * D / 8192)
    workgroups -- is part of the contract (models.workloads.default_quantize_mx_workgroups);
  * gemm_mx (native/hip/gemm_mx.hip): M, N multiples of 64, K of 128; element rows 16-byte aligned (row stride a
    multiple of 16 bytes); scale rows any stride >= K / 32; C and bias as the other GEMMs'.  Tiles and fill rule are
    gemm_fp8's (models.workloads.default_gemm_mx_workgroups).  fp32 accumulation inside the scaled MFMA (one
    instruction per 128 k, its internal adder undocumented: tests/test_gpu_gemm_mx_exact.py measures it), K tiles
    summed in order, one rounding to bf16; no split-K, no atomics, launches repeat bit for bit;
  * THE FP8 KV FORMAT (rope_append with float8_e4m3fn caches, paged_decode_attention_kv8 and
    paged_prefill_attention_kv8; stated once in
    native/hip/api.h): k_cache [NB, Hkv, 32, 128] and v_cache [NB, Hkv, 128, 32] as for bf16, one OCP e4m3fn byte
    per element, and k_scale, v_scale fp32 [Hkv], contiguous, on the operands' device; a stored byte c of KV head g
    stands for e4m3fn(c) * scale[g].  Every other operand rule of the ops is unchanged; both caches have one
    dtype; paged_decode_attention and paged_prefill_attention do not read such a cache.  THE QUANTISATION RULE for an fp32 value z: a NaN
    gives 0x7F | sign << 7; otherwise the magnitude is rounded to the nearest e4m3fn value, ties to even (the
    subnormal step is 2^-9 below 2^-6); whatever rounds above 448, +-Inf included, saturates to 0x7E; the sign bit
    is always carried (-0.0 and a negative value that rounds to zero give 0x80).  torch's cast does not saturate
    (500 -> NaN) and agrees only for |z| <= 448: quantize_kv8_reference is the reference.  rope_append stores
    z = y / k_scale[g] for K, y the fp32 rotation result NOT first rounded to bf16, and z = float(v) / v_scale[g]
    for V, both IEEE fp32 divisions; q_out is as for bf16 caches.  The decode kernels convert the bytes to bf16
    in registers (exact for all 254 non-NaN codes; 0x7F and 0xFF are NaN) and keep the bf16 contract below with
    scores = mfma_sum * (scale * k_scale[g]), the two scalars multiplied once in fp32, and
    out = bf16((acc / lsum) * v_scale[g]); the split kernel's partials are unscaled by v_scale, the merge applies
    it.  check=True also verifies that the scales are finite and > 0 (pinned by tests/test_gpu_rope_append_kv8_exact.py,
    test_gpu_decode_kv8_exact.py and test_gpu_kv8_chain.py).

Nothing outside the M x K, N x K and M x N windows (or the n floats of the triad) is read or
written; the gather reads only the D elements of the rows the bags name (and the idx entries
[offsets[0], offsets[B]) and the offsets) and writes only the B x D window.  The decode attention
reads q's S x Hq x 128 window, ctx_lens, the named table entries and the (block, KV head) slabs they
name -- whole slabs, but the slots of a sequence's last block past ctx may hold anything (NaN
included) without touching the output: their scores are replaced by -inf and their V elements by
zero -- and writes only out's S x Hq x 128 window.  The prefill attention reads the q rows
[q_start[s], q_start[s + 1]) of each sequence, ctx_lens, q_start, the ceil(ctx / 32) leading table
entries of each sequence and the (block, KV head) slabs they name, and writes only the out rows
[q_start[0], q_start[S]).  The slots of a sequence's last block past ctx may again hold anything:
they lie above every position, so their scores are replaced by -inf with a select, and their V
elements by zero.  A non-finite K or V value of a token inside ctx follows the NaN rule below for
that sequence's queries at or after the token; it leaves the outputs of earlier queries of the same
sequence unspecified (the token's probability is 0 there, but 0 * NaN in the V fragment the columns
share cannot be kept out per column); it never reaches another sequence or KV head.  rope_append
reads the qkv rows [q_start[0], q_start[S]), ctx_lens, q_start, the cos_sin rows of the chunks'
positions and the touched table entries; it writes the same rows of q_out and, per chunk token and KV
head, the 128 K elements of the token's slot and its 128 V elements -- every other byte of the caches,
the earlier slots of the chunk's first block and the slots past ctx of its last included, is
bit-preserved, and the caches are never read.  q_len == 0 and ctx == 0 write nothing; replaying the
launch is idempotent.  add_rmsnorm reads the T x D windows of x and residual and the D elements of
weight and writes the T x D windows of out and residual_out; swiglu reads the T x 2F window of gate_up and
writes the T x F window of out.  sample_tokens reads the S x V window of logits and the S elements of u,
temperature, top_k and top_p and writes the S elements of out.  moe_route reads the T x E window of logits and writes
every element of its six outputs.  moe_gemm reads sorted_ids and tile_expert, the K elements of the rows of a that the
valid rows of used tiles name -- never a pad row's own, and nothing for an unused tile -- and the N x K windows of the
experts that own a used tile; it writes the N columns of every row of a used tile (a pad row, sorted_ids[i] >= n_slots,
as +0.0, 0x0000) and leaves the rows of unused tiles bit-preserved.  moe_combine reads slot_pos, topk_w and the D
elements of the T * k rows of y that slot_pos names and writes the T x D window of out.  The padding between the rows of a strided
operand is neither read nor written.

Numeric contract (pinned bitwise by tests/test_gpu_numeric_edges.py against an integer definition
of the conversion and float64 sums):

  * every bf16 output is the round-to-nearest-even encoding of its fp32 value over the whole fp32
    range: ties go to the even neighbour, a rounding may carry into the exponent, values past the
    largest finite bf16 (from 0x7F7F8000 on) become +-Inf;
  * subnormals are kept, in the fp32 arithmetic (bias add, gather and triad sums, MFMA
    accumulators) and in the conversion: an fp32 subnormal rounds to a bf16 subnormal or to +-0,
    nothing is flushed;
  * a NaN in gives a NaN out in every cell that depends on it and in no other (Inf * 0 and
    Inf - Inf are NaN too: no zero is skipped); which NaN -- sign and payload -- is unspecified, also
    for NaNs whose payload lies only in the 16 bits the conversion drops.  An fp32 accumulator that
    overflows gives +-Inf;
  * ReLU is `v > 0 ? v : 0` in every epilogue: NaN and every negative value, -0.0 and -Inf
    included, give +0.0 -- unlike torch.relu, which passes NaN on;
  * without ReLU, -0.0 survives only where nothing is added to it: the GEMM epilogues compute
    acc + bias with acc = +0.0 for all-zero operands, so a bias of -0.0 gives +0.0; the gather
    starts every bag at +0.0, so an empty bag and a bag of a single -0.0 row give +0.0 (bit
    pattern 0x0000); the triad's -0.0 + s * -0.0 is -0.0 for s > 0;
  * paged_decode_attention (pinned by tests/test_gpu_decode_attn_exact.py): q . k accumulates in
    fp32 on the MFMA and scale multiplies the fp32 score (it is not folded into a bf16 q); the
    softmax is the online one (running maximum) in fp32 with exp(x) = 2^(x * log2 e), so a
    probability whose exponent is below fp32's range is exactly 0 and exp(0) exactly 1; the
    normaliser is summed from the fp32 probabilities; the probabilities are rounded to bf16 for
    the P . V MFMA (at most 2^-9 relative each), which accumulates in fp32; the partial results
    of the four waves are merged in fp32, divided by the normaliser (an IEEE division) and rounded
    to bf16 once.  ctx == 0 gives a row of +0.0.  A non-finite q, K or V value inside ctx follows the
    NaN rule for the heads of its (sequence, KV head) and never leaves them: a NaN or +Inf score
    (Inf - Inf) makes the head's whole row NaN -- the normaliser is NaN, and the division is not
    guarded against it --, a -Inf score is probability 0, and a non-finite V element poisons only
    its own d (0 * Inf and 0 * NaN are NaN: no probability-0 token is skipped).  Left unspecified:
    the row of a head whose -Inf score belongs to the only token inside ctx of the only block its
    wave takes (the last token of a context of 33, 65 or 97 tokens) -- that wave's running maximum
    is then -Inf itself;
  * paged_decode_attention with kv_splits >= 2 (pinned by tests/test_gpu_decode_split_exact.py): the
    split rule -- with nblk = ceil(ctx / 32) and bps = ceil(nblk / kv_splits), workgroup p of a
    (sequence, KV head) takes the blocks [p * bps, min(nblk, (p + 1) * bps)), none where
    p * bps >= nblk (decode_split_range) -- and the workspace rule -- 132 fp32 per (sequence, head,
    split): the unnormalised O, the maximum and the normaliser of the split, two unused words;
    decode_split_workspace_floats(S, Hq, kv_splits) in all, 16-byte aligned, one launch in flight
    per workspace; every word the merge reads was written by the same launch, so the workspace
    may hold anything before, NaN included -- are part of the contract.  The numeric contract of
    the unsplit op carries over with one more fp32 merge level: inside a split everything is as
    above up to the merge of the four waves, which is left undivided; the splits are merged by the
    same formula (weight exp(m_p - max m), exactly 0 for an empty split), then the same single
    IEEE division and the same single bf16 rounding.  ctx == 0 gives a row of +0.0, and the NaN
    rule is the one above;
  * paged_prefill_attention (pinned by tests/test_gpu_prefill_attn_exact.py): the same contract, so
    the decode attention's error derivation carries over -- fp32 q . k on the MFMA, scale on the
    fp32 score, the online softmax in fp32 with exp(x) = 2^(x * log2 e), the normaliser summed from
    the fp32 probabilities, the probabilities rounded to bf16 only as the P . V operand, O in fp32,
    one IEEE division by the normaliser and one bf16 rounding.  A column's running state lives in
    one wave for the whole walk: there is no merge of partial results;
  * both attentions (pinned by tests/test_gpu_attn_numeric_edges.py on every finite bf16 code as a
    V element, on rounding ties, exponent carries, subnormal and overflowing sums of two V
    elements, on NaN / +-Inf planted in q, K and V, and at scale 0, the negated and two other
    scales): bf16 subnormals pass through the P . V MFMA, the division and the rounding
    unchanged, 0x7F7F stays finite, an fp32 sum past the range gives +-Inf.  The sign of a zero
    output is unspecified except for ctx == 0: an accumulator that a rescale by alpha = 0 zeroed
    keeps the sign of what it held, so V = -0.0 with probability 1, or v + (-v), may give +0.0 or
    -0.0; a nonzero value that only rounds to zero keeps its own sign;
  * rope_append (pinned by tests/test_gpu_rope_append_exact.py): rotate-half pairing (Llama / NeoX) on
    every q head and every K head -- for i in [0, 64), with x1 = x[i], x2 = x[i + 64],
    c = cos_sin[p, i] and s = cos_sin[p, 64 + i], all in fp32: y[i] = fma(x1, c, -(x2 * s)) and
    y[i + 64] = fma(x2, c, x1 * s), the product rounded to fp32, the fma fused, whatever the compiler's
    contraction setting, then one rounding to bf16 (nearest even, subnormals kept).  A NaN or Inf in
    x1, x2, c or s reaches both outputs of its pair wherever IEEE says so (0 * NaN and 0 * Inf are NaN:
    no zero is skipped) and no other element.  V is copied bit for bit, NaN payloads and -0.0
    included;
  * add_rmsnorm (pinned by tests/test_gpu_rmsnorm_exact.py): h = fp32(x) + fp32(residual) is one fp32 add
    and residual_out = bf16(h), round to nearest even.  hb = fp32(residual_out) is the ROUNDED stream and
    the norm is computed from it, so add_rmsnorm(x, w, residual) gives bit for bit the y of
    add_rmsnorm(residual_out, w) without a residual; without a residual hb = fp32(x) and no
    residual_out is written.  ss = sum of hb^2 is accumulated in fp32 with fma: per-thread partials, a
    wave butterfly, then the four wave partials summed in one fixed order by every thread -- all threads
    of a row hold the same ss; the order is otherwise unspecified; there are no atomics, so two launches
    on the same inputs are bit-identical.  r = 1.0f / sqrtf(ss / float(D) + eps): an IEEE division, an
    fp32 add, a correctly rounded square root and an IEEE division (no rsqrt, no fast-math).
    y = bf16((hb * r) * fp32(w)): two fp32 multiplies in that order and one rounding.  Non-finite values
    and zeros are not special-cased: a NaN in a row makes that row's y all NaN and, in residual_out, only
    its own element; an all-zero row with eps > 0 gives zeros with the sign of hb * w, with eps == 0
    NaN (0 * Inf); no other row is ever affected;
  * swiglu (pinned by tests/test_gpu_swiglu_exact.py): in fp32, e = exp2(-g * log2 e) -- the product
    rounded to fp32, the hardware exponential (v_exp_f32) -- s = g / (1.0f + e), an IEEE division, and
    out = bf16(s * u), one rounding.  So g = +-0 gives e == 1 and s = +-0; g >= 128 gives e == 0 exactly,
    s == g and out = bf16(g * u), an exact fp32 product; g <= -128 gives e == +Inf and s = -0.0;
    g = -Inf gives NaN, as torch.nn.functional.silu does; g = +Inf gives +-Inf * u.  A NaN or Inf in g or
    u reaches its own output element and no other;
  * sample_tokens (pinned by tests/test_gpu_sample_exact.py).  Row-level rules:
      - Comparisons are on values: +0.0 == -0.0.
      - A row that holds any NaN, or whose maximum is -Inf, gives token -1.  No other row is affected.
      - A row whose maximum is +Inf gives the lowest index holding +Inf, in either mode.
      - Greedy (temperature == 0 or top_k == 1): the token is the lowest index of the row maximum.  No
        exponential is computed.  u and top_p are not read as numbers and may be NaN.
    Candidates:
      - k = min(clamp(top_k, 1, 64), V).
      - The candidates are the k largest logits.  Ties at the threshold value go to the lowest indices.
      - They are ranked c_0 .. c_{k-1} by (value descending, index ascending).
      - The kernel itself clamps top_k into [1, 64].  This is one v_med3, and an out-of-range value must not
        be able to run past the LDS candidate array.
    Weights:
      - c = 1.44269504f / temperature is an IEEE division.
      - a_j = (l_{c_j} - l_{c_0}) * c is one fp32 subtraction and one fp32 multiply.
      - w_j is the hardware exp2 (v_exp_f32) of a_j, as in swiglu.hip and the attentions.
      - Consequences: w_0 == 1 exactly; equal logits give exactly 1; a_j <= -150 (and -Inf) gives exactly 0.
    Cumulative sum:
      - cum_j is the inclusive fp32 prefix sum of w in rank order.
      - The association is unspecified but fixed (a wave scan).
      - There are no float atomics, so two launches on the same inputs give identical tokens.
      - Z = cum_{k-1}.
    Top-p:
      - n is the smallest n >= 1 with cum_{n-1} >= top_p * Z (one fp32 multiply).
      - top_p == 1 keeps all k.
    Pick:
      - target = u * cum_{n-1}.
      - The token is c_j for the smallest j < n with cum_j > target.
      - If no such j exists, the token is c_{n-1}.
    Memory:
      - Nothing outside the S x V window and the five [S] vectors is read.
      - Only out[0..S) is written.
  * moe_route (pinned by tests/test_gpu_moe_route_exact.py).  Selection: the k largest logits of a token ranked by
    (value descending, index ascending); comparisons are on values (+0.0 == -0.0) and ties go to the lowest index, so
    topk_ids is exact for any finite or +-Inf input.  Weights, in fp32: e_j = exp2((l_j - l_0) * 1.44269504f) -- one
    subtraction, one multiply, the hardware v_exp_f32 --, their sum over j = 0 .. k - 1 in that order, and
    topk_w[t, j] = e_j / sum, an IEEE division: softmax-then-renormalise over the k selected logits.  Equal logits
    give exactly 1 / k for k a power of two; k = 1 gives exactly 1.0.  A row that holds a NaN, or whose maximum is
    -Inf, has unspecified weights; its ids are still k distinct values in [0, E), and nothing downstream can index
    out of range because of data.  The layout has no float in it, integer atomics only count, and the order inside
    an expert is the stable one: two launches are bit-identical;
  * moe_gemm (pinned by tests/test_gpu_moe_gemm_exact.py): no bias, no activation; out = bf16(acc), one rounding to
    nearest even of an fp32 MFMA accumulation (v_mfma_f32_16x16x32_bf16) whose K order is fixed -- no split-K, no
    atomics, so launches repeat bit for bit -- and the same for every row of a tile: a row's result does not depend
    on where in a tile it sits.  The NaN rule is the GEMMs';
  * moe_combine (pinned by tests/test_gpu_moe_combine_exact.py): acc = 0.0f, then for j = 0 .. k - 1 in that order
    acc = fmaf(topk_w[t, j], fp32(y[slot_pos[t k + j], c]), acc), fused whatever the contraction setting, and one
    rounding to bf16.  Nothing is skipped (0 * NaN is NaN): a NaN reaches its own (t, column) and no other.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import _native
from ..models.workloads import ATTN_BLOCK_TOKENS, ATTN_HEAD_DIM          # the decode-attention kernel's fixed sizes
from ..models.workloads import (ATTN_MAX_KV_SPLITS, decode_split_range,      # the split-KV decode's rules, pure Python
                                decode_split_workspace_floats)
from ..models.workloads import (MOE_BLOCK_M, MOE_MAX_EXPERTS, MOE_MAX_SLOTS, MOE_MAX_TOP_K,      # the MoE layout's sizes
                                moe_max_tiles)

BM, BN, BK = 64, 64, 64          # minimum granularity; the tile (128x128 / 64x128 / 64x64) is picked per shape


def _stream_ptr(stream: Optional[torch.cuda.Stream], device: Optional[torch.device] = None) -> int:
    s = stream if stream is not None else torch.cuda.current_stream(device)
    if device is not None and s.device != device:
        raise ValueError(f"stream is on {s.device}, operands on {device}")
    return int(s.cuda_stream)


def _check_devices(name: str, *ts: Optional[torch.Tensor]) -> torch.device:
    """Every operand (and output/bias when given) must be a device tensor on ONE GPU: a host
    pointer handed to the kernel is a GPU memory fault (XNACK off), another GPU's pointer
    a launch on the wrong device."""
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise ValueError(f"{name} expects device tensors (got a {t.device} tensor)")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError(f"{name}: operands on different devices ({dev} vs {t.device})")
    return dev


def _launch_stream(stream: Optional[torch.cuda.Stream], device: torch.device):
    """The launch stream (the caller's, or the device's current one) as a context: torch work
    inside it -- an allocation, a check -- is ordered with the kernel."""
    return torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(device))


def _row_stride(t: torch.Tensor, rows: int, default: int) -> int:
    """The stride of dim 0 in elements; of a single row torch may report anything: the default."""
    return t.stride(0) if rows > 1 else default


def check_gemm_shapes(M: int, N: int, K: int, bk: int = BK, name: str = "gemm") -> None:
    if M <= 0 or N <= 0 or K <= 0 or M % BM or N % BN or K % bk:
        raise ValueError(f"{name} shape ({M},{N},{K}) must be positive multiples of ({BM},{BN},{bk})")


FP8 = torch.float8_e4m3fn          # OCP e4m3 (gfx950), not the MI300 "fnuz" encoding
_OPERAND_NAMES = {torch.bfloat16: "bf16", FP8: "float8_e4m3fn"}


def _gemm_operands(name: str, dtype: torch.dtype, bk: int, rows16: bool, a: torch.Tensor, bt: torch.Tensor,
                   out: Optional[torch.Tensor], bias: Optional[torch.Tensor]):
    """The checks `gemm` and `gemm_fp8` share: operands of `dtype` (K a multiple of `bk`, row
    strides multiples of 16 elements with `rows16`), the output (made when None) and the bias.
    Returns (M, N, K, out, the bias pointer or 0)."""
    if a.dtype != dtype or bt.dtype != dtype:
        raise TypeError(f"{name} expects {_OPERAND_NAMES[dtype]} operands")
    _check_devices(name, a, bt, out, bias)
    if a.dim() != 2 or bt.dim() != 2 or a.shape[1] != bt.shape[1]:
        raise ValueError(f"{name} shape mismatch {tuple(a.shape)} x {tuple(bt.shape)}^T")
    if a.stride(1) != 1 or bt.stride(1) != 1 or (rows16 and (a.stride(0) % 16 or bt.stride(0) % 16)):
        raise ValueError(f"{name} expects row-major operands with 16-byte aligned rows" if rows16 else
                         f"{name} expects row-major (K-contiguous) operands")
    M, K = a.shape
    N = bt.shape[0]
    check_gemm_shapes(M, N, K, bk, name)
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=a.device)
    if out.shape != (M, N) or out.dtype != torch.bfloat16 or out.stride(1) != 1:
        raise ValueError("bad output tensor")
    bptr = 0
    if bias is not None:
        if bias.dtype != torch.float32 or bias.numel() != N or not bias.is_contiguous():
            raise ValueError("bias must be a contiguous fp32 vector of length N")
        bptr = bias.data_ptr()
    return M, N, K, out, bptr


def gemm(a: torch.Tensor, bt: torch.Tensor, out: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
         relu: bool = False, stream: Optional[torch.cuda.Stream] = None, cu_budget: int = 0) -> torch.Tensor:
    """out[M,N] = act(a[M,K] @ bt[N,K]^T + bias[N]) -- bf16 in/out, fp32 accumulate.
    cu_budget: CUs this GEMM can expect to own (the pod's share when pods co-run; 0 = the
    whole chip) -- steers the tile choice (native pick_gemm_tile)."""
    M, N, K, out, bptr = _gemm_operands("gemm", torch.bfloat16, BK, False, a, bt, out, bias)
    h = _native.hip()
    with torch.cuda.device(a.device):
        sp = _stream_ptr(stream, a.device)
        # split-K (lone GEMMs whose 256x256 tiles leave CUs idle): an fp32 partial workspace from
        # the caching allocator, allocated on the launch stream so its reuse is ordered after
        # the reduce kernel
        wsf = h.splitk_workspace_floats(M, N, K, cu_budget)
        ws = None
        if wsf:
            with _launch_stream(stream, a.device):
                ws = torch.empty(wsf, dtype=torch.float32, device=a.device)
        h.gemm_bf16_nt(a.data_ptr(), bt.data_ptr(), out.data_ptr(), bptr, M, N, K, a.stride(0), bt.stride(0),
                       out.stride(0), relu, sp, cu_budget, ws.data_ptr() if ws is not None else 0, wsf)
    return out


def gemm_fp8(a: torch.Tensor, bt: torch.Tensor, out: Optional[torch.Tensor] = None,
             bias: Optional[torch.Tensor] = None, relu: bool = False, stream: Optional[torch.cuda.Stream] = None,
             cu_budget: int = 0) -> torch.Tensor:
    """out[M,N] = act(a[M,K] @ bt[N,K]^T + bias[N]) -- e4m3fn operands, fp32 accumulate, bf16
    out, on the block-scaled fp8 MFMA (unit scales).  M, N multiples of 64, K of 128."""
    M, N, K, out, bptr = _gemm_operands("gemm_fp8", FP8, 128, True, a, bt, out, bias)
    with torch.cuda.device(a.device):
        _native.hip().gemm_fp8_nt(a.data_ptr(), bt.data_ptr(), out.data_ptr(), bptr, M, N, K, a.stride(0),
                                  bt.stride(0), out.stride(0), relu, _stream_ptr(stream, a.device), cu_budget)
    return out


def triad(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor, s: float = 1.5, blocks: int = 0,
          stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """a = b + s*c (fp32, contiguous, numel % 4 == 0)."""
    _check_devices("triad", a, b, c)
    for t in (a, b, c):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("triad expects contiguous fp32 device tensors")
    n = a.numel()
    if b.numel() != n or c.numel() != n or n % 4:
        raise ValueError("triad: sizes must match and be a multiple of 4")
    with torch.cuda.device(a.device):
        _native.hip().stream_triad(a.data_ptr(), b.data_ptr(), c.data_ptr(), float(s), n, int(blocks),
                                   _stream_ptr(stream, a.device))
    return a


GATHER_D_MIN, GATHER_D_MAX = 64, 2048


def embedding_bag(table: torch.Tensor, idx: torch.Tensor, offsets: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None, blocks: int = 0, stream: Optional[torch.cuda.Stream] = None,
                  check_indices: bool = True) -> torch.Tensor:
    """out[b, :] = bf16(sum of table[idx[j], :] over j in [offsets[b], offsets[b+1])) -- bf16 rows,
    fp32 accumulate, one rounding; an empty bag gives a row of +0.0.  idx 2-D [B, P] (no offsets):
    bag b is row b.  blocks > 0 caps the grid (the workgroups walk the bags grid-stride).
    check_indices=False skips the device-side range check (and its sync): for callers whose
    indices are in range by construction, and under graph capture."""
    _check_devices("embedding_bag", table, idx, offsets, out)
    if table.dtype != torch.bfloat16:
        raise TypeError("embedding_bag expects a bf16 table")
    if idx.dtype != torch.int32 or (offsets is not None and offsets.dtype != torch.int32):
        raise TypeError("embedding_bag expects int32 indices and offsets")
    if table.dim() != 2 or table.stride(1) != 1:
        raise ValueError("embedding_bag expects a row-major (D-contiguous) 2-D table")
    R, D = table.shape
    if D < GATHER_D_MIN or D > GATHER_D_MAX or D & (D - 1):
        raise ValueError(f"embedding_bag: D = {D} must be a power of two in [{GATHER_D_MIN}, {GATHER_D_MAX}]")
    if R > 1 and (table.stride(0) < D or table.stride(0) % 8):
        raise ValueError(f"embedding_bag: table row stride {table.stride(0)} must be >= D and a multiple of 8")
    if table.data_ptr() % 16:
        raise ValueError("embedding_bag: table must be 16-byte aligned")
    if idx.dim() == 2:
        if offsets is not None:
            raise ValueError("embedding_bag: a 2-D idx is fixed pooling and takes no offsets")
        if not idx.is_contiguous():
            raise ValueError("embedding_bag expects contiguous indices")
        B, P = idx.shape
        if B * P >= 2 ** 31:
            raise ValueError("embedding_bag: more than 2^31 - 1 indices")
        # made on the launch stream: the kernel that reads them, and the allocator's reuse of their
        # memory after this call, are then ordered with it
        with _launch_stream(stream, idx.device):
            offsets = torch.arange(B + 1, dtype=torch.int32, device=idx.device) * P
        idx = idx.reshape(-1)
    elif idx.dim() == 1:
        if offsets is None:
            raise ValueError("embedding_bag: a 1-D idx needs offsets")
        if offsets.dim() != 1 or offsets.numel() < 1:
            raise ValueError("embedding_bag: offsets must be 1-D of length B + 1")
        if not idx.is_contiguous() or not offsets.is_contiguous():
            raise ValueError("embedding_bag expects contiguous indices and offsets")
        B = offsets.numel() - 1
    else:
        raise ValueError(f"embedding_bag: idx must be 1-D or 2-D (got {idx.dim()}-D)")
    L = idx.numel()
    if L >= 2 ** 31 or B >= 2 ** 31:
        raise ValueError("embedding_bag: more than 2^31 - 1 indices or bags")
    if out is None:
        out = torch.empty((B, D), dtype=torch.bfloat16, device=table.device)
    if out.dim() != 2 or out.shape != (B, D) or out.dtype != torch.bfloat16 or out.stride(1) != 1:
        raise ValueError("bad output tensor")
    if B > 1 and (out.stride(0) < D or out.stride(0) % 8):
        raise ValueError(f"embedding_bag: output row stride {out.stride(0)} must be >= D and a multiple of 8")
    if out.data_ptr() % 16:
        raise ValueError("embedding_bag: out must be 16-byte aligned")
    ld_table, ld_out = _row_stride(table, R, D), _row_stride(out, B, D)
    h = _native.hip()
    with torch.cuda.device(table.device):
        sp = _stream_ptr(stream, table.device)
        if check_indices:
            with _launch_stream(stream, table.device):
                pos = torch.arange(L, dtype=torch.int32, device=idx.device)
                named = (pos >= offsets[0]) & (pos < offsets[-1])      # only these are read as indices
                bad = torch.stack([(((idx < 0) | (idx >= R)) & named).any(), (offsets[1:] < offsets[:-1]).any(),
                                   offsets[0] < 0, offsets[-1] > L]).tolist()          # the one sync
            if bad[0]:
                raise ValueError(f"embedding_bag: an index is outside [0, {R})")
            if bad[1] or bad[2] or bad[3]:
                raise ValueError(f"embedding_bag: offsets must be non-decreasing within [0, {L}]")
        if B:
            h.embedding_bag_bf16(table.data_ptr(), idx.data_ptr(), offsets.data_ptr(), out.data_ptr(), B, D,
                                 ld_table, ld_out, int(blocks), sp)
    return out


ATTN_GROUPS = (1, 2, 4, 8, 16)          # query heads per KV head (the MFMA's 16 columns hold a group)


def _paged_attn_operands(name: str, rows: str, q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                         block_table: torch.Tensor, ctx_lens: torch.Tensor, out: Optional[torch.Tensor],
                         q_start: Optional[torch.Tensor] = None, kv8: bool = False):
    """The host checks the two paged attentions share: dtypes, ranks, the fixed head dim and block
    size, the head ratio, the cache layout, the table and ctx_lens against the S sequences, the output
    (made when None) and the strides and alignment of q and out.  `rows` names what q's first
    dimension counts: "sequence" (decode: S is that dimension) or "token" (prefill: S is
    q_start's length less one).  kv8: both caches may be FP8 (float8_e4m3fn) instead of bf16.
    Returns (S, Hq, Hkv, NB, max_blocks, out, ld_q, ld_out, ld_table)."""
    kinds = {k_cache.dtype, v_cache.dtype}
    if kinds == {torch.bfloat16, FP8}:
        raise TypeError(f"{name}: k_cache is {_OPERAND_NAMES[k_cache.dtype]} and v_cache {_OPERAND_NAMES[v_cache.dtype]}: "
                        "one cache dtype, bf16 or float8_e4m3fn")
    if kinds == {FP8} and not kv8:
        raise TypeError(f"{name} expects bf16 q, k_cache and v_cache (it does not read an FP8 cache)")
    if q.dtype != torch.bfloat16 or kinds not in ({torch.bfloat16}, {FP8}):
        raise TypeError(f"{name} expects bf16 q, k_cache and v_cache" + (" (or float8_e4m3fn caches)" if kv8 else ""))
    if block_table.dtype != torch.int32 or ctx_lens.dtype != torch.int32:
        raise TypeError(f"{name} expects an int32 block_table and ctx_lens")
    if q_start is not None and q_start.dtype != torch.int32:
        raise TypeError(f"{name} expects an int32 q_start")
    first = "S" if q_start is None else "Tq"
    if q.dim() != 3 or k_cache.dim() != 4 or v_cache.dim() != 4 or block_table.dim() != 2 or ctx_lens.dim() != 1:
        raise ValueError(f"{name} expects q [{first}, Hq, 128], k_cache [NB, Hkv, 32, 128], "
                         "v_cache [NB, Hkv, 128, 32], block_table [S, max_blocks] and ctx_lens [S]")
    if q_start is not None and (q_start.dim() != 1 or q_start.numel() < 1):
        raise ValueError(f"{name}: q_start must be 1-D of length S + 1")
    R, Hq, D = q.shape
    S, of = (R, "q") if q_start is None else (q_start.numel() - 1, "q_start")
    NB, Hkv, T, Dk = k_cache.shape
    if D != ATTN_HEAD_DIM or Dk != ATTN_HEAD_DIM or v_cache.shape[2] != ATTN_HEAD_DIM:
        raise ValueError(f"{name}: the head dim must be {ATTN_HEAD_DIM}")
    if T != ATTN_BLOCK_TOKENS or v_cache.shape[3] != ATTN_BLOCK_TOKENS:
        raise ValueError(f"{name}: the cache block size must be {ATTN_BLOCK_TOKENS} tokens")
    if tuple(v_cache.shape) != (NB, Hkv, ATTN_HEAD_DIM, ATTN_BLOCK_TOKENS):
        raise ValueError(f"{name}: k_cache {tuple(k_cache.shape)} and v_cache {tuple(v_cache.shape)} "
                         "disagree on the blocks or the KV heads")
    if Hkv <= 0 or Hq % Hkv or Hq // Hkv not in ATTN_GROUPS:
        raise ValueError(f"{name}: Hq / Hkv = {Hq} / {Hkv} must be one of {ATTN_GROUPS}")
    if not k_cache.is_contiguous() or not v_cache.is_contiguous():
        raise ValueError(f"{name} expects contiguous caches")
    if k_cache.data_ptr() % 16 or v_cache.data_ptr() % 16:
        raise ValueError(f"{name}: the caches must be 16-byte aligned")
    if block_table.shape[0] != S or ctx_lens.shape[0] != S:
        raise ValueError(f"{name}: block_table {tuple(block_table.shape)} / ctx_lens "
                         f"{tuple(ctx_lens.shape)} do not match the {S} sequences of {of}")
    max_blocks = block_table.shape[1]
    if max_blocks > 1 and block_table.stride(1) != 1:
        raise ValueError(f"{name} expects contiguous block_table rows")
    if S > 1 and block_table.stride(0) < max_blocks:
        raise ValueError(f"{name}: block_table row stride {block_table.stride(0)} must be >= {max_blocks}")
    if S > 1 and ctx_lens.stride(0) != 1:
        raise ValueError(f"{name} expects contiguous ctx_lens")
    if q_start is not None and S > 0 and q_start.stride(0) != 1:
        raise ValueError(f"{name} expects a contiguous q_start")
    if S * Hkv >= 2 ** 31 or NB * Hkv >= 2 ** 31 or R >= 2 ** 31:
        raise ValueError(f"{name}: more than 2^31 - 1 workgroups, cache slabs or rows of q")
    if out is None:
        out = torch.empty((R, Hq, D), dtype=torch.bfloat16, device=q.device)
    if out.dim() != 3 or tuple(out.shape) != (R, Hq, D) or out.dtype != torch.bfloat16:
        raise ValueError("bad output tensor")
    slab = Hq * ATTN_HEAD_DIM
    for nm, t in (("q", q), ("out", out)):
        if t.stride(2) != 1 or (Hq > 1 and t.stride(1) != ATTN_HEAD_DIM):
            raise ValueError(f"{name}: {nm} must have contiguous [Hq, {ATTN_HEAD_DIM}] slabs")
        if R > 1 and (t.stride(0) < slab or t.stride(0) % 8):
            raise ValueError(f"{name}: {nm} {rows} stride {t.stride(0)} must be >= {slab} "
                             "and a multiple of 8")
        if t.data_ptr() % 16:
            raise ValueError(f"{name}: {nm} must be 16-byte aligned")
    return (S, Hq, Hkv, NB, max_blocks, out, _row_stride(q, R, slab), _row_stride(out, R, slab),
            _row_stride(block_table, S, max_blocks))


def _kv8_scales(name: str, k_cache: torch.Tensor, k_scale: Optional[torch.Tensor], v_scale: Optional[torch.Tensor],
                Hkv: int) -> bool:
    """The scales of a paged cache against its dtype: True for FP8 caches (both scales needed: fp32 [Hkv],
    contiguous, on the caches' device), False for bf16 ones (no scale may be given)."""
    if k_cache.dtype != FP8:
        if k_scale is not None or v_scale is not None:
            raise ValueError(f"{name}: k_scale / v_scale belong to float8_e4m3fn caches, these are bf16")
        return False
    if k_scale is None or v_scale is None:
        raise ValueError(f"{name}: float8_e4m3fn caches need k_scale and v_scale")
    for nm, t in (("k_scale", k_scale), ("v_scale", v_scale)):
        if t.dtype != torch.float32:
            raise TypeError(f"{name} expects an fp32 {nm}")
        if t.device != k_cache.device:
            raise ValueError(f"{name}: {nm} on {t.device}, the caches on {k_cache.device}")
        if t.dim() != 1 or t.shape[0] != Hkv or not t.is_contiguous():
            raise ValueError(f"{name}: {nm} {tuple(t.shape)} must be a contiguous [{Hkv}] vector, one scale per KV head")
    return True


def _scales_bad(k_scale: torch.Tensor, v_scale: torch.Tensor) -> torch.Tensor:
    """A device boolean: a scale that is not finite and > 0 (a NaN compares false)."""
    return ~((k_scale > 0) & k_scale.isfinite()).all() | ~((v_scale > 0) & v_scale.isfinite()).all()


def _named_blocks_bad(block_table: torch.Tensor, ctx_lens: torch.Tensor, NB: int, max_blocks: int):
    """Two device booleans: a context length outside [0, 32 * max_blocks]; a block id outside [0, NB)
    among the ceil(ctx / 32) leading entries of a row, the only ones read as block ids."""
    need = (ctx_lens + (ATTN_BLOCK_TOKENS - 1)) // ATTN_BLOCK_TOKENS
    named = torch.arange(max_blocks, dtype=torch.int32, device=ctx_lens.device)[None, :] < need[:, None]
    return (((ctx_lens < 0) | (ctx_lens > ATTN_BLOCK_TOKENS * max_blocks)).any(),
            (((block_table < 0) | (block_table >= NB)) & named).any())


def paged_decode_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, block_table: torch.Tensor,
                           ctx_lens: torch.Tensor, out: Optional[torch.Tensor] = None, scale: Optional[float] = None,
                           stream: Optional[torch.cuda.Stream] = None, check: bool = True, kv_splits: int = 1,
                           workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[s, h, :] = bf16(softmax_t(scale * q[s, h, :] . K[t, g, :]) . V[t, g, :]) over the ctx_lens[s]
    tokens of sequence s, g = h // (Hq // Hkv): one new token per sequence against a paged KV cache.
    Token t is slot t % 32 of block block_table[s, t // 32]; k_cache [NB, Hkv, 32, 128], v_cache
    [NB, Hkv, 128, 32].  scale defaults to 1 / sqrt(128).  ctx_lens[s] == 0 gives a row of +0.0.
    check=False skips the device-side check of ctx_lens and the block ids (and its sync): for
    callers that guarantee them, and under graph capture.

    kv_splits == 1 is one workgroup per (sequence, KV head); the workspace is neither needed nor
    touched.  2 <= kv_splits <= ATTN_MAX_KV_SPLITS is the split-KV launch pair for a few long
    sequences: kv_splits workgroups per (sequence, KV head), each over the contiguous range of
    blocks decode_split_range gives it (with nblk = ceil(ctx / 32) and bps = ceil(nblk /
    kv_splits), split p takes [p * bps, min(nblk, (p + 1) * bps)); empty where p * bps >= nblk),
    write fp32 partials to `workspace`, and a merge kernel on the same stream combines them.
    workspace is a contiguous, 16-byte aligned fp32 tensor on the operands' device of at least
    decode_split_workspace_floats(S, Hq, kv_splits) elements; None allocates one on the launch
    stream.  One workspace serves ONE launch in flight: two launches on different streams need two,
    and a caller under graph capture passes its own (it must outlive the graph).

    The caches are bf16; paged_decode_attention_kv8 is the same attention over an FP8 cache."""
    return _paged_decode("paged_decode_attention", False, q, k_cache, v_cache, block_table, ctx_lens, None, None, out,
                         scale, stream, check, kv_splits, workspace)


def paged_decode_attention_kv8(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, block_table: torch.Tensor,
                               ctx_lens: torch.Tensor, k_scale: Optional[torch.Tensor] = None,
                               v_scale: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                               scale: Optional[float] = None, stream: Optional[torch.cuda.Stream] = None,
                               check: bool = True, kv_splits: int = 1,
                               workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """paged_decode_attention over an FP8 cache: both caches torch.float8_e4m3fn (FP8) with k_scale and v_scale, fp32
    [Hkv], contiguous, on the operands' device: a stored byte c of KV head g stands for e4m3fn(c) * scale[g] (THE
    FP8 KV FORMAT, native/hip/api.h; rope_append writes it).  The kernels dequantise in registers -- exactly --
    and keep the bf16 MFMAs: scores = mfma_sum * (scale * k_scale[g]), the two scalars multiplied once in fp32,
    and out = bf16((acc / lsum) * v_scale[g]); everything else, kv_splits and the workspace included, is
    paged_decode_attention's.  check=True also verifies, in the same sync, that the scales are finite and > 0.
    bf16 caches (with or without scales) raise ValueError, mixed cache dtypes TypeError.  (A function of its
    own and not two more keywords of paged_decode_attention: that function's parameter list is pinned.)"""
    return _paged_decode("paged_decode_attention_kv8", True, q, k_cache, v_cache, block_table, ctx_lens, k_scale,
                         v_scale, out, scale, stream, check, kv_splits, workspace)


def _paged_decode(name, fp8, q, k_cache, v_cache, block_table, ctx_lens, k_scale, v_scale, out, scale, stream, check,
                  kv_splits, workspace):
    """The two decode wrappers: fp8 says which cache dtype the caller's function reads."""
    _check_devices(name, q, k_cache, v_cache, block_table, ctx_lens, out, k_scale, v_scale)
    S, Hq, Hkv, NB, max_blocks, out, ld_q, ld_out, ld_table = _paged_attn_operands(
        name, "sequence", q, k_cache, v_cache, block_table, ctx_lens, out, kv8=fp8)
    kv8 = _kv8_scales(name, k_cache, k_scale, v_scale, Hkv)
    if fp8 and not kv8:
        raise ValueError(f"{name} reads float8_e4m3fn caches, these are bf16: paged_decode_attention reads them")
    if isinstance(kv_splits, bool) or not isinstance(kv_splits, int) or not 1 <= kv_splits <= ATTN_MAX_KV_SPLITS:
        raise ValueError(f"{name}: kv_splits = {kv_splits!r} must be an int in [1, {ATTN_MAX_KV_SPLITS}]")
    if kv_splits > 1 and workspace is not None:
        need = decode_split_workspace_floats(S, Hq, kv_splits)
        if workspace.dtype != torch.float32:
            raise TypeError(f"{name} expects an fp32 workspace")
        if workspace.device != q.device:
            raise ValueError(f"{name}: workspace on {workspace.device}, operands on {q.device}")
        if not workspace.is_contiguous() or workspace.data_ptr() % 16:
            raise ValueError(f"{name}: workspace must be contiguous and 16-byte aligned")
        if workspace.numel() < need:
            raise ValueError(f"{name}: workspace of {workspace.numel()} floats, {kv_splits} splits need {need}")
    if scale is None:
        scale = ATTN_HEAD_DIM ** -0.5
    if S == 0:
        return out
    h = _native.hip()
    with torch.cuda.device(q.device):
        sp = _stream_ptr(stream, q.device)
        if check:
            with _launch_stream(stream, q.device):
                bad = torch.stack(_named_blocks_bad(block_table, ctx_lens, NB, max_blocks)
                                  + ((_scales_bad(k_scale, v_scale),) if kv8 else ())).tolist()         # the one sync
            if bad[0]:
                raise ValueError(f"{name}: a context length is outside [0, {ATTN_BLOCK_TOKENS * max_blocks}]")
            if bad[1]:
                raise ValueError(f"{name}: a block id is outside [0, {NB})")
            if kv8 and bad[2]:
                raise ValueError(f"{name}: k_scale and v_scale must be finite and > 0")
        if kv8 and kv_splits == 1:
            h.paged_decode_kv8(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), k_scale.data_ptr(),
                               v_scale.data_ptr(), block_table.data_ptr(), ctx_lens.data_ptr(), out.data_ptr(), S, Hq,
                               Hkv, ld_q, ld_out, ld_table, float(scale), sp)
            return out
        if kv_splits == 1:
            h.paged_decode_bf16(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), block_table.data_ptr(),
                                ctx_lens.data_ptr(), out.data_ptr(), S, Hq, Hkv, ld_q, ld_out, ld_table, float(scale),
                                sp)
            return out
        if workspace is None:
            # from the caching allocator, on the launch stream: its reuse is ordered after the merge
            with _launch_stream(stream, q.device):
                workspace = torch.empty(decode_split_workspace_floats(S, Hq, kv_splits), dtype=torch.float32,
                                        device=q.device)
        if kv8:
            h.paged_decode_split_kv8(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), k_scale.data_ptr(),
                                     v_scale.data_ptr(), block_table.data_ptr(), ctx_lens.data_ptr(),
                                     workspace.data_ptr(), out.data_ptr(), S, Hq, Hkv, kv_splits, ld_q, ld_out, ld_table,
                                     float(scale), sp)
            return out
        h.paged_decode_split_bf16(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), block_table.data_ptr(),
                                  ctx_lens.data_ptr(), workspace.data_ptr(), out.data_ptr(), S, Hq, Hkv, kv_splits,
                                  ld_q, ld_out, ld_table, float(scale), sp)
    return out


def paged_prefill_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, block_table: torch.Tensor,
                            ctx_lens: torch.Tensor, q_start: torch.Tensor, max_q_len: Optional[int] = None,
                            out: Optional[torch.Tensor] = None, scale: Optional[float] = None,
                            stream: Optional[torch.cuda.Stream] = None, check: bool = True) -> torch.Tensor:
    """Chunked-prefill (append) attention over the paged KV cache of paged_decode_attention.  q and
    out are [Tq, Hq, 128], packed over the S sequences: the chunk of sequence s is rows q_start[s] ..
    q_start[s + 1] - 1 (q_start int32 [S + 1], CSR), q_len[s] of them.  ctx_lens[s] counts all tokens
    of s in the cache, the chunk's own included; query i of the chunk has position
    p = ctx_lens[s] - q_len[s] + i and
    out[row, h, :] = bf16(softmax_{t <= p}(scale * q[row, h, :] . K[t, g, :]) . V[t, g, :]), g = h // (Hq // Hkv).
    q_len[s] == 0 writes nothing; rows outside [q_start[0], q_start[S]) are neither read nor written.
    max_q_len is an upper bound on every q_len (it sizes the grid); scale defaults to 1 / sqrt(128).
    check=True verifies ctx_lens, the named block ids, q_start (non-decreasing within [0, Tq]),
    q_len <= ctx_lens and q_len <= max_q_len on the device first (one sync), and computes max_q_len
    when it is None.  check=False needs max_q_len and never syncs: for callers that guarantee all of
    it, and under graph capture.

    The caches are bf16; paged_prefill_attention_kv8 is the same attention over an FP8 cache."""
    return _paged_prefill("paged_prefill_attention", False, q, k_cache, v_cache, block_table, ctx_lens, q_start, None, None,
                          max_q_len, out, scale, stream, check)


def paged_prefill_attention_kv8(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, block_table: torch.Tensor,
                                ctx_lens: torch.Tensor, q_start: torch.Tensor, k_scale: Optional[torch.Tensor] = None,
                                v_scale: Optional[torch.Tensor] = None, max_q_len: Optional[int] = None,
                                out: Optional[torch.Tensor] = None, scale: Optional[float] = None,
                                stream: Optional[torch.cuda.Stream] = None, check: bool = True) -> torch.Tensor:
    """paged_prefill_attention over an FP8 cache: both caches torch.float8_e4m3fn (FP8) with k_scale and v_scale, fp32
    [Hkv], contiguous, on the operands' device (THE FP8 KV FORMAT, native/hip/api.h; rope_append writes it).  The
    kernel dequantises in registers -- exactly -- and keeps the bf16 MFMAs: scores = mfma_sum * (scale * k_scale[g]),
    the two scalars multiplied once in fp32, and out = bf16((acc / l) * v_scale[g]); q_len == 0, the rows outside
    the chunks, max_q_len and check are paged_prefill_attention's.  check=True also verifies, in the same sync,
    that the scales are finite and > 0.  bf16 caches (with or without scales) raise ValueError, mixed cache
    dtypes TypeError.  (A function of its own, as paged_decode_attention_kv8 is: paged_prefill_attention's
    parameter list is pinned.)"""
    return _paged_prefill("paged_prefill_attention_kv8", True, q, k_cache, v_cache, block_table, ctx_lens, q_start, k_scale,
                          v_scale, max_q_len, out, scale, stream, check)


def _paged_prefill(name, fp8, q, k_cache, v_cache, block_table, ctx_lens, q_start, k_scale, v_scale, max_q_len, out, scale,
                   stream, check):
    """The two prefill wrappers: fp8 says which cache dtype the caller's function reads."""
    _check_devices(name, q, k_cache, v_cache, block_table, ctx_lens, q_start, out, k_scale, v_scale)
    S, Hq, Hkv, NB, max_blocks, out, ld_q, ld_out, ld_table = _paged_attn_operands(
        name, "token", q, k_cache, v_cache, block_table, ctx_lens, out, q_start, kv8=fp8)
    kv8 = _kv8_scales(name, k_cache, k_scale, v_scale, Hkv)
    if fp8 and not kv8:
        raise ValueError(f"{name} reads float8_e4m3fn caches, these are bf16: paged_prefill_attention reads them")
    Tq = q.shape[0]
    if max_q_len is None and not check:
        raise ValueError(f"{name}: check=False needs max_q_len")
    if max_q_len is not None and not 0 <= max_q_len < 2 ** 31:
        raise ValueError(f"{name}: max_q_len {max_q_len} is outside [0, 2^31)")
    if scale is None:
        scale = ATTN_HEAD_DIM ** -0.5
    if S == 0 or Tq == 0 or max_q_len == 0:
        return out
    h = _native.hip()
    with torch.cuda.device(q.device):
        sp = _stream_ptr(stream, q.device)
        if check:
            with _launch_stream(stream, q.device):
                q_len = q_start[1:] - q_start[:-1]
                bad = torch.stack([b.long() for b in _named_blocks_bad(block_table, ctx_lens, NB, max_blocks)]
                                  + [((q_len < 0).any() | (q_start[0] < 0) | (q_start[-1] > Tq)).long(),
                                     (q_len > ctx_lens).any().long(), q_len.max().long()]
                                  + ([_scales_bad(k_scale, v_scale).long()] if kv8 else [])).tolist()    # the one sync
            if bad[0]:
                raise ValueError(f"{name}: a context length is outside [0, {ATTN_BLOCK_TOKENS * max_blocks}]")
            if bad[1]:
                raise ValueError(f"{name}: a block id is outside [0, {NB})")
            if bad[2]:
                raise ValueError(f"{name}: q_start must be non-decreasing within [0, {Tq}]")
            if bad[3]:
                raise ValueError(f"{name}: a chunk is longer than its sequence's context (q_len > ctx_lens)")
            if max_q_len is None:
                max_q_len = bad[4]
            elif bad[4] > max_q_len:
                raise ValueError(f"{name}: a chunk of {bad[4]} tokens is longer than max_q_len = {max_q_len}")
            if kv8 and bad[5]:
                raise ValueError(f"{name}: k_scale and v_scale must be finite and > 0")
        if max_q_len and kv8:
            h.paged_prefill_kv8(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), k_scale.data_ptr(),
                                v_scale.data_ptr(), block_table.data_ptr(), ctx_lens.data_ptr(), q_start.data_ptr(),
                                out.data_ptr(), S, Hq, Hkv, int(max_q_len), ld_q, ld_out, ld_table, float(scale), sp)
        elif max_q_len:
            h.paged_prefill_bf16(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), block_table.data_ptr(),
                                 ctx_lens.data_ptr(), q_start.data_ptr(), out.data_ptr(), S, Hq, Hkv, int(max_q_len),
                                 ld_q, ld_out, ld_table, float(scale), sp)
    return out


ROPE_BASE = 500000.0          # Llama-3's rotary base


def rope_table(max_pos: int, base: float = ROPE_BASE) -> torch.Tensor:
    """The cos_sin operand of rope_append: fp32 [max_pos, 128] on the CPU, row p holding cos(p * f_i) for
    i in [0, 64) and then sin(p * f_i), f_i = base ** (-i / 64).  The angles and their cosines and sines
    are computed in float64 and cast once."""
    if max_pos < 0:
        raise ValueError(f"rope_table: max_pos {max_pos} is negative")
    half = ATTN_HEAD_DIM // 2
    freq = torch.tensor([base ** (-i / half) for i in range(half)], dtype=torch.float64)
    ang = torch.arange(max_pos, dtype=torch.float64)[:, None] * freq[None, :]
    return torch.cat([ang.cos(), ang.sin()], dim=1).to(torch.float32)


def _storage_range(t: torch.Tensor):
    """[lo, hi): the bytes between the first and the last element of t, as addresses."""
    if t.numel() == 0:
        return t.data_ptr(), t.data_ptr()
    last = sum((n - 1) * st for n, st in zip(t.shape, t.stride()))
    return t.data_ptr(), t.data_ptr() + (last + 1) * t.element_size()


def rope_append(qkv: torch.Tensor, cos_sin: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                block_table: torch.Tensor, ctx_lens: torch.Tensor, q_start: torch.Tensor,
                max_q_len: Optional[int] = None, q_out: Optional[torch.Tensor] = None,
                stream: Optional[torch.cuda.Stream] = None, check: bool = True,
                k_scale: Optional[torch.Tensor] = None, v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Rotary position embedding of q and K and the append of the new K / V to the paged KV cache of the
    attentions.  qkv is [Tq, Hq + 2 * Hkv, 128] -- the Hq query heads, the Hkv K heads, the Hkv V heads,
    what a fused QKV projection produces --, packed over the S sequences by q_start (int32 [S + 1], CSR)
    as paged_prefill_attention's q is.  ctx_lens[s] counts the chunk's own tokens: row q_start[s] + i is
    token p = ctx_lens[s] - q_len[s] + i of s and goes to slot p % 32 of block block_table[s, p // 32].
    cos_sin is fp32 [max_pos, 128], row p holding 64 cosines and then 64 sines (rope_table).  With
    x1 = x[i], x2 = x[i + 64], c = cos_sin[p, i] and s = cos_sin[p, 64 + i] for i in [0, 64), in fp32,
    y[i] = fma(x1, c, -(x2 * s)) and y[i + 64] = fma(x2, c, x1 * s), rounded to bf16 once: the rotated q
    heads go to q_out [Tq, Hq, 128] (made when None; returned), the rotated K heads to
    k_cache[block, g, slot, :]; V is copied bit for bit to v_cache[block, g, :, slot].  The caches are
    never read and nothing else of them is written; q_len[s] == 0 writes nothing; replaying the launch
    gives the same.  max_q_len is an upper bound on every q_len (it sizes the grid).
    check=True verifies on the device first (one sync): ctx_lens within [0, 32 * max_blocks] and at most
    max_pos, q_start non-decreasing within [0, Tq], q_len <= ctx_lens and q_len <= max_q_len (computed
    when None), the table entries the chunks touch -- (ctx - q_len) // 32 .. (ctx - 1) // 32 of each
    sequence with q_len > 0 -- within [0, NB) and pairwise distinct over the launch (two sequences
    appending into one block is a silent race).  check=False needs max_q_len and never syncs: for
    callers that guarantee all of it, and under graph capture.

    The caches are bf16, or both torch.float8_e4m3fn (FP8) with k_scale and v_scale, fp32 [Hkv], contiguous, on
    the operands' device (THE FP8 KV FORMAT, native/hip/api.h).  q_out is then unchanged; the K byte is
    quantize_kv8_reference(y / k_scale[g]) with y the fp32 rotation result, NOT first rounded to bf16, and the V
    byte quantize_kv8_reference(float(v) / v_scale[g]), both divisions IEEE fp32 (rope_append_kv8_reference).
    check=True also verifies, in the same sync, that the scales are finite and > 0.  bf16 caches with a scale
    given raise ValueError, mixed cache dtypes TypeError."""
    name = "rope_append"
    _check_devices(name, qkv, cos_sin, k_cache, v_cache, block_table, ctx_lens, q_start, q_out, k_scale, v_scale)
    if cos_sin.dtype != torch.float32:
        raise TypeError(f"{name} expects an fp32 cos_sin")
    if qkv.dtype != torch.bfloat16:
        raise TypeError(f"{name} expects bf16 qkv, k_cache and v_cache")
    if (qkv.dim() != 3 or cos_sin.dim() != 2 or k_cache.dim() != 4 or v_cache.dim() != 4 or block_table.dim() != 2
            or ctx_lens.dim() != 1):
        raise ValueError(f"{name} expects qkv [Tq, Hq + 2 * Hkv, 128], cos_sin [max_pos, 128], k_cache [NB, Hkv, 32, 128], "
                         "v_cache [NB, Hkv, 128, 32], block_table [S, max_blocks], ctx_lens [S] and q_start [S + 1]")
    Tq, Ht = qkv.shape[0], qkv.shape[1]
    Hq = Ht - 2 * k_cache.shape[1]
    if Hq <= 0:
        raise ValueError(f"{name}: qkv has {Ht} heads, the caches {k_cache.shape[1]} KV heads: no Hq + 2 * Hkv")
    slab = Ht * ATTN_HEAD_DIM
    if qkv.shape[2] != ATTN_HEAD_DIM:
        raise ValueError(f"{name}: the head dim must be {ATTN_HEAD_DIM}")
    if qkv.stride(2) != 1 or (Ht > 1 and qkv.stride(1) != ATTN_HEAD_DIM):
        raise ValueError(f"{name}: qkv must have contiguous [Hq + 2 * Hkv, {ATTN_HEAD_DIM}] slabs")
    if Tq > 1 and (qkv.stride(0) < slab or qkv.stride(0) % 8):
        raise ValueError(f"{name}: qkv token stride {qkv.stride(0)} must be >= {slab} and a multiple of 8")
    ld_qkv = _row_stride(qkv, Tq, slab)
    # the q heads as a view: the attentions' checks then cover the caches, the table, ctx_lens, q_start, the
    # head dim, the group, qkv's alignment and q_out
    S, Hq, Hkv, NB, max_blocks, q_out, _, ld_q_out, ld_table = _paged_attn_operands(
        name, "token", qkv[:, :Hq], k_cache, v_cache, block_table, ctx_lens, q_out, q_start, kv8=True)
    kv8 = _kv8_scales(name, k_cache, k_scale, v_scale, Hkv)
    if cos_sin.shape[1] != ATTN_HEAD_DIM:
        raise ValueError(f"{name}: cos_sin must be [max_pos, {ATTN_HEAD_DIM}]: 64 cosines, then 64 sines")
    if not cos_sin.is_contiguous() or cos_sin.data_ptr() % 16:
        raise ValueError(f"{name}: cos_sin must be contiguous and 16-byte aligned")
    max_pos = cos_sin.shape[0]
    if max_pos >= 2 ** 31:
        raise ValueError(f"{name}: more than 2^31 - 1 rows of cos_sin")
    (a0, a1), (b0, b1) = _storage_range(qkv), _storage_range(q_out)
    if a0 < b1 and b0 < a1:
        raise ValueError(f"{name}: q_out overlaps qkv (q is not rotated in place: a replayed launch must give the same)")
    if max_q_len is None and not check:
        raise ValueError(f"{name}: check=False needs max_q_len")
    if max_q_len is not None and not 0 <= max_q_len < 2 ** 31:
        raise ValueError(f"{name}: max_q_len {max_q_len} is outside [0, 2^31)")
    if S == 0 or Tq == 0 or max_q_len == 0:
        return q_out
    h = _native.hip()
    with torch.cuda.device(qkv.device):
        sp = _stream_ptr(stream, qkv.device)
        if check:
            with _launch_stream(stream, qkv.device):
                q_len = q_start[1:] - q_start[:-1]
                first = (ctx_lens - q_len) // ATTN_BLOCK_TOKENS               # floor: negative where q_len > ctx
                last = (ctx_lens - 1) // ATTN_BLOCK_TOKENS
                col = torch.arange(max_blocks, dtype=torch.int32, device=qkv.device)[None, :]
                touched = (col >= first[:, None]) & (col <= last[:, None]) & (q_len > 0)[:, None]
                # the untouched entries as ids of their own past every block, then equal neighbours after a sort
                own = NB + torch.arange(S * max_blocks, dtype=torch.int64, device=qkv.device).view(S, max_blocks)
                ids = torch.where(touched, block_table.long(), own).flatten().sort().values
                bad = torch.stack([((ctx_lens < 0) | (ctx_lens > ATTN_BLOCK_TOKENS * max_blocks)).any().long(),
                                   (ctx_lens > max_pos).any().long(),
                                   ((q_len < 0).any() | (q_start[0] < 0) | (q_start[-1] > Tq)).long(),
                                   (q_len > ctx_lens).any().long(), q_len.max().long(),
                                   (((block_table < 0) | (block_table >= NB)) & touched).any().long(),
                                   (ids[1:] == ids[:-1]).any().long()]
                                  + ([_scales_bad(k_scale, v_scale).long()] if kv8 else [])).tolist()   # the one sync
            if bad[0]:
                raise ValueError(f"{name}: a context length is outside [0, {ATTN_BLOCK_TOKENS * max_blocks}]")
            if bad[1]:
                raise ValueError(f"{name}: a context length is past the {max_pos} positions of cos_sin")
            if bad[2]:
                raise ValueError(f"{name}: q_start must be non-decreasing within [0, {Tq}]")
            if bad[3]:
                raise ValueError(f"{name}: a chunk is longer than its sequence's context (q_len > ctx_lens)")
            if max_q_len is None:
                max_q_len = bad[4]
            elif bad[4] > max_q_len:
                raise ValueError(f"{name}: a chunk of {bad[4]} tokens is longer than max_q_len = {max_q_len}")
            if bad[5]:
                raise ValueError(f"{name}: a block id is outside [0, {NB})")
            if bad[6]:
                raise ValueError(f"{name}: two chunks append into one cache block")
            if kv8 and bad[7]:
                raise ValueError(f"{name}: k_scale and v_scale must be finite and > 0")
        if max_q_len and kv8:
            h.rope_append_kv8(qkv.data_ptr(), cos_sin.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                              k_scale.data_ptr(), v_scale.data_ptr(), block_table.data_ptr(), ctx_lens.data_ptr(),
                              q_start.data_ptr(), q_out.data_ptr(), S, Hq, Hkv, int(max_q_len), int(max_pos), ld_qkv,
                              ld_q_out, ld_table, sp)
        elif max_q_len:
            h.rope_append_bf16(qkv.data_ptr(), cos_sin.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                               block_table.data_ptr(), ctx_lens.data_ptr(), q_start.data_ptr(), q_out.data_ptr(), S, Hq,
                               Hkv, int(max_q_len), int(max_pos), ld_qkv, ld_q_out, ld_table, sp)
    return q_out


RMSNORM_D_MIN, RMSNORM_D_MAX = 8, 8192


def _bf16_rows(name: str, nm: str, t: torch.Tensor, cols: Optional[int] = None) -> int:
    """The checks add_rmsnorm and swiglu make of every 2-D operand: bf16, 2-D (of `cols` columns when
    given), last dim contiguous, a row stride >= the row length and a multiple of 8, the first element
    16-byte aligned, fewer than 2^31 rows.  Returns the row stride in elements."""
    if t.dtype != torch.bfloat16:
        raise TypeError(f"{name} expects bf16 tensors ({nm} is {t.dtype})")
    if t.dim() != 2 or (cols is not None and t.shape[1] != cols):
        raise ValueError(f"{name}: {nm} must be 2-D" + (f" with {cols} columns" if cols is not None else "")
                         + f" (got {tuple(t.shape)})")
    rows, n = t.shape
    if n > 1 and t.stride(1) != 1:
        raise ValueError(f"{name}: {nm} must have contiguous rows")
    if rows > 1 and (t.stride(0) < n or t.stride(0) % 8):
        raise ValueError(f"{name}: {nm} row stride {t.stride(0)} must be >= {n} and a multiple of 8")
    if t.data_ptr() % 16:
        raise ValueError(f"{name}: {nm} must be 16-byte aligned")
    if rows >= 2 ** 31:
        raise ValueError(f"{name}: more than 2^31 - 1 rows")
    return _row_stride(t, rows, n)


def _overlap(a: torch.Tensor, b: torch.Tensor) -> bool:
    (a0, a1), (b0, b1) = _storage_range(a), _storage_range(b)
    return a0 < b1 and b0 < a1


def add_rmsnorm(x: torch.Tensor, weight: torch.Tensor, residual: Optional[torch.Tensor] = None, eps: float = 1e-5,
                out: Optional[torch.Tensor] = None, residual_out: Optional[torch.Tensor] = None,
                stream: Optional[torch.cuda.Stream] = None):
    """Residual add + RMSNorm over the rows of x [T, D] (bf16, D a multiple of 8 in [8, 8192]), weight bf16
    [D].  With a residual [T, D]: residual_out = bf16(fp32(x) + fp32(residual)) and, from the ROUNDED sum
    hb = fp32(residual_out), y = bf16((hb * r) * fp32(weight)) with r = 1 / sqrt(mean(hb^2) + eps) in fp32;
    returns (y, residual_out).  Without one hb = fp32(x), nothing but y is written and y is returned:
    add_rmsnorm(x, w, residual)[0] is bit for bit add_rmsnorm(residual_out, w).  `out` and `residual_out`
    are made when None.  residual_out may be EXACTLY residual (same data_ptr, shape and strides): the
    in-place update of the residual stream -- a thread reads its chunks before it writes them.  A captured
    launch of that form is not idempotent: every replay adds x again.  Any other overlap of an output with
    an operand or with the other output raises.  eps is finite, >= 0 and rounded to fp32 once, here.
    T == 0 launches nothing."""
    name = "add_rmsnorm"
    _check_devices(name, x, weight, residual, out, residual_out)
    if x.dim() == 2 and (x.shape[1] < RMSNORM_D_MIN or x.shape[1] > RMSNORM_D_MAX or x.shape[1] % 8):
        raise ValueError(f"{name}: D = {x.shape[1]} must be a multiple of 8 in [{RMSNORM_D_MIN}, {RMSNORM_D_MAX}]")
    ld_x = _bf16_rows(name, "x", x)
    T, D = x.shape
    if weight.dtype != torch.bfloat16:
        raise TypeError(f"{name} expects bf16 tensors (weight is {weight.dtype})")
    if weight.dim() != 1 or weight.numel() != D or not weight.is_contiguous() or weight.data_ptr() % 16:
        raise ValueError(f"{name}: weight must be a contiguous, 16-byte aligned vector of length D = {D}")
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not 0.0 <= eps < float("inf"):
        raise ValueError(f"{name}: eps = {eps!r} must be finite and >= 0")
    eps32 = torch.tensor(float(eps), dtype=torch.float32).item()          # rounded to fp32 once
    if eps32 == float("inf"):
        raise ValueError(f"{name}: eps = {eps!r} is past the fp32 range")
    if residual is None and residual_out is not None:
        raise ValueError(f"{name}: residual_out without a residual")
    ld_res = ld_ro = 0
    if residual is not None:
        ld_res = _bf16_rows(name, "residual", residual, D)
        if residual.shape[0] != T:
            raise ValueError(f"{name}: residual {tuple(residual.shape)} does not match x {tuple(x.shape)}")
        if residual_out is None:
            residual_out = torch.empty((T, D), dtype=torch.bfloat16, device=x.device)
        ld_ro = _bf16_rows(name, "residual_out", residual_out, D)
        if residual_out.shape[0] != T:
            raise ValueError(f"{name}: residual_out {tuple(residual_out.shape)} does not match x {tuple(x.shape)}")
    if out is None:
        out = torch.empty((T, D), dtype=torch.bfloat16, device=x.device)
    ld_y = _bf16_rows(name, "out", out, D)
    if out.shape[0] != T:
        raise ValueError(f"{name}: out {tuple(out.shape)} does not match x {tuple(x.shape)}")
    for nm, t in (("x", x), ("weight", weight), ("residual", residual), ("residual_out", residual_out)):
        if t is not None and _overlap(out, t):
            raise ValueError(f"{name}: out overlaps {nm}")
    if residual_out is not None:
        in_place = (residual_out.data_ptr() == residual.data_ptr() and residual_out.shape == residual.shape
                    and residual_out.stride() == residual.stride())
        for nm, t in (("x", x), ("weight", weight), ("residual", None if in_place else residual)):
            if t is not None and _overlap(residual_out, t):
                raise ValueError(f"{name}: residual_out overlaps {nm} (it may only be exactly residual)")
    result = out if residual is None else (out, residual_out)
    if T == 0:
        return result
    h = _native.hip()
    with torch.cuda.device(x.device):
        h.add_rmsnorm_bf16(x.data_ptr(), residual.data_ptr() if residual is not None else 0, weight.data_ptr(),
                           residual_out.data_ptr() if residual is not None else 0, out.data_ptr(), T, D, ld_x, ld_res,
                           ld_ro, ld_y, eps32, _stream_ptr(stream, x.device))
    return result


def swiglu(gate_up: torch.Tensor, out: Optional[torch.Tensor] = None,
           stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """out[t, j] = bf16(silu(g) * u) with g = gate_up[t, j], u = gate_up[t, F + j] -- gate_up bf16 [T, 2F], the
    output of a fused gate / up projection, out bf16 [T, F] (made when None), F a multiple of 8.  In fp32:
    e = exp2(-g * log2 e) on the hardware exponential, s = g / (1 + e) (an IEEE division), s * u rounded to
    bf16 once.  out may not overlap gate_up.  T == 0 launches nothing; replaying a launch gives the same."""
    name = "swiglu"
    _check_devices(name, gate_up, out)
    if gate_up.dim() == 2 and (gate_up.shape[1] < 16 or gate_up.shape[1] % 16):
        raise ValueError(f"{name}: gate_up has {gate_up.shape[1]} columns: no 2 * F with F a positive multiple of 8")
    ld_in = _bf16_rows(name, "gate_up", gate_up)
    T, F2 = gate_up.shape
    F = F2 // 2
    if T * (F // 8) >= 2 ** 31 * 1024:
        raise ValueError(f"{name}: more than 2^31 - 1 workgroups")
    if out is None:
        out = torch.empty((T, F), dtype=torch.bfloat16, device=gate_up.device)
    ld_out = _bf16_rows(name, "out", out, F)
    if out.shape[0] != T:
        raise ValueError(f"{name}: out {tuple(out.shape)} does not match gate_up {tuple(gate_up.shape)}")
    if _overlap(out, gate_up):
        raise ValueError(f"{name}: out overlaps gate_up")
    if T == 0:
        return out
    h = _native.hip()
    with torch.cuda.device(gate_up.device):
        h.swiglu_bf16(gate_up.data_ptr(), out.data_ptr(), T, F, ld_in, ld_out, _stream_ptr(stream, gate_up.device))
    return out


SAMPLE_V_MIN, SAMPLE_V_MAX = 8, 131072
SAMPLE_MAX_TOP_K = 64


def sample_tokens(logits: torch.Tensor, u: torch.Tensor, temperature: torch.Tensor, top_k: torch.Tensor,
                  top_p: torch.Tensor, out: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                  check: bool = True) -> torch.Tensor:
    """Top-k / top-p sampling of one token per row of logits bf16 [S, V] (V a multiple of 8 in [8, 131072]);
    returns out, int32 [S] (made when None).  Per row s, with the parameters temperature[s] (fp32), top_k[s]
    (int32), top_p[s] (fp32) and the caller's uniform u[s] (fp32, in [0, 1): there is no RNG in the kernel, so a
    replayed launch gives the same): the k = min(clamp(top_k, 1, 64), V) largest logits, ties at the threshold
    to the lowest indices, ranked c_0 .. c_{k-1} by (value descending, index ascending); in fp32
    w_j = exp2((l_{c_j} - l_{c_0}) * (1.44269504f / temperature)) on the hardware exponential, cum the
    inclusive prefix sum of w; n the smallest n >= 1 with cum_{n-1} >= top_p * cum_{k-1}; the token is c_j for
    the smallest j < n with cum_j > u * cum_{n-1}, c_{n-1} if there is none.  temperature == 0 or top_k == 1 is
    greedy: the lowest index of the row maximum, u and top_p unused (they may be NaN).  A row with a NaN, or
    whose maximum is -Inf, gives -1; a maximum of +Inf gives its lowest index; no other row is affected.
    check=True verifies on the device first (one sync): 1 <= top_k <= 64, temperature finite and >= 0, and on
    the rows that are not greedy 0 < top_p <= 1 and 0 <= u < 1.  check=False never syncs (the kernel still
    clamps top_k into [1, 64]): for callers that guarantee the parameters, and under graph capture.
    S == 0 launches nothing."""
    name = "sample_tokens"
    _check_devices(name, logits, u, temperature, top_k, top_p, out)
    if logits.dtype != torch.bfloat16:
        raise TypeError(f"{name} expects bf16 logits (got {logits.dtype})")
    for nm, t in (("u", u), ("temperature", temperature), ("top_p", top_p)):
        if t.dtype != torch.float32:
            raise TypeError(f"{name} expects an fp32 {nm} (got {t.dtype})")
    if top_k.dtype != torch.int32:
        raise TypeError(f"{name} expects an int32 top_k (got {top_k.dtype})")
    if out is not None and out.dtype != torch.int32:
        raise TypeError(f"{name} expects an int32 out (got {out.dtype})")
    ld = _bf16_rows(name, "logits", logits)
    S, V = logits.shape
    if V < SAMPLE_V_MIN or V > SAMPLE_V_MAX or V % 8:
        raise ValueError(f"{name}: V = {V} must be a multiple of 8 in [{SAMPLE_V_MIN}, {SAMPLE_V_MAX}]")
    for nm, t in (("u", u), ("temperature", temperature), ("top_k", top_k), ("top_p", top_p)):
        if t.dim() != 1 or t.numel() != S or not t.is_contiguous():
            raise ValueError(f"{name}: {nm} must be a contiguous vector of length S = {S} (got {tuple(t.shape)})")
    if out is None:
        out = torch.empty(S, dtype=torch.int32, device=logits.device)
    if out.dim() != 1 or out.numel() != S or not out.is_contiguous():
        raise ValueError(f"{name}: out must be a contiguous vector of length S = {S} (got {tuple(out.shape)})")
    for nm, t in (("logits", logits), ("u", u), ("temperature", temperature), ("top_k", top_k), ("top_p", top_p)):
        if _overlap(out, t):
            raise ValueError(f"{name}: out overlaps {nm}")
    if S == 0:
        return out
    h = _native.hip()
    with torch.cuda.device(logits.device):
        sp = _stream_ptr(stream, logits.device)
        if check:
            with _launch_stream(stream, logits.device):
                sampled = (temperature != 0) & (top_k != 1)
                bad = torch.stack([((top_k < 1) | (top_k > SAMPLE_MAX_TOP_K)).any(),
                                   (~torch.isfinite(temperature) | (temperature < 0)).any(),
                                   (~((top_p > 0) & (top_p <= 1)) & sampled).any(),
                                   (~((u >= 0) & (u < 1)) & sampled).any()]).tolist()          # the one sync
            if bad[0]:
                raise ValueError(f"{name}: a top_k is outside [1, {SAMPLE_MAX_TOP_K}]")
            if bad[1]:
                raise ValueError(f"{name}: a temperature is negative or not finite")
            if bad[2]:
                raise ValueError(f"{name}: a top_p of a sampled row is outside (0, 1]")
            if bad[3]:
                raise ValueError(f"{name}: a u of a sampled row is outside [0, 1)")
        h.sample_topk_bf16(logits.data_ptr(), u.data_ptr(), temperature.data_ptr(), top_k.data_ptr(), top_p.data_ptr(),
                           out.data_ptr(), S, V, ld, sp)
    return out


def moe_topk_reference(logits: torch.Tensor, top_k: int):
    """(topk_ids int32 [T, k], topk_w fp32 [T, k]) of moe_route in pure torch, on logits' device: the k largest by
    (value descending, index ascending) -- a stable descending sort of the values, so ties and +-0 go to the lowest
    index -- and the softmax over the selected logits, computed in float64 and cast once.  The ids are the kernel's
    exactly for rows without a NaN; the weights are the kernel's within its fp32 rounding."""
    order = logits.double().sort(dim=1, descending=True, stable=True)
    ids, l = order.indices[:, :top_k], order.values[:, :top_k]
    e = torch.exp2((l - l[:, :1]) * 1.4426950408889634)
    return ids.to(torch.int32), (e / e.sum(dim=1, keepdim=True)).to(torch.float32)


def moe_align_reference(topk_ids: torch.Tensor, E: int):
    """(sorted_ids, tile_expert, expert_offsets, slot_pos) of the MoE layout for topk_ids int [T, k] with entries
    in [0, E), in pure torch on the CPU (int32): the oracle of the GPU tests and what the executor's operand
    builders route with."""
    if topk_ids.dim() != 2:
        raise ValueError(f"moe_align_reference: topk_ids must be [T, k] (got {tuple(topk_ids.shape)})")
    T, k = topk_ids.shape
    ids = topk_ids.reshape(-1).to("cpu", torch.int64)
    n = T * k
    if n and not (0 <= int(ids.min()) and int(ids.max()) < E):
        raise ValueError(f"moe_align_reference: an expert id is outside [0, {E})")
    tiles = moe_max_tiles(T, k, E)
    counts = torch.bincount(ids, minlength=E)
    padded = (counts + MOE_BLOCK_M - 1) // MOE_BLOCK_M * MOE_BLOCK_M
    off = torch.zeros(E + 1, dtype=torch.int64)
    off[1:] = padded.cumsum(0)
    order = ids.sort(stable=True).indices                             # the slots by (expert, slot)
    first = counts.cumsum(0) - counts                                 # of each expert, in that order
    e_of = ids[order]
    pos = off[e_of] + torch.arange(n) - first[e_of]
    sorted_ids = torch.full((tiles * MOE_BLOCK_M,), n, dtype=torch.int64)
    sorted_ids[pos] = order
    slot_pos = torch.empty(n, dtype=torch.int64)
    slot_pos[order] = pos
    tile_expert = torch.full((tiles,), -1, dtype=torch.int64)
    tile_expert[:int(off[E]) // MOE_BLOCK_M] = torch.repeat_interleave(torch.arange(E), padded // MOE_BLOCK_M)
    return tuple(t.to(torch.int32) for t in (sorted_ids, tile_expert, off, slot_pos))


def _moe_vector(name: str, nm: str, t: Optional[torch.Tensor], shape: tuple, dtype: torch.dtype, device) -> torch.Tensor:
    """An int32 / fp32 operand of the MoE ops: made when None, else of exactly this dtype and shape, contiguous."""
    what = "int32" if dtype == torch.int32 else "fp32"
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if t.dtype != dtype:
        raise TypeError(f"{name} expects an {what} {nm} (got {t.dtype})")
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name}: {nm} must be contiguous of shape {tuple(shape)} (got {tuple(t.shape)})")
    return t


def _moe_route_sizes(name: str, T: int, E: int, top_k) -> None:
    if E < 8 or E > MOE_MAX_EXPERTS or E % 8:
        raise ValueError(f"{name}: E = {E} must be a multiple of 8 in [8, {MOE_MAX_EXPERTS}]")
    if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= min(MOE_MAX_TOP_K, E):
        raise ValueError(f"{name}: top_k = {top_k!r} must be an int in [1, min({MOE_MAX_TOP_K}, E)]")
    if T * top_k > MOE_MAX_SLOTS:
        raise ValueError(f"{name}: T * top_k = {T * top_k} is more than {MOE_MAX_SLOTS} slots")


def moe_route(logits: torch.Tensor, top_k: int, *, topk_ids: Optional[torch.Tensor] = None,
              topk_w: Optional[torch.Tensor] = None, sorted_ids: Optional[torch.Tensor] = None,
              tile_expert: Optional[torch.Tensor] = None, expert_offsets: Optional[torch.Tensor] = None,
              slot_pos: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None, check: bool = True):
    """MoE routing of T tokens over E experts from the router's logits bf16 [T, E] (E a multiple of 8 in [8, 256],
    1 <= top_k <= min(8, E), T * top_k <= 32768); returns (topk_ids, topk_w, sorted_ids, tile_expert, expert_offsets,
    slot_pos), each made when None.  topk_ids int32 [T, k]: the k largest logits by (value descending, index
    ascending); topk_w fp32 [T, k] = e_j / sum e with e_j = exp2((l_j - l_0) * 1.44269504f) in fp32 (softmax, then
    renormalised over the k).  The other four are the sorted, tile-aligned layout of the n = T * k slots
    (s = t * k + j) that moe_gemm and moe_combine take: sorted_ids int32 [64 * moe_max_tiles(T, k, E)] -- expert e
    owns rows [off[e], off[e + 1]), a multiple of 64, its slots first in ascending order, n elsewhere --, tile_expert
    int32 [moe_max_tiles] (-1: unused), expert_offsets int32 [E + 1] (off) and slot_pos int32 [n] (the inverse map).
    Every element of the six is written.  Nothing here depends on data, so there is nothing to check on the device:
    `check` is accepted for symmetry with the other ops and neither value ever syncs.  T == 0 reads nothing and
    writes the E + 1 zero offsets."""
    name = "moe_route"
    outs = (("topk_ids", topk_ids), ("topk_w", topk_w), ("sorted_ids", sorted_ids), ("tile_expert", tile_expert),
            ("expert_offsets", expert_offsets), ("slot_pos", slot_pos))
    _check_devices(name, logits, *(t for _, t in outs))
    if logits.dtype != torch.bfloat16:
        raise TypeError(f"{name} expects bf16 logits (got {logits.dtype})")
    if logits.dim() == 2:                                            # the E rule before the stride rules it implies
        _moe_route_sizes(name, logits.shape[0], logits.shape[1], top_k)
    ld = _bf16_rows(name, "logits", logits)
    T, E = logits.shape
    k, n, tiles, dev = top_k, T * top_k, moe_max_tiles(T, top_k, E), logits.device
    topk_ids = _moe_vector(name, "topk_ids", topk_ids, (T, k), torch.int32, dev)
    topk_w = _moe_vector(name, "topk_w", topk_w, (T, k), torch.float32, dev)
    sorted_ids = _moe_vector(name, "sorted_ids", sorted_ids, (tiles * MOE_BLOCK_M,), torch.int32, dev)
    tile_expert = _moe_vector(name, "tile_expert", tile_expert, (tiles,), torch.int32, dev)
    expert_offsets = _moe_vector(name, "expert_offsets", expert_offsets, (E + 1,), torch.int32, dev)
    slot_pos = _moe_vector(name, "slot_pos", slot_pos, (n,), torch.int32, dev)
    result = (topk_ids, topk_w, sorted_ids, tile_expert, expert_offsets, slot_pos)
    named = list(zip((nm for nm, _ in outs), result))
    for i, (nm, t) in enumerate(named):
        if _overlap(t, logits):
            raise ValueError(f"{name}: {nm} overlaps logits")
        for other, u in named[:i]:
            if _overlap(t, u):
                raise ValueError(f"{name}: {nm} overlaps {other}")
    h = _native.hip()
    with torch.cuda.device(dev):
        h.moe_route_bf16(logits.data_ptr(), topk_ids.data_ptr(), topk_w.data_ptr(), sorted_ids.data_ptr(),
                         tile_expert.data_ptr(), expert_offsets.data_ptr(), slot_pos.data_ptr(), T, E, k, ld,
                         _stream_ptr(stream, dev))
    return result


def moe_gemm(a: torch.Tensor, w: torch.Tensor, sorted_ids: torch.Tensor, tile_expert: torch.Tensor, n_slots: int, *,
             gather_div: int, out: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
             check: bool = True) -> torch.Tensor:
    """The grouped expert GEMM of an MoE MLP over the sorted layout of moe_route: for every row i of a used tile,
    out[i, :] = bf16(a[src(i), :] . w[tile_expert[i // 64]]^T) -- a bf16 [R, K], w bf16 [E, N, K], out bf16
    [P_max, N] (made when None), N and K multiples of 64, fp32 accumulation, no bias, no activation.
    gather_div = k >= 1: src(i) = sorted_ids[i] // k, the first projection reading token rows through the
    permutation; gather_div = 0: src(i) = i, the down projection reading the sorted intermediate in place.  A pad
    row (sorted_ids[i] >= n_slots) reads nothing of its own and is written as +0.0; the rows of unused tiles
    (tile_expert == -1) are neither read nor written -- a fresh `out` keeps whatever torch.empty gave them.
    check=True verifies on the device first (one sync): tile_expert within [-1, E), sorted_ids within [0, n_slots]
    and every source row of a used tile < R.  check=False never syncs: for callers that took the layout from
    moe_route, and under graph capture.  No used tile (or P_max == 0) writes nothing."""
    name = "moe_gemm"
    _check_devices(name, a, w, sorted_ids, tile_expert, out)
    if w.dtype != torch.bfloat16:
        raise TypeError(f"{name} expects bf16 tensors (w is {w.dtype})")
    if sorted_ids.dtype != torch.int32 or tile_expert.dtype != torch.int32:
        raise TypeError(f"{name} expects an int32 sorted_ids and tile_expert")
    lda = _bf16_rows(name, "a", a)
    R, K = a.shape
    if w.dim() != 3 or w.shape[2] != K:
        raise ValueError(f"{name}: w must be [E, N, K = {K}] (got {tuple(w.shape)})")
    E, N, _ = w.shape
    if E < 1 or E > MOE_MAX_EXPERTS:
        raise ValueError(f"{name}: E = {E} must be in [1, {MOE_MAX_EXPERTS}]")
    if N <= 0 or K <= 0 or N % 64 or K % 64:
        raise ValueError(f"{name}: N = {N} and K = {K} must be positive multiples of 64")
    if w.stride(2) != 1:
        raise ValueError(f"{name}: w must have K-contiguous rows")
    ldw, se = w.stride(1), (w.stride(0) if E > 1 else 0)
    if ldw < K or ldw % 8 or ldw >= 2 ** 31:
        raise ValueError(f"{name}: w row stride {ldw} must be >= {K}, a multiple of 8 and below 2^31")
    if se < 0 or se % 8:
        raise ValueError(f"{name}: w expert stride {se} must be a non-negative multiple of 8")
    if w.data_ptr() % 16:
        raise ValueError(f"{name}: w must be 16-byte aligned")
    if sorted_ids.dim() != 1 or tile_expert.dim() != 1 or not sorted_ids.is_contiguous() or not tile_expert.is_contiguous():
        raise ValueError(f"{name}: sorted_ids and tile_expert must be contiguous vectors")
    tiles = tile_expert.numel()
    if sorted_ids.numel() != tiles * MOE_BLOCK_M:
        raise ValueError(f"{name}: sorted_ids has {sorted_ids.numel()} rows, the {tiles} tiles of tile_expert need "
                         f"{tiles * MOE_BLOCK_M}")
    if isinstance(n_slots, bool) or not isinstance(n_slots, int) or not 0 <= n_slots <= MOE_MAX_SLOTS:
        raise ValueError(f"{name}: n_slots = {n_slots!r} must be an int in [0, {MOE_MAX_SLOTS}]")
    if isinstance(gather_div, bool) or not isinstance(gather_div, int) or not 0 <= gather_div <= MOE_MAX_TOP_K:
        raise ValueError(f"{name}: gather_div = {gather_div!r} must be 0 or the top-k, an int in [1, {MOE_MAX_TOP_K}]")
    P = tiles * MOE_BLOCK_M
    if out is None:
        out = torch.empty((P, N), dtype=torch.bfloat16, device=a.device)
    ldc = _bf16_rows(name, "out", out, N)
    if out.shape[0] != P:
        raise ValueError(f"{name}: out has {out.shape[0]} rows, the layout {P}")
    for nm, t in (("a", a), ("w", w), ("sorted_ids", sorted_ids), ("tile_expert", tile_expert)):
        if _overlap(out, t):
            raise ValueError(f"{name}: out overlaps {nm}")
    if tiles == 0:
        return out
    h = _native.hip()
    with torch.cuda.device(a.device):
        sp = _stream_ptr(stream, a.device)
        if check:
            with _launch_stream(stream, a.device):
                used = (tile_expert >= 0).repeat_interleave(MOE_BLOCK_M)
                valid = used & (sorted_ids >= 0) & (sorted_ids < n_slots)
                src = sorted_ids // gather_div if gather_div else torch.arange(P, dtype=torch.int32, device=a.device)
                bad = torch.stack([((tile_expert < -1) | (tile_expert >= E)).any(),
                                   ((sorted_ids < 0) | (sorted_ids > n_slots)).any(),
                                   (valid & (src >= R)).any()]).tolist()                      # the one sync
            if bad[0]:
                raise ValueError(f"{name}: a tile_expert entry is outside [-1, {E})")
            if bad[1]:
                raise ValueError(f"{name}: a sorted_ids entry is outside [0, {n_slots}]")
            if bad[2]:
                raise ValueError(f"{name}: a source row is past the {R} rows of a")
        h.moe_gemm_bf16(a.data_ptr(), w.data_ptr(), sorted_ids.data_ptr(), tile_expert.data_ptr(), out.data_ptr(), tiles,
                        n_slots, gather_div, N, K, lda, ldw, se, ldc, sp)
    return out


def moe_combine(y: torch.Tensor, slot_pos: torch.Tensor, topk_w: torch.Tensor, *, out: Optional[torch.Tensor] = None,
                stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """The weighted sum of each token's k expert outputs back in token order: out[t, :] = bf16(sum over
    j = 0 .. k - 1 of topk_w[t, j] * y[slot_pos[t * k + j], :]) -- y bf16 [P_max, D] in the sorted layout of moe_route,
    slot_pos int32 [T * k], topk_w fp32 [T, k] (1 <= k <= 8), out bf16 [T, D] (made when None), D a multiple of 8.
    In fp32, acc = 0.0f and acc = fmaf(w, y, acc) for j = 0 .. k - 1 in that order, then one rounding; nothing is
    skipped, so a NaN reaches exactly its own (t, column).  slot_pos is trusted (moe_route wrote it): every entry
    names a row of y.  T == 0 launches nothing; replaying a launch gives the same."""
    name = "moe_combine"
    _check_devices(name, y, slot_pos, topk_w, out)
    if topk_w.dtype != torch.float32:
        raise TypeError(f"{name} expects an fp32 topk_w (got {topk_w.dtype})")
    if slot_pos.dtype != torch.int32:
        raise TypeError(f"{name} expects an int32 slot_pos (got {slot_pos.dtype})")
    if y.dim() == 2 and y.dtype == torch.bfloat16 and (y.shape[1] <= 0 or y.shape[1] % 8):
        raise ValueError(f"{name}: D = {y.shape[1]} must be a positive multiple of 8")
    ld_y = _bf16_rows(name, "y", y)
    D = y.shape[1]
    if topk_w.dim() != 2 or not 1 <= topk_w.shape[1] <= MOE_MAX_TOP_K or not topk_w.is_contiguous():
        raise ValueError(f"{name}: topk_w must be contiguous [T, k] with 1 <= k <= {MOE_MAX_TOP_K} (got {tuple(topk_w.shape)})")
    T, k = topk_w.shape
    if slot_pos.dim() != 1 or slot_pos.numel() != T * k or not slot_pos.is_contiguous():
        raise ValueError(f"{name}: slot_pos must be a contiguous vector of length T * k = {T * k} (got {tuple(slot_pos.shape)})")
    if out is None:
        out = torch.empty((T, D), dtype=torch.bfloat16, device=y.device)
    ld_out = _bf16_rows(name, "out", out, D)
    if out.shape[0] != T:
        raise ValueError(f"{name}: out {tuple(out.shape)} does not match the {T} tokens of topk_w")
    for nm, t in (("y", y), ("slot_pos", slot_pos), ("topk_w", topk_w)):
        if _overlap(out, t):
            raise ValueError(f"{name}: out overlaps {nm}")
    if T == 0:
        return out
    h = _native.hip()
    with torch.cuda.device(y.device):
        h.moe_combine_bf16(y.data_ptr(), slot_pos.data_ptr(), topk_w.data_ptr(), out.data_ptr(), T, D, k, ld_y, ld_out,
                           _stream_ptr(stream, y.device))
    return out


def moe_workspace(T: int, E: int, top_k: int, D: int, F: int, device) -> dict:
    """The intermediates of moe_mlp for T tokens, E experts, top-k, hidden size D and expert width F, allocated once
    (a caller under graph capture passes them in: they must outlive the graph): the six outputs of moe_route, h13
    bf16 [P_max, 2F], act bf16 [P_max, F] and y bf16 [P_max, D].  h13 starts as zeros: the rows of unused tiles are
    never written by moe_gemm but are read by swiglu, whose output nothing then reads -- zeros keep that dead work
    finite."""
    _moe_route_sizes("moe_workspace", T, E, top_k)
    tiles = moe_max_tiles(T, top_k, E)
    P = tiles * MOE_BLOCK_M
    i32 = dict(dtype=torch.int32, device=device)
    bf = dict(dtype=torch.bfloat16, device=device)
    return {"topk_ids": torch.empty((T, top_k), **i32), "topk_w": torch.empty((T, top_k), dtype=torch.float32, device=device),
            "sorted_ids": torch.empty(P, **i32), "tile_expert": torch.empty(tiles, **i32),
            "expert_offsets": torch.empty(E + 1, **i32), "slot_pos": torch.empty(T * top_k, **i32),
            "h13": torch.zeros((P, 2 * F), **bf), "act": torch.empty((P, F), **bf), "y": torch.empty((P, D), **bf)}


def moe_mlp(x: torch.Tensor, router_logits: torch.Tensor, w13: torch.Tensor, w2: torch.Tensor, top_k: int, *,
            workspace: Optional[dict] = None, out: Optional[torch.Tensor] = None,
            stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """The MLP of a mixture-of-experts block: x bf16 [T, D], router_logits bf16 [T, E], w13 bf16 [E, 2F, D] (each
    expert's fused gate / up projection), w2 bf16 [E, D, F] (its down projection); returns out bf16 [T, D].  Five
    ops on one stream -- moe_route, moe_gemm gathered (gather_div = top_k) to h13 [P_max, 2F], swiglu to act
    [P_max, F], moe_gemm in place (gather_div = 0) to y [P_max, D], moe_combine -- with check=False throughout: it
    never syncs and can be captured in a graph.  workspace: moe_workspace(T, E, top_k, D, F, device), made on the
    launch stream when None.  The result is bit for bit that of the five calls made one by one."""
    name = "moe_mlp"
    dev = _check_devices(name, x, router_logits, w13, w2, out)
    for nm, t in (("x", x), ("router_logits", router_logits), ("w13", w13), ("w2", w2)):
        if t.dtype != torch.bfloat16:
            raise TypeError(f"{name} expects bf16 tensors ({nm} is {t.dtype})")
    if x.dim() != 2 or router_logits.dim() != 2 or w13.dim() != 3 or w2.dim() != 3:
        raise ValueError(f"{name} expects x [T, D], router_logits [T, E], w13 [E, 2F, D] and w2 [E, D, F]")
    (T, D), E, F = x.shape, router_logits.shape[1], w2.shape[2]
    if router_logits.shape[0] != T or tuple(w13.shape) != (E, 2 * F, D) or tuple(w2.shape) != (E, D, F):
        raise ValueError(f"{name}: x {tuple(x.shape)}, router_logits {tuple(router_logits.shape)}, w13 {tuple(w13.shape)} "
                         f"and w2 {tuple(w2.shape)} disagree on T, D, E or F")
    _moe_route_sizes(name, T, E, top_k)
    if workspace is None:
        with _launch_stream(stream, dev):
            workspace = moe_workspace(T, E, top_k, D, F, dev)
    ws = workspace
    _, topk_w, sorted_ids, tile_expert, _, slot_pos = moe_route(
        router_logits, top_k, topk_ids=ws["topk_ids"], topk_w=ws["topk_w"], sorted_ids=ws["sorted_ids"],
        tile_expert=ws["tile_expert"], expert_offsets=ws["expert_offsets"], slot_pos=ws["slot_pos"], stream=stream,
        check=False)
    n = T * top_k
    moe_gemm(x, w13, sorted_ids, tile_expert, n, gather_div=top_k, out=ws["h13"], stream=stream, check=False)
    swiglu(ws["h13"], out=ws["act"], stream=stream)
    moe_gemm(ws["act"], w2, sorted_ids, tile_expert, n, gather_div=0, out=ws["y"], stream=stream, check=False)
    return moe_combine(ws["y"], slot_pos, topk_w, out=out, stream=stream)


# ------------------------------------------------------------------------------------------------ MX operands
MX_BLOCK = 32                                             # elements of a row that share one scale byte
MX_FORMATS = ("fp8", "fp4")
_MX_EMAX = {"fp8": 8, "fp4": 2}                           # exponent of the largest finite magnitude: 448 = 1.75 * 2^8, 6 = 1.5 * 2^2
_MX_MANT = {"fp8": 3, "fp4": 1}                           # mantissa bits
_MX_EMIN = {"fp8": -6, "fp4": 0}                          # exponent of the smallest normal magnitude
_MX_MAX_CODE = {"fp8": 0x7E, "fp4": 0x7}                  # the code of the largest finite magnitude (0x7F is fp8's NaN)
_MX_SIGN_SHIFT = {"fp8": 7, "fp4": 3}
_FP4_MAGNITUDES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def _mx_fmt(name: str, fmt) -> str:
    if fmt not in MX_FORMATS:
        raise ValueError(f"{name}: fmt = {fmt!r} must be one of {MX_FORMATS}")
    return fmt


def _mx_code(fmt: str) -> int:
    """The native layer's code of a format: the MFMA's cbsz / blgp value (api.h kMxFp8 / kMxFp4)."""
    return 0 if fmt == "fp8" else 4


def mx_element_dtype(fmt: str) -> torch.dtype:
    return FP8 if _mx_fmt("mx_element_dtype", fmt) == "fp8" else torch.uint8


def mx_row_bytes(fmt: str, K: int) -> int:
    """Bytes (= array elements) of a row of K MX elements."""
    return K if _mx_fmt("mx_row_bytes", fmt) == "fp8" else K // 2


def quantize_mx_reference(x: torch.Tensor, fmt: str):
    """THE quantisation rule of the MX operands (the module docstring states the format) on the CPU, in integer torch
    ops only: x bf16 [T, D], D a multiple of 32 -> (q, scales) as quantize_mx gives them, bit for bit.  Per block of
    32: e = the largest exponent field (bits >> 7) & 0xFF; e == 255 gives scale byte 255 and element bytes 0x00;
    otherwise b = max(e - emax, 0) and an element is v * 2^(127 - b) rounded to the element format to nearest, ties to
    even, saturated at 448 / 6, the sign bit always carried.  The rounding is done on the 8-bit significand: with
    sig * 2^p the exact scaled magnitude, L = floor(log2) of it and the format's step 2^(max(L, emin) - M) at it,
    k = RNE(sig * 2^p / step) and the code is ((L - emin + 1) << M) + k - 2^M for L >= emin, else k -- a rounding
    carry walks into the exponent by itself -- capped at the code of the largest finite magnitude."""
    _mx_fmt("quantize_mx_reference", fmt)
    if x.dtype != torch.bfloat16 or x.dim() != 2 or x.shape[1] % MX_BLOCK or x.is_cuda:
        raise ValueError("quantize_mx_reference expects a CPU bf16 [T, D] tensor with D a multiple of 32")
    T, D = x.shape
    M, emin, emax = _MX_MANT[fmt], _MX_EMIN[fmt], _MX_EMAX[fmt]
    bits = x.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF
    sign, E, m = bits >> 15, (bits >> 7) & 0xFF, bits & 0x7F
    e = E.view(T, D // MX_BLOCK, MX_BLOCK).amax(dim=2)                  # [T, D / 32]
    nonfinite = e == 255
    b = torch.where(nonfinite, torch.full_like(e, 255), (e - emax).clamp(min=0))
    bb = b.clamp(max=253).repeat_interleave(MX_BLOCK, dim=1)            # per element
    sig = m + (E > 0).to(torch.int64) * 128                              # |v| = sig * 2^(max(E, 1) - 134)
    p = E.clamp(min=1) - 134 + 127 - bb                                  # scaled magnitude = sig * 2^p
    bitlen = sum((sig >= (1 << i)).to(torch.int64) for i in range(8))
    L = p + bitlen - 1                                                   # floor(log2), meaningless for sig == 0
    s = torch.maximum(L, torch.full_like(L, emin)) - M - p               # the step is 2^(p + s)
    down = s.clamp(min=1, max=16)                                        # s > 0: k = RNE(sig / 2^s); sig < 2^8
    k_down = (sig + (torch.ones_like(down) << (down - 1)) - 1 + ((sig >> down) & 1)) >> down
    k_up = sig << (-s).clamp(min=0, max=M)                               # s <= 0: exact
    k = torch.where(s > 0, k_down, k_up)
    code = torch.where(L >= emin, ((L - emin + 1) << M) + k - (1 << M), k)
    code = torch.where(sig == 0, torch.zeros_like(code), code).clamp(max=_MX_MAX_CODE[fmt])
    code = code | (sign << _MX_SIGN_SHIFT[fmt])
    code = torch.where(nonfinite.repeat_interleave(MX_BLOCK, dim=1), torch.zeros_like(code), code)
    if fmt == "fp8":
        q = code.to(torch.uint8).view(FP8)
    else:
        q = (code[:, 0::2] | (code[:, 1::2] << 4)).to(torch.uint8)
    return q, b.to(torch.uint8)


def dequantize_mx_reference(q: torch.Tensor, scales: torch.Tensor, fmt: str) -> torch.Tensor:
    """The values an MX operand (q, scales) stands for, float64 [rows, K], on the CPU: element * 2^(b - 127), a block
    with scale byte 255 all NaN.  Every finite result is exact in float64."""
    _mx_fmt("dequantize_mx_reference", fmt)
    if q.is_cuda or scales.is_cuda or q.dim() != 2 or scales.dim() != 2 or scales.dtype != torch.uint8:
        raise ValueError("dequantize_mx_reference expects CPU 2-D q and uint8 scales")
    if fmt == "fp8":
        if q.dtype not in (FP8, torch.uint8):
            raise ValueError("dequantize_mx_reference: fp8 elements are float8_e4m3fn (or their bytes as uint8)")
        el = (q.view(FP8) if q.dtype == torch.uint8 else q).to(torch.float32).to(torch.float64)
    else:
        if q.dtype != torch.uint8:
            raise ValueError("dequantize_mx_reference: fp4 elements are packed in uint8")
        lut = torch.tensor(_FP4_MAGNITUDES + tuple(-v for v in _FP4_MAGNITUDES), dtype=torch.float64)
        qi = q.to(torch.int64)
        el = torch.stack((lut[qi & 0xF], lut[qi >> 4]), dim=2).reshape(q.shape[0], 2 * q.shape[1])
    rows, K = el.shape
    if K % MX_BLOCK or tuple(scales.shape) != (rows, K // MX_BLOCK):
        raise ValueError(f"dequantize_mx_reference: scales {tuple(scales.shape)} do not match {rows} x {K} elements")
    b = scales.to(torch.int64)
    factor = torch.ldexp(torch.ones((), dtype=torch.float64), b - 127)
    factor = torch.where(b == 255, torch.full_like(factor, float("nan")), factor)
    return el * factor.repeat_interleave(MX_BLOCK, dim=1)


def _mx_rows(name: str, nm: str, t: torch.Tensor, dtype: torch.dtype, rows: Optional[int], cols: int,
             align: int) -> int:
    """The checks of a 2-D byte operand (MX elements or scales): dtype, [rows, cols], contiguous rows, a row stride
    >= cols and a multiple of `align` bytes, the first element `align`-byte aligned.  Returns the row stride."""
    if t.dtype != dtype:
        raise ValueError(f"{name}: {nm} must be {dtype} (got {t.dtype})")
    if t.dim() != 2 or t.shape[1] != cols or (rows is not None and t.shape[0] != rows):
        raise ValueError(f"{name}: {nm} must be [{'rows' if rows is None else rows}, {cols}] (got {tuple(t.shape)})")
    n = t.shape[0]
    if cols > 1 and t.stride(1) != 1:
        raise ValueError(f"{name}: {nm} must have contiguous rows")
    if n > 1 and (t.stride(0) < cols or t.stride(0) % align):
        raise ValueError(f"{name}: {nm} row stride {t.stride(0)} must be >= {cols}"
                         + (f" and a multiple of {align}" if align > 1 else ""))
    if t.data_ptr() % align:
        raise ValueError(f"{name}: {nm} must be {align}-byte aligned")
    return _row_stride(t, n, cols)


def quantize_mx(x: torch.Tensor, fmt: str, *, out: Optional[torch.Tensor] = None,
                scales: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None):
    """x bf16 [T, D], D a multiple of 32 -> (q, scales) in the MX format `fmt` ("fp8" or "fp4"; the module docstring
    states format and rule; quantize_mx_reference is the same rule on the CPU, bit for bit).  q (`out`) is
    float8_e4m3fn [T, D] or uint8 [T, D / 2], scales uint8 [T, D / 32]; both are made when None, may be row-strided
    views (any row stride >= the row; 8-byte / 4-byte aligned q rows get one store per lane, others byte stores) and
    have every byte of their windows written.  x follows add_rmsnorm's row rules.  No operand may overlap another.
    Nothing here reads device data: the launch can be captured into a graph, and replays give the same bytes.
    T == 0 launches nothing."""
    name = "quantize_mx"
    _mx_fmt(name, fmt)
    _check_devices(name, x, out, scales)
    if x.dim() == 2 and (x.shape[1] < MX_BLOCK or x.shape[1] % MX_BLOCK):
        raise ValueError(f"{name}: D = {x.shape[1]} must be a positive multiple of {MX_BLOCK}")
    if x.dtype != torch.bfloat16:
        raise ValueError(f"{name}: x must be bf16 (got {x.dtype})")
    ld_x = _bf16_rows(name, "x", x)
    T, D = x.shape
    if T * (D // 8) >= 2 ** 31 * 1024:
        raise ValueError(f"{name}: more than 2^31 - 1 workgroups")
    if out is None:
        out = torch.empty((T, mx_row_bytes(fmt, D)), dtype=mx_element_dtype(fmt), device=x.device)
    if scales is None:
        scales = torch.empty((T, D // MX_BLOCK), dtype=torch.uint8, device=x.device)
    ld_q = _mx_rows(name, "out", out, mx_element_dtype(fmt), T, mx_row_bytes(fmt, D), 1)
    ld_s = _mx_rows(name, "scales", scales, torch.uint8, T, D // MX_BLOCK, 1)
    for (na, ta), (nb, tb) in ((("out", out), ("x", x)), (("scales", scales), ("x", x)), (("out", out), ("scales", scales))):
        if _overlap(ta, tb):
            raise ValueError(f"{name}: {na} overlaps {nb}")
    if T == 0:
        return out, scales
    h = _native.hip()
    with torch.cuda.device(x.device):
        h.quantize_mx_bf16(x.data_ptr(), out.data_ptr(), scales.data_ptr(), T, D, ld_x, ld_q, ld_s, _mx_code(fmt),
                           _stream_ptr(stream, x.device))
    return out, scales


def gemm_mx(a_q: torch.Tensor, a_scales: torch.Tensor, w_q: torch.Tensor, w_scales: torch.Tensor, a_fmt: str, *,
            out: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None, relu: bool = False,
            stream: Optional[torch.cuda.Stream] = None, cu_budget: int = 0) -> torch.Tensor:
    """out[M, N] = act(A[M, K] @ W[N, K]^T + bias[N]) -- both operands MX (elements, scales) pairs (the module
    docstring states the format): W always "fp4" (w_q uint8 [N, K / 2]), A of format a_fmt: "fp8" (a_q float8_e4m3fn
    [M, K]) or "fp4" (a_q uint8 [M, K / 2]); scales uint8 [rows, K / 32].  fp32 accumulate on the block-scaled MFMA,
    bf16 out.  M, N multiples of 64, K of 128.  Element rows are 16-byte aligned (row stride a multiple of 16, the
    first element 16-byte aligned); scale rows may have any row stride >= K / 32; out, bias, relu and cu_budget as
    gemm_fp8.  out may not overlap an operand.  Scale byte 255 and scale byte 0 under non-zero elements are outside
    the contract; a block of zero elements with scale byte 0 contributes exactly 0.  Nothing here reads device data:
    the launch can be captured into a graph."""
    name = "gemm_mx"
    _mx_fmt(name, a_fmt)
    _check_devices(name, a_q, a_scales, w_q, w_scales, out, bias)
    if a_q.dim() != 2 or w_q.dim() != 2:
        raise ValueError(f"{name}: a_q and w_q must be 2-D (got {tuple(a_q.shape)} and {tuple(w_q.shape)})")
    M, N, K = a_q.shape[0], w_q.shape[0], 2 * w_q.shape[1]
    check_gemm_shapes(M, N, K, 128, name)
    lda = _mx_rows(name, "a_q", a_q, mx_element_dtype(a_fmt), M, mx_row_bytes(a_fmt, K), 16)
    ldw = _mx_rows(name, "w_q", w_q, torch.uint8, N, K // 2, 16)
    ld_as = _mx_rows(name, "a_scales", a_scales, torch.uint8, M, K // MX_BLOCK, 1)
    ld_ws = _mx_rows(name, "w_scales", w_scales, torch.uint8, N, K // MX_BLOCK, 1)
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=a_q.device)
    if (out.dim() != 2 or tuple(out.shape) != (M, N) or out.dtype != torch.bfloat16 or out.stride(1) != 1
            or out.stride(0) < N or out.stride(0) % 4 or out.data_ptr() % 8):
        raise ValueError(f"{name}: out must be bf16 [{M}, {N}] with contiguous, 8-byte aligned rows")
    bptr = 0
    if bias is not None:
        if bias.dtype != torch.float32 or bias.dim() != 1 or bias.numel() != N or not bias.is_contiguous() \
                or bias.data_ptr() % 16:
            raise ValueError(f"{name}: bias must be a contiguous, 16-byte aligned fp32 vector of length N = {N}")
        bptr = bias.data_ptr()
    for nm, t in (("a_q", a_q), ("a_scales", a_scales), ("w_q", w_q), ("w_scales", w_scales), ("bias", bias)):
        if t is not None and _overlap(out, t):
            raise ValueError(f"{name}: out overlaps {nm}")
    h = _native.hip()
    with torch.cuda.device(a_q.device):
        h.gemm_mx_nt(a_q.data_ptr(), a_scales.data_ptr(), w_q.data_ptr(), w_scales.data_ptr(), out.data_ptr(), bptr,
                     M, N, K, lda, ld_as, ldw, ld_ws, out.stride(0), _mx_code(a_fmt), bool(relu),
                     _stream_ptr(stream, a_q.device), cu_budget)
    return out


# ------------------------------------------------------------------------------------------------ FP8 KV cache
def quantize_kv8_reference(z: torch.Tensor) -> torch.Tensor:
    """THE quantisation rule of the FP8 KV cache (native/hip/api.h) on the CPU, in integer torch ops on the fp32
    bits: z fp32, any shape -> uint8 e4m3fn codes of the same shape, bit for bit what rope_append stores for
    z = value / scale.  A NaN gives 0x7F | sign << 7; otherwise the magnitude is rounded to the nearest e4m3fn value,
    ties to even (step 2^-9 below 2^-6), whatever rounds above 448, +-Inf included, saturates to 0x7E; the sign bit
    is always carried (-0.0 and a negative value that rounds to zero give 0x80).  With mag the 31 magnitude bits and
    e = mag >> 23: for e >= 121 (|z| >= 2^-6) the code is RNE(mag / 2^20) - (120 << 3) -- the rounding carry walks
    into the exponent by itself --, below that RNE(significand / 2^(141 - e)) in units of 2^-9."""
    if z.dtype != torch.float32 or z.is_cuda:
        raise ValueError("quantize_kv8_reference expects a CPU fp32 tensor")
    bits = z.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    sign, mag = bits >> 31, bits & 0x7FFFFFFF
    e = mag >> 23

    def rne(x, s):                                                         # round(x / 2^s) to nearest even, s >= 1
        return (x + (torch.ones_like(s) << (s - 1)) - 1 + ((x >> s) & 1)) >> s
    normal = rne(mag, torch.full_like(mag, 20)) - (120 << 3)
    sig = (mag & 0x7FFFFF) | ((e > 0).to(torch.int64) << 23)              # |z| = sig * 2^(max(e, 1) - 150)
    sub = rne(sig, (141 - e.clamp(min=1)).clamp(min=1, max=40))           # below 2^-10: 0
    code = torch.where(e >= 121, normal, sub).clamp(max=0x7E)
    code = torch.where(mag > 0x7F800000, torch.full_like(code, 0x7F), code)
    return (code | (sign << 7)).to(torch.uint8)


def dequantize_kv8_reference(codes: torch.Tensor, scale) -> torch.Tensor:
    """The values the bytes of an FP8 KV cache stand for, float64 on the CPU: e4m3fn(c) * scale, both exact in
    float64 (0x7F and 0xFF are NaN).  codes: uint8 or float8_e4m3fn, any shape; scale: a float, or a tensor that
    broadcasts against codes (one scale per KV head: scale.view(1, Hkv, 1, 1) for a cache)."""
    if codes.is_cuda or codes.dtype not in (FP8, torch.uint8):
        raise ValueError("dequantize_kv8_reference expects CPU float8_e4m3fn codes (or their bytes as uint8)")
    el = (codes.view(FP8) if codes.dtype == torch.uint8 else codes).to(torch.float32).to(torch.float64)
    return el * (scale.to(torch.float64) if isinstance(scale, torch.Tensor) else float(scale))


def rope_append_kv8_reference(qkv: torch.Tensor, cos_sin: torch.Tensor, ctx_lens: torch.Tensor, q_start: torch.Tensor,
                              k_scale: torch.Tensor, v_scale: torch.Tensor):
    """(k_codes, v_codes) uint8 [Tq, Hkv, 128]: the cache bytes rope_append writes for every row of qkv (bf16
    [Tq, Hq + 2 Hkv, 128], CPU) that belongs to a chunk -- zeros elsewhere.  The rotation is computed in float64
    (y[i] = x1 c - x2 s, y[i + 64] = x2 c + x1 s at the row's position ctx - q_len + i) and cast to fp32 once,
    then z = y / k_scale[g] and z = float(v) / v_scale[g] are fp32 divisions and quantize_kv8_reference gives the
    bytes.  Where the float64 rotation is exact in fp32 (the exact regimes of the tests) that is bit for bit the
    kernel's result; otherwise the kernel's fp32 FMA may land one ulp away, and a near-tie one e4m3 step."""
    Hkv = k_scale.numel()
    Tq, Ht, D = qkv.shape
    Hq, half = Ht - 2 * Hkv, ATTN_HEAD_DIM // 2
    k64 = torch.zeros(Tq, Hkv, D, dtype=torch.float64)
    live = torch.zeros(Tq, dtype=torch.bool)
    starts = q_start.tolist()
    for s, ctx in enumerate(ctx_lens.tolist()):
        r0, r1 = starts[s], starts[s + 1]
        if r1 <= r0:
            continue
        cs = cos_sin[ctx - (r1 - r0) + torch.arange(r1 - r0)].double()[:, None, :]
        x = qkv[r0:r1, Hq:Hq + Hkv].double()
        x1, x2, c, sn = x[..., :half], x[..., half:], cs[..., :half], cs[..., half:]
        k64[r0:r1] = torch.cat([x1 * c - x2 * sn, x2 * c + x1 * sn], dim=-1)
        live[r0:r1] = True
    kz = k64.float() / k_scale.float().view(1, Hkv, 1)
    vz = qkv[:, Hq + Hkv:].float() / v_scale.float().view(1, Hkv, 1)
    keep = live.view(Tq, 1, 1)
    return (torch.where(keep, quantize_kv8_reference(kz), torch.zeros((), dtype=torch.uint8)),
            torch.where(keep, quantize_kv8_reference(vz), torch.zeros((), dtype=torch.uint8)))


def gemm_flops(M: int, N: int, K: int) -> float:
    return 2.0 * M * N * K
