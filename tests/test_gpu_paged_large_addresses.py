"""The four paged-KV kernels -- decode, split decode and prefill attention, rope_append -- on addresses
past 4 GiB (run with `-m gpu` on an MI355X): a cache of NB = 262144 + 128 blocks (two KV heads: a block of
one cache is 16 KiB, K and V are 4 GiB each), and q / out / qkv / q_out rows 2^28 + 8 elements apart.
The kernels' headers say "all addresses are 64-bit"; nothing else in the suite holds them to it.  The
operands, references and guards are those of test_gpu_decode_attn_exact.py, test_gpu_prefill_attn_exact.py
and test_gpu_rope_append_exact.py; every comparison is exact.

The big caches are never built on the host.  A launch's logical caches and block table are built on
the CPU over COMPACT = 128 compact ids (the builders' table re-dealt by `spread`, the rest spares), the
expectation is computed there with the float64 references, and compact id c becomes the physical id
c (c < 64) or c + NB - 128 >= 262144 + 64 (a high block: element offset >= 2^31, byte offset >= 2^32).  The compact
blocks are scattered into device caches at those ids.

  * `spread` deals the entries of a row to low and high ids by the parity of j // 4 + j + s (entry j
    of sequence s): consecutive entries (the prefill walk, the chunk of an append) and entries four
    apart (a decode wave's next block) alternate between the two ends of the cache, three times in
    four and always, so the next-block prefetch crosses the 4 GiB line in both directions.  Every row with
    two blocks or more holds ids of both ends (asserted by assert_rows_mix; the decode contexts all have two,
    SEQS_A and SEQS_C also hold one-block sequences, which lie on either side);
  * decoys turn a wrap into a wrong value, not a fault: a 32-bit byte offset (or an element offset
    taken mod 2^31) sends high block b to block b - 262144 -- and NB was chosen so that this is the
    physical block c of its compact id, inside [64, 128): no table entry names it.  For the readers it
    holds 1 - x (K) and 1/128 - x (V) of the block's x (0 for its NaNs): finite, different in every
    cell; for the writer SENT16 like every other cell;
  * every other unnamed block holds NaN (readers) or SENT16 (writer), filled on the device;
  * after rope_append the 128 compact blocks, fetched back by physical id, equal the compact expectation
    bit for bit, and a device-side count of the cells that differ from SENT16 over the whole of both
    caches (in pieces of 1 GiB) equals that of the expectation: nothing else was written, decoys included.

The row-offset tests use small caches and 10 rows ROW_LD = 2^28 + 8 elements apart in allocations of
5 GiB: rows 8 and 9 start past 2^32 bytes.  Only the touched rows of the inputs are initialised; the
outputs are SENT16 everywhere before the launch and compared in full on the device afterwards.

The builders and what they claim to cover are CPU-tested in test_paged_large_addresses_cpu.py.
"""
import functools

import pytest
import torch

import test_gpu_decode_attn_exact as ATT
import test_gpu_prefill_attn_exact as PRE
import test_gpu_rope_append_exact as ROPE
from test_gpu_kernels_exact import NAN, SENT16, SENT32, guarded_input, guarded_output, guards_intact

pytestmark = pytest.mark.gpu

# MEASURED on an MI355X (printed by the tests):
MEASURED = """
  All 7 tests ran (none skipped) and passed; the module takes 0.1 s inside the whole suite (2.0 s in a run where
  the allocator had to fetch the 5 GiB buffers anew, 3 s alone including the first use of the device).  A fill of
  4 GiB is about a millisecond; no test compares or copies more than the 128 compact blocks and the rows.
  With the slab offset of one kernel taken mod 2^31 elements (a 32-bit byte offset; such a read or write lands on
  the decoy and stays inside the allocation) the kernel's test fails and no other: decode and split decode "7406
  elements differ, first at row 0, head 0, d 0: got 0.203125, expected 0.0234375", prefill "90703 elements differ",
  rope_append "('k_cache', 74240, [67, 0, 0, 0])" -- compact block 67, a high block, still SENT16.
"""

D, T, C0, R0 = ATT.D, ATT.T, ATT.C0, PRE.R0
HKV, GROUP = 2, 4
HQ = HKV * GROUP
BLOCK_ELEMS = HKV * T * D               # elements of a block of one cache: 8192, 16 KiB
HIGH = 262144                           # the first block id at element offset 2^31, byte offset 2^32
COMPACT = 128
HALF_IDS = COMPACT // 2                 # compact ids below it stay where they are
NB = HIGH + COMPACT
PIECE = 1 << 29                         # int16 cells per device-side reduction: 1 GiB
CTX_DECODE = (257, 33, 64, 290, 129, 65, 97, 200)          # every sequence has two blocks or more; two have 9 and 10
ROW_LD = (1 << 28) + 8                  # elements between rows of the strided q / out / qkv / q_out
ROWS = 10
READER_NEED = 10 << 30                  # bytes of free device memory: two caches of 4 GiB and slack
WRITER_NEED = 10 << 30                  # ... and a 512 MiB mask per piece of the count
ROW_NEED = 12 << 30                     # two allocations of 5 GiB and slack


# ------------------------------------------------------------------------------------------------
# compact ids, physical ids, decoys (CPU-tested in test_paged_large_addresses_cpu.py)
# ------------------------------------------------------------------------------------------------
def spread(table, g):
    """The builders' table with its named entries dealt new, distinct compact ids of [0, 128): entry j
    of row s gets a low id (< 64) where j // 4 + j + s is even, else a high one; each pool is a random
    permutation.  SENT32 entries stay."""
    low = torch.randperm(HALF_IDS, generator=g).tolist()
    high = (HALF_IDS + torch.randperm(HALF_IDS, generator=g)).tolist()
    out = table.clone()
    for s in range(table.shape[0]):
        for j in range(table.shape[1]):
            if int(table[s, j]) != SENT32:
                out[s, j] = (low if (j // 4 + j + s) % 2 == 0 else high).pop()
    named = out[out != SENT32]
    assert named.numel() == named.unique().numel() and int(named.max()) < COMPACT
    return out


def physical(ids):
    """Compact ids (a tensor; SENT32 entries stay) to physical block ids."""
    return torch.where((ids == SENT32) | (ids < HALF_IDS), ids, ids + (NB - COMPACT))


def assert_beyond_4_gib():
    first_high = int(physical(torch.tensor([HALF_IDS]))[0])
    assert first_high == HIGH + HALF_IDS and int(physical(torch.tensor([COMPACT - 1]))[0]) == NB - 1
    assert HIGH * BLOCK_ELEMS == 1 << 31 and HIGH * BLOCK_ELEMS * 2 == 1 << 32           # every id >= HIGH lies past them
    assert first_high * BLOCK_ELEMS >= 1 << 31 and first_high * BLOCK_ELEMS * 2 >= 1 << 32
    assert (HIGH - 1) * BLOCK_ELEMS * 2 < 1 << 32 and BLOCK_ELEMS * 2 == 16 << 10
    assert NB * BLOCK_ELEMS * 2 < 5 << 30                                       # a cache is 4 GiB and 2 MiB


def assert_rows_mix(table, first, last, stride4):
    """On a compact table: every row whose entries [first[s], last[s]] are two or more holds low and
    high ids there; over the launch consecutive entries cross in both directions, and with stride4
    so do entries four apart (a decode wave's next block) inside one row."""
    low = lambda s, j: int(table[s, j]) < HALF_IDS                              # noqa: E731
    steps = {1: set(), 4: set()}
    for s in range(table.shape[0]):
        js = list(range(first[s], last[s] + 1))
        if len(js) >= 2:
            assert {low(s, j) for j in js} == {True, False}, ("a row on one side of 4 GiB", s)
        for d in steps:
            steps[d] |= {(low(s, j), low(s, j + d)) for j in js if j + d <= last[s]}
    assert {(True, False), (False, True)} <= steps[1]
    if stride4:
        assert {(True, False), (False, True)} <= steps[4]
        assert any(last[s] - first[s] >= 8 and low(s, first[s]) != low(s, first[s] + 4) != low(s, first[s] + 8)
                   for s in range(table.shape[0]))                              # one wave, three blocks, two crossings


def decoys_of(kc, vc):
    """(K, V) [64, Hkv, ...] bf16: what the blocks a 32-bit wrap of the high blocks' offsets lands on
    hold for the readers -- finite, and different from the high block in every cell."""
    hk, hv = kc[HALF_IDS:].float().nan_to_num(0.0), vc[HALF_IDS:].float().nan_to_num(0.0)
    dk, dv = (1 - hk).to(torch.bfloat16), (2.0 ** -7 - hv).to(torch.bfloat16)
    for d, h in ((dk, kc[HALF_IDS:]), (dv, vc[HALF_IDS:])):
        assert bool(d.float().isfinite().all()) and bool((d.float() != h.float()).all())
    return dk, dv


def assert_decoys_unnamed(table):
    """The block a wrap sends high block b to, b - 262144, is the physical block of no table entry."""
    named = physical(table[table != SENT32])
    high = named[named >= HIGH]
    assert high.numel() and bool((named < HIGH).any())
    assert not set((high - HIGH).tolist()) & set(named.tolist())
    assert bool(((high - HIGH >= HALF_IDS) & (high - HIGH < COMPACT)).all())


class ReaderCase:
    """CPU side of a decode (seqs: context lengths, pair regime) or prefill (seqs: (ctx, q_len), match
    regime) launch over the compact ids, with the exact expectation of the exact modules."""

    def __init__(self, seqs, seed):
        g = torch.Generator().manual_seed(seed)
        self.decode = not isinstance(seqs[0], tuple)
        self.ctxs = tuple(seqs) if self.decode else tuple(c for c, _ in seqs)
        self.seqs, self.S = seqs, len(seqs)
        need = [-(-c // T) for c in self.ctxs]
        builder, nb = (ATT if self.decode else PRE).block_tables(self.ctxs, g)
        assert nb <= COMPACT
        self.table = spread(builder, g)
        if self.decode:
            q, ks, vs = ATT.logical_operands("pair", GROUP, HKV, self.ctxs, g)
            self.q_start = None
        else:
            q, ks, vs = PRE.logical_operands("match", GROUP, HKV, seqs, g)
            self.q_start = torch.tensor([0] + [n for _, n in seqs]).cumsum(0).to(torch.int32)
            self.max_q_len = max(n for _, n in seqs)
        self.kc, self.vc = ATT.paged_caches(ks, vs, self.table, COMPACT, HKV)
        self.ctx = torch.tensor(self.ctxs, dtype=torch.int32)
        self.qb = q.to(torch.bfloat16)
        assert torch.equal(self.qb.float(), q)
        self.ref = self.reference(self.kc, self.vc)
        if self.decode:
            big = self.ref.abs() > 2.0 ** -20
            f = self.ref.float()
            assert torch.equal(f.double()[big], self.ref[big]) and bool(((f.view(torch.int32) & 0xFFFF) == 0x8000).any())
        else:
            exact, _ = PRE.exact_expectation("match", GROUP, HKV, seqs, vs)
            f = exact.float()
            assert torch.equal(f.double(), exact) and torch.equal(self.ref.float().to(torch.bfloat16), f.to(torch.bfloat16))
        self.exp = f.to(torch.bfloat16)
        # what the table must cover
        assert_beyond_4_gib()
        assert_rows_mix(self.table, [0] * self.S, [n - 1 for n in need], stride4=self.decode)
        assert_decoys_unnamed(self.table)
        self.decoy_k, self.decoy_v = decoys_of(self.kc, self.vc)
        if self.decode:
            assert max(need) >= 9 and min(need) >= 2

    def reference(self, kc, vc):
        if self.decode:
            return ATT.reference(self.qb, kc, vc, self.table, self.ctx)
        return PRE.reference(self.qb, kc, vc, self.table, self.ctx, self.q_start)

    def wrapped_caches(self):
        """The compact caches as a kernel whose slab offsets wrap at 4 GiB sees them: every high block
        replaced by its decoy."""
        kc, vc = self.kc.clone(), self.vc.clone()
        kc[HALF_IDS:], vc[HALF_IDS:] = self.decoy_k, self.decoy_v
        return kc, vc


@functools.lru_cache(maxsize=None)
def decode_case():
    return ReaderCase(CTX_DECODE, seed=9100)


@functools.lru_cache(maxsize=None)
def prefill_case():
    return ReaderCase(PRE.SEQS_A, seed=9200)


class WriterCase:
    """CPU side of a rope_append launch of SEQS_C in the dyadic regime over the compact ids: the
    operands as the rope module's Case builds them, the expected q_out and the expected compact
    caches (SENT16 outside the chunks' slots)."""

    def __init__(self, seqs, seed, regime="dyadic"):
        g = torch.Generator().manual_seed(seed)
        self.seqs, self.S = seqs, len(seqs)
        self.Ht = HQ + 2 * HKV
        ctxs = tuple(c for c, _ in seqs)
        self.n = sum(n for _, n in seqs)
        self.max_q_len = max(n for _, n in seqs)
        builder, nb = PRE.block_tables(ctxs, g)
        assert nb <= COMPACT
        self.table = spread(builder, g)
        max_pos = max(257, max(ctxs))
        x, v_bits, self.cs = ROPE.logical_operands(regime, self.n, self.Ht, HKV, max_pos, g)
        self.qkv = x.to(torch.bfloat16)
        assert torch.equal(self.qkv.float(), x)
        ROPE.bits(self.qkv)[:, HQ + HKV:] = v_bits
        self.ctx = torch.tensor(ctxs, dtype=torch.int32)
        self.q_start = torch.tensor([0] + [n for _, n in seqs]).cumsum(0).to(torch.int32)
        ref_q, ref_k, pos, seq = ROPE.reference(self.qkv, self.cs, self.ctx, self.q_start, HKV)
        for r in (ref_q, ref_k):
            assert bool(r.isfinite().all()) and torch.equal(r.float().double(), r)           # exact in fp32
        self.exp_q = ref_q.float().to(torch.bfloat16)
        self.exp_kc, self.exp_vc, _, _ = ROPE.expected_caches(COMPACT, HKV, ROPE.bits(ref_k.float().to(torch.bfloat16)),
                                                              v_bits, pos, seq, self.table)
        self.owned = self.n * HKV * D                                                        # cells per cache the chunks own
        self.first = [(c - n) // T if n else 0 for c, n in seqs]
        self.last = [(c - 1) // T if n else -1 for c, n in seqs]
        assert_beyond_4_gib()
        assert_rows_mix(self.table, self.first, self.last, stride4=False)
        assert_decoys_unnamed(self.table)
        assert max(b - a + 1 for a, b in zip(self.first, self.last)) >= 9
        touched = [int(self.table[s, j]) for s in range(self.S) for j in range(self.first[s], self.last[s] + 1)]
        assert any(c < HALF_IDS for c in touched) and sum(c >= HALF_IDS for c in touched) >= 9
        # the decoys of the touched high blocks hold SENT16 in the expectation, like every unnamed block
        assert bool((self.exp_kc[HALF_IDS:].flatten(1) != SENT16).any(1).sum() >= 9)

    def cells(self):
        """Cells per cache that differ from SENT16 in the expectation: all the chunks own, less the few
        of V's random bit patterns that are SENT16 themselves."""
        k, v = int((self.exp_kc != SENT16).sum()), int((self.exp_vc != SENT16).sum())
        assert self.owned - 64 <= v <= self.owned and self.owned - 64 <= k <= self.owned
        return k, v


@functools.lru_cache(maxsize=None)
def writer_case():
    return WriterCase(ROPE.SEQS_C, seed=9300)


# ------------------------------------------------------------------------------------------------
# device side
# ------------------------------------------------------------------------------------------------
def need_free(need, what):
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"{what} needs {need >> 30} GiB of free device memory ({free >> 30} GiB free)")


def big_cache(shape_tail, fill_bits):
    """An int16 [NB, Hkv, *shape_tail] cache filled on the device, as bf16."""
    c = torch.empty((NB, HKV) + shape_tail, dtype=torch.int16, device="cuda")
    c.fill_(fill_bits)
    return c.view(torch.bfloat16)


NAN_BITS = int(torch.tensor([NAN]).to(torch.bfloat16).view(torch.int16)[0])


def reader_caches(c):
    """The 4 GiB K and V of a ReaderCase: NaN, the compact blocks at their physical ids, the decoys."""
    kc, vc = big_cache((T, D), NAN_BITS), big_cache((D, T), NAN_BITS)
    ids = physical(torch.arange(COMPACT)).cuda()
    kc[ids], vc[ids] = c.kc.cuda(), c.vc.cuda()
    kc[HALF_IDS:COMPACT], vc[HALF_IDS:COMPACT] = c.decoy_k.cuda(), c.decoy_v.cuda()
    assert kc.numel() * 2 > 1 << 32 and bool(kc[NB - COMPACT - 1].float().isnan().all())
    return kc, vc


def count_not_sentinel(t):
    """Cells of an int16 view of t that differ from SENT16, reduced in pieces of 1 GiB."""
    flat = t.view(torch.int16).flatten()
    return sum(int(torch.count_nonzero(flat[i:i + PIECE] != SENT16)) for i in range(0, flat.numel(), PIECE))


def run_reader(c, kv_splits=1):
    from k8s_gpu_scheduler_amd.ops import loadgen
    need_free(READER_NEED, "a paged attention over two caches of 4 GiB")
    kc = vc = None
    try:
        kc, vc = reader_caches(c)
        rows = c.qb.shape[0]
        W = HQ * D
        q = guarded_input(c.qb.view(rows, W).cuda(), W + C0, c0=C0).unflatten(1, (HQ, D))
        raw, out2d = guarded_output(rows, W, W + C0, C0, "cuda")
        out = out2d.unflatten(1, (HQ, D))
        _, table = ATT.guarded_ints_2d(physical(c.table), c.table.shape[1] + 2)
        _, ctx = PRE.guarded_ints(c.ctx)
        if c.decode:
            kw = {}
            if kv_splits > 1:
                kw = dict(kv_splits=kv_splits, workspace=torch.full(
                    (loadgen.decode_split_workspace_floats(c.S, HQ, kv_splits),), NAN, device="cuda"))
            loadgen.paged_decode_attention(q, kc, vc, table, ctx, out=out, **kw)
        else:
            _, q_start = PRE.guarded_ints(c.q_start)
            loadgen.paged_prefill_attention(q, kc, vc, table, ctx, q_start, out=out)
        torch.cuda.synchronize()
        assert guards_intact(raw, (slice(R0, R0 + rows), slice(C0, C0 + W)), SENT16), "write outside the window"
        got, exp = out.cpu(), c.exp
        if not torch.equal(got, exp):
            bad = (got.float() != exp.float()).nonzero()
            r, h, d = bad[0].tolist()
            raise AssertionError(f"{len(bad)} elements differ, first at row {r}, head {h}, d {d}: got {got[r, h, d].item()}, "
                                 f"expected {exp[r, h, d].item()}")
    finally:
        del kc, vc
        torch.cuda.empty_cache()


def test_decode_attention_over_a_cache_beyond_4_gib():
    run_reader(decode_case())


def test_split_decode_attention_over_a_cache_beyond_4_gib():
    run_reader(decode_case(), kv_splits=4)


def test_prefill_attention_over_a_cache_beyond_4_gib():
    run_reader(prefill_case())


def test_rope_append_into_a_cache_beyond_4_gib():
    from k8s_gpu_scheduler_amd.ops import loadgen
    c = writer_case()
    need_free(WRITER_NEED, "rope_append into two caches of 4 GiB")
    kc = vc = None
    try:
        kc, vc = big_cache((T, D), SENT16), big_cache((D, T), SENT16)
        W = c.Ht * D
        qkv = guarded_input(c.qkv.view(c.n, W).cuda(), W + C0, c0=C0).unflatten(1, (c.Ht, D))
        raw, out2d = guarded_output(c.n, HQ * D, HQ * D + C0, C0, "cuda")
        q_out = out2d.unflatten(1, (HQ, D))
        _, table = ATT.guarded_ints_2d(physical(c.table), c.table.shape[1] + 2)
        _, ctx = PRE.guarded_ints(c.ctx)
        _, q_start = PRE.guarded_ints(c.q_start)
        loadgen.rope_append(qkv, guarded_input(c.cs.cuda(), D, c0=0), kc, vc, table, ctx, q_start, q_out=q_out)
        torch.cuda.synchronize()
        assert guards_intact(raw, (slice(R0, R0 + c.n), slice(C0, C0 + HQ * D)), SENT16), "write outside q_out's rows"
        assert torch.equal(q_out.cpu(), c.exp_q)
        ids = physical(torch.arange(COMPACT)).cuda()
        got_kc, got_vc = ROPE.bits(kc[ids]).cpu(), ROPE.bits(vc[ids]).cpu()
        same = ROPE.unsigned_zero(got_kc) == ROPE.unsigned_zero(c.exp_kc)
        assert bool(same.all()), ("k_cache", int((~same).sum()), (~same).nonzero()[0].tolist())
        assert torch.equal(got_vc, c.exp_vc), ("v_cache", int((got_vc != c.exp_vc).sum()))
        # nothing else of the 8 GiB was written: the decoys, the blocks between, the spares
        want_k, want_v = c.cells()
        assert (count_not_sentinel(kc), count_not_sentinel(vc)) == (want_k, want_v)
    finally:
        del kc, vc
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------
# row offsets beyond 4 GiB
# ------------------------------------------------------------------------------------------------
ROW_CTX = (257, 33, 64, 0, 129, 65, 97, 200, 31, 130)                 # decode: 10 sequences
ROW_SEQS = ((33, 3), (64, 1), (97, 4), (40, 0), (130, 2))             # prefill: chunks packed over the 10 rows
ROW_APPEND = tuple((c, 1) for c in (1, 32, 33, 64, 65, 97, 128, 200, 31, 130))     # rope_append: 10 decode tokens


def assert_rows_beyond_4_gib():
    assert ROW_LD % 8 == 0 and ROW_LD >= (HQ + 2 * HKV) * D
    assert 7 * ROW_LD * 2 < 1 << 32 <= 8 * ROW_LD * 2 and ROWS == 10                # rows 8 and 9 start past 2^32 bytes
    assert len(ROW_CTX) == ROWS == sum(n for _, n in ROW_SEQS) == len(ROW_APPEND)
    assert ROW_CTX[8] > 0 and ROW_CTX[9] > 0 and sum(n for _, n in ROW_SEQS[:-1]) == 8     # rows 8, 9 are a chunk's


def strided_rows(heads, values=None):
    """(raw, view): a bf16 [10, heads, 128] view with row stride ROW_LD of one allocation.  With values the
    allocation is left uninitialised but for the rows; without, every cell holds SENT16."""
    raw = torch.empty(((ROWS - 1) * ROW_LD + heads * D,), dtype=torch.int16, device="cuda")
    view = raw.view(torch.bfloat16).as_strided((ROWS, heads, D), (ROW_LD, D, 1))
    if values is None:
        raw.fill_(SENT16)
    else:
        view.copy_(values)
    assert view.data_ptr() % 16 == 0 and view.stride(0) * 2 * 8 >= 1 << 32
    return raw, view


def only_the_rows_changed(raw, view, exp):
    """The rows' windows hold exp (bf16 [10, heads, 128], on the CPU; a zero of either sign, as in the exact
    modules), every other cell of the allocation still SENT16 -- compared in full on the device."""
    if not torch.equal(view.cpu(), exp):
        return False
    view.view(torch.int16).fill_(SENT16)
    return count_not_sentinel(raw) == 0


@functools.lru_cache(maxsize=None)
def row_case(kind):
    """CPU side: ("decode" | "prefill") -> a small ATT / PRE launch's operands and expectation with their
    own tables; "append" -> a WriterCase-like launch of 10 decode tokens."""
    assert_rows_beyond_4_gib()
    g = torch.Generator().manual_seed(9400 + len(kind))
    if kind == "append":
        ctxs = tuple(c for c, _ in ROW_APPEND)
        table, nb = PRE.block_tables(ctxs, g)
        x, v_bits, cs = ROPE.logical_operands("dyadic", ROWS, HQ + 2 * HKV, HKV, 257, g)
        qkv = x.to(torch.bfloat16)
        ROPE.bits(qkv)[:, HQ + HKV:] = v_bits
        ctx, q_start = torch.tensor(ctxs, dtype=torch.int32), torch.arange(ROWS + 1, dtype=torch.int32)
        ref_q, ref_k, pos, seq = ROPE.reference(qkv, cs, ctx, q_start, HKV)
        assert torch.equal(ref_q.float().double(), ref_q) and torch.equal(ref_k.float().double(), ref_k)
        exp_kc, exp_vc, _, _ = ROPE.expected_caches(nb, HKV, ROPE.bits(ref_k.float().to(torch.bfloat16)), v_bits, pos, seq, table)
        return dict(qkv=qkv, cs=cs, table=table, nb=nb, ctx=ctx, q_start=q_start, exp_q=ref_q.float().to(torch.bfloat16),
                    exp_kc=exp_kc, exp_vc=exp_vc)
    seqs = ROW_CTX if kind == "decode" else ROW_SEQS
    ctxs = tuple(seqs) if kind == "decode" else tuple(c for c, _ in seqs)
    mod = ATT if kind == "decode" else PRE
    table, nb = mod.block_tables(ctxs, g)
    q, ks, vs = mod.logical_operands("pair" if kind == "decode" else "match", GROUP, HKV, seqs, g)
    kc, vc = ATT.paged_caches(ks, vs, table, nb, HKV)
    ctx, qb = torch.tensor(ctxs, dtype=torch.int32), q.to(torch.bfloat16)
    assert qb.shape[0] == ROWS and torch.equal(qb.float(), q)
    if kind == "decode":
        q_start, ref = None, ATT.reference(qb, kc, vc, table, ctx)
    else:
        q_start = torch.tensor([0] + [n for _, n in seqs]).cumsum(0).to(torch.int32)
        ref = PRE.reference(qb, kc, vc, table, ctx, q_start)
    big = ref.abs() > 2.0 ** -20
    assert torch.equal(ref.float().double()[big], ref[big])                               # the means are exact in fp32
    return dict(q=qb, kc=kc, vc=vc, table=table, ctx=ctx, q_start=q_start, exp=ref.float().to(torch.bfloat16))


@pytest.mark.parametrize("kind", ["decode", "prefill", "append"])
def test_row_offsets_beyond_4_gib(kind):
    from k8s_gpu_scheduler_amd.ops import loadgen
    c = row_case(kind)
    need_free(ROW_NEED, "rows 2^28 + 8 elements apart: two allocations of 5 GiB")
    raw_in = raw_out = src = dst = None
    try:
        _, table = ATT.guarded_ints_2d(c["table"], c["table"].shape[1] + 2)
        _, ctx = PRE.guarded_ints(c["ctx"])
        if kind == "append":
            raw_in, src = strided_rows(HQ + 2 * HKV, c["qkv"].cuda())
            raw_out, dst = strided_rows(HQ)
            nb = c["nb"]
            kc = torch.full((nb, HKV, T, D), SENT16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
            vc = torch.full((nb, HKV, D, T), SENT16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
            _, q_start = PRE.guarded_ints(c["q_start"])
            loadgen.rope_append(src, guarded_input(c["cs"].cuda(), D, c0=0), kc, vc, table, ctx, q_start, q_out=dst)
            torch.cuda.synchronize()
            assert bool((ROPE.unsigned_zero(ROPE.bits(kc).cpu()) == ROPE.unsigned_zero(c["exp_kc"])).all())
            assert torch.equal(ROPE.bits(vc).cpu(), c["exp_vc"])
            assert only_the_rows_changed(raw_out, dst, c["exp_q"])
            return
        raw_in, src = strided_rows(HQ, c["q"].cuda())
        raw_out, dst = strided_rows(HQ)
        if kind == "decode":
            loadgen.paged_decode_attention(src, c["kc"].cuda(), c["vc"].cuda(), table, ctx, out=dst)
        else:
            _, q_start = PRE.guarded_ints(c["q_start"])
            loadgen.paged_prefill_attention(src, c["kc"].cuda(), c["vc"].cuda(), table, ctx, q_start, out=dst)
        torch.cuda.synchronize()
        assert torch.equal(dst.cpu(), c["exp"]), int((dst.cpu().float() != c["exp"].float()).sum())
        assert only_the_rows_changed(raw_out, dst, c["exp"])
    finally:
        del raw_in, raw_out, src, dst
        torch.cuda.empty_cache()
