"""CPU-only tests of the builders of test_gpu_paged_large_addresses.py: the geometry that puts blocks and
rows past 4 GiB, the re-dealt block tables, the decoys, and that a kernel whose offsets wrapped at 4 GiB
would miss the expectation -- computed with the float64 references on the compact caches alone."""
import pytest
import torch

import test_gpu_paged_large_addresses as L
import test_gpu_prefill_attn_exact as PRE
import test_gpu_rope_append_exact as ROPE
from test_gpu_kernels_exact import SENT16, SENT32


def test_blocks_and_rows_lie_beyond_4_gib():
    L.assert_beyond_4_gib()
    L.assert_rows_beyond_4_gib()
    assert L.NB == 262144 + 128 and L.HKV == 2 and L.GROUP == 4 and L.BLOCK_ELEMS * 2 == 16384
    ids = L.physical(torch.tensor([0, 63, 64, 127, SENT32]))
    assert ids.tolist() == [0, 63, 262144 + 64, L.NB - 1, SENT32]
    # a 32-bit byte offset, or an element offset mod 2^31, of a high block is its compact id's block
    for c in (64, 100, 127):
        b = int(L.physical(torch.tensor([c]))[0])
        assert (b * L.BLOCK_ELEMS * 2) % (1 << 32) == c * L.BLOCK_ELEMS * 2
        assert (b * L.BLOCK_ELEMS) % (1 << 31) == c * L.BLOCK_ELEMS
    assert L.ROW_LD == 2 ** 28 + 8 and 9 * L.ROW_LD * 2 + 12 * 128 * 2 < 6 << 30


def test_spread_keeps_the_shape_and_alternates():
    g = torch.Generator().manual_seed(1)
    table, nb = PRE.block_tables(L.CTX_DECODE, g)
    out = L.spread(table, g)
    assert torch.equal(out == SENT32, table == SENT32) and out.shape == table.shape
    for s in range(out.shape[0]):
        for j in range(out.shape[1]):
            if int(out[s, j]) != SENT32:
                assert (int(out[s, j]) < L.HALF_IDS) == ((j // 4 + j + s) % 2 == 0)
    one_side = out.clone()
    one_side[out != SENT32] = torch.arange(int((out != SENT32).sum()), dtype=torch.int32) % L.HALF_IDS
    with pytest.raises(AssertionError):
        L.assert_rows_mix(one_side, [0] * 8, [-(-c // 32) - 1 for c in L.CTX_DECODE], stride4=True)
    L.assert_decoys_unnamed(out)
    with pytest.raises(AssertionError):                               # all low: no high block, no decoy to land on
        L.assert_decoys_unnamed(one_side)


@pytest.mark.parametrize("kind", ["decode", "prefill"])
def test_a_reader_that_wraps_misses_the_expectation(kind):
    c = L.decode_case() if kind == "decode" else L.prefill_case()
    assert c.kc.shape == (128, 2, 32, 128) and c.vc.shape == (128, 2, 128, 32)
    assert bool((c.table[c.table != SENT32] < 128).all())
    if kind == "decode":
        assert c.ctxs == L.CTX_DECODE and max(-(-x // 32) for x in c.ctxs) == 10
    else:
        assert c.seqs == PRE.SEQS_A
    again = c.reference(c.kc, c.vc).float().to(torch.bfloat16)
    assert torch.equal(again, c.exp)
    wrapped = c.reference(*c.wrapped_caches())
    assert bool(wrapped.isfinite().all())                             # a wrong value, not a NaN the eye would catch
    wrong = (wrapped.float().to(torch.bfloat16).float() != c.exp.float()).flatten(1).any(1)
    assert float(wrong.float().mean()) > 0.5, int(wrong.sum())
    # the device's physical table names no decoy
    phys = L.physical(c.table)
    named = phys[phys != SENT32]
    assert not bool(((named >= L.HALF_IDS) & (named < L.COMPACT)).any())
    assert bool((named >= L.HIGH).any()) and bool((named < L.HALF_IDS).any()) and int(named.max()) < L.NB


def test_the_writer_case():
    c = L.writer_case()
    assert c.seqs == ROPE.SEQS_C and c.n == sum(n for _, n in ROPE.SEQS_C) == 582
    k, v = c.cells()
    assert k <= c.owned == 582 * 2 * 128 and v <= c.owned
    named = torch.zeros(128, dtype=torch.bool)
    for s in range(c.S):
        named[c.table[s, c.first[s]:c.last[s] + 1].long()] = True
    touched_k = (c.exp_kc.flatten(1) != SENT16).any(1)
    assert torch.equal(touched_k, named) and torch.equal((c.exp_vc.flatten(1) != SENT16).any(1), named)
    # a writer that wraps leaves the high blocks SENT16 and writes their decoys: both break the count's twin,
    # the bitwise comparison of the named blocks
    assert bool(named[L.HALF_IDS:].any()) and bool(named[:L.HALF_IDS].any())
    assert bool(c.exp_q.float().isfinite().all()) and c.exp_q.shape == (582, 8, 128)


@pytest.mark.parametrize("kind", ["decode", "prefill", "append"])
def test_the_row_cases(kind):
    c = L.row_case(kind)
    if kind == "append":
        assert c["qkv"].shape == (10, 12, 128) and c["q_start"].tolist() == list(range(11))
        assert int((c["exp_kc"] != SENT16).any(-1).sum()) == 10 * 2                      # one slot per token and KV head
        return
    assert c["q"].shape == (10, 8, 128) == c["exp"].shape and bool(c["exp"].float().isfinite().all())
    if kind == "prefill":
        assert c["q_start"].tolist() == [0, 3, 4, 8, 8, 10]
    assert bool(c["exp"][8:].float().abs().sum() > 0)                                     # rows 8 and 9 have something to show
