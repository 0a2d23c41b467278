"""Top-k / top-p token sampling without a GPU: the workload model's op kind, the two LLM-head workloads and their
table, the pure-Python grid rule, the host wrapper's validation (which must fire before the native module is
touched), the executor's op dispatch and operands, and the float64 reference sampler of the GPU tests with the
separation its cases keep.  The kernel itself is pinned on the GPU by test_gpu_sample_exact.py, the LM-head
projection's shape by test_gpu_lm_head_gemm_exact.py."""
import pytest
import torch

from k8s_gpu_scheduler_amd import _native
from k8s_gpu_scheduler_amd.models import workloads as W
from k8s_gpu_scheduler_amd.ops import loadgen

BF = torch.bfloat16
OLD_TABLES = ("CATALOG", "EXTRA", "STAGED", "LONG_CONTEXT", "LLM_LAYER", "LLM_BLOCK")


# ------------------------------------------------------------------------------------------------
# workload model
# ------------------------------------------------------------------------------------------------
def test_op_flops_bytes_workgroups():
    s = W.Op("sample", 3, 1016, 50)
    assert not s.is_gemm and not s.on_mfma and s.mfma_rate() == 1.0
    assert s.flops == 2 * 3 * 1016 == 6096                            # the maximum's and the selection's compare per logit
    assert s.bytes == 2 * 3 * 1016 + 20 * 3 == 6156                   # the logits once, five words per row
    assert s.workgroups(0) == s.workgroups(64) == 3
    big = W.Op("sample", 256, 128256, 50)
    assert big.flops == 65667072 and big.bytes == 65672192 and big.workgroups(64) == 256
    assert W.Op("sample", 0, 128256, 50).bytes == 0 and W.Op("sample", 0, 128256, 50).workgroups(0) == 0
    assert [W.default_sample_workgroups(s) for s in (0, 1, 8, 256, 4096)] == [0, 1, 8, 256, 4096]


@pytest.mark.skipif(_native.hip(required=False) is None, reason="HIP extension not built")
def test_default_workgroups_match_the_native_rule():
    h = _native.hip()
    for S in (0, 1, 3, 8, 256, 4096, 100000, 2 ** 31 - 1):
        assert h.sample_workgroups(S) == W.default_sample_workgroups(S)
    with pytest.raises(RuntimeError):
        h.sample_workgroups(-1)


def operand_bytes(o):
    """Bytes of the operands parallel.executor allocates for one op, from its shapes (the rule of
    test_norm_act_cpu.py, with the sampler's row)."""
    if o.kind == "gemm":
        return 2 * (o.M * o.K + o.N * o.K + o.M * o.N) + 4 * o.N
    if o.kind == "add_rmsnorm":
        return 2 * (4 * o.M * o.N + o.N)
    if o.kind == "sample":
        return 2 * o.M * o.N + 5 * 4 * o.M
    raise AssertionError(o.kind)


def test_llm_head_workloads_and_their_table():
    big, few = W.get("llm_head_decode_256"), W.get("llm_head_decode_8")
    assert W.LLM_HEAD == {"llm_head_decode_256": big, "llm_head_decode_8": few}
    assert big.ops == (W.Op("add_rmsnorm", 256, 4096), W.Op("gemm", 256, 128256, 4096, relu=False), W.Op("sample", 256, 128256, 50))
    assert few.ops == (W.Op("add_rmsnorm", 64, 4096), W.Op("gemm", 64, 128256, 4096, relu=False), W.Op("sample", 8, 128256, 50))
    assert (big.family, big.framework, big.batch, big.hbm_gib) == ("llm_head_decode", "hip", 256, 1.25)
    assert (few.family, few.framework, few.batch, few.hbm_gib) == ("llm_head_decode_few", "hip", 8, 1.0)
    for w in (big, few):
        norm, head, pick = w.ops
        assert norm.M == head.M and norm.N == head.K == 4096 and head.N == pick.N == 128256 and not head.relu
        assert pick.M == w.batch <= head.M and 1 <= pick.K <= 64
        need = sum(operand_bytes(o) for o in w.ops)
        assert w.hbm_gib * 2 ** 30 >= need > (w.hbm_gib - 0.25) * 2 ** 30, (w.name, need / 2 ** 30)
        assert 0.0 < W.cu_fill(w) <= 1.0
        m, h = W.roofline_split(w.name.replace("_", "-") + "-0")
        assert m > 0 and h >= (norm.bytes + pick.bytes) / 6.0e12 > 0
        assert 2 * head.N * head.K == 1050673152 and head.bytes > 10 * (norm.bytes + pick.bytes)    # the weights dominate the traffic
    assert [o.workgroups(64) for o in big.ops] == [256, 501, 256]
    assert [o.workgroups(64) for o in few.ops] == [64, 1002, 8]                          # 8 workgroups on 256 CUs
    assert [o.workgroups(0) for o in few.ops] == [64, 1002, 8]
    assert W.cu_fill(few) < 1.0 == W.cu_fill(big)


def test_the_older_tables_are_unchanged():
    assert len(W.CATALOG) == 18 and set(W.EXTRA) == {"fp8_llm_2048", "triad_only_2048", "dlrm_2048", "llm_decode_256"}
    assert set(W.STAGED) == {"llm_prefill_2048"} and set(W.LONG_CONTEXT) == {"llm_decode_long_8"}
    assert set(W.LLM_LAYER) == {"llm_layer_decode_256", "llm_layer_prefill_2048"}
    assert set(W.LLM_BLOCK) == {"llm_block_decode_256", "llm_block_prefill_2048"}
    assert len(W.LLM_BLOCK["llm_block_decode_256"].ops) == 9 and W.LLM_BLOCK["llm_block_decode_256"].hbm_gib == 2.5
    assert W.LONG_CONTEXT["llm_decode_long_8"].ops == (W.Op("gemm", 64, 6144, 4096), W.Op("attn_split", 8, 32, 32768, rows=8, splits=4),
                                                       W.Op("gemm", 64, 4096, 4096))
    for name in OLD_TABLES:
        assert all(o.kind != "sample" for w in getattr(W, name).values() for o in w.ops), name


def test_get_and_workload_for_pod():
    big, few = W.LLM_HEAD["llm_head_decode_256"], W.LLM_HEAD["llm_head_decode_8"]
    assert W.get("llm_head_decode_256") is big and W.get("llm_head_decode_8") is few
    assert W.workload_for_pod("llm-head-decode-256-x") is big and W.workload_for_pod("pod-llm-head-decode-8-7") is few
    assert W.workload_for_pod("llm-block-decode-256-x") is W.LLM_BLOCK["llm_block_decode_256"]
    assert W.workload_for_pod("llm-decode-long-8-x") is W.LONG_CONTEXT["llm_decode_long_8"]
    # a pod name that holds an old and a new name: the older tables are consulted first
    assert W.workload_for_pod("llm-head-decode-256-and-llm-block-decode-256") is W.LLM_BLOCK["llm_block_decode_256"]
    assert W.workload_for_pod("llm-head-decode-8-and-llm-decode-long-8") is W.LONG_CONTEXT["llm_decode_long_8"]
    names = [n for t in OLD_TABLES for n in getattr(W, t)]
    for new in W.LLM_HEAD:
        assert not any(old in new or new in old for old in names), new
    assert not any(a != b and a in b for a in W.LLM_HEAD for b in W.LLM_HEAD)
    for bad in ("llm_head", "llm_head_decode", "llm-head-decode-256", "llm_head_decode_255", "llm_head_decode_"):
        with pytest.raises(KeyError):
            W.get(bad)
    for bad in ("llm-head-decode-255", "llm-head-decode", "llm-head-decode-7"):
        with pytest.raises(KeyError):
            W.workload_for_pod(bad)


# ------------------------------------------------------------------------------------------------
# host wrapper: every rejection happens before the native module is asked for
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def no_native(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the native module was touched")
    monkeypatch.setattr(_native, "hip", boom)


@pytest.fixture
def host_operands_pass(monkeypatch, no_native):
    """The checks after the device check run on host tensors once it is stubbed out."""
    monkeypatch.setattr(loadgen, "_check_devices", lambda name, *ts: torch.device("cpu"))


def _args(S=3, V=16):
    return (torch.zeros(S, V, dtype=BF), torch.zeros(S), torch.ones(S), torch.full((S,), 5, dtype=torch.int32), torch.ones(S))


def test_wrapper_rejects_cpu_tensors(no_native):
    lg, u, t, k, p = _args()
    with pytest.raises(ValueError, match="device tensors"):
        loadgen.sample_tokens(lg, u, t, k, p)
    with pytest.raises(ValueError, match="device tensors"):          # before any dtype complaint
        loadgen.sample_tokens(lg.float(), u, t, k.long(), p)


def test_wrapper_rejects_dtypes_then_shapes_and_strides(host_operands_pass):
    lg, u, t, k, p = _args()
    with pytest.raises(TypeError, match="bf16 logits"):
        loadgen.sample_tokens(lg.float(), u, t, k, p)
    with pytest.raises(TypeError, match="bf16 logits"):               # dtypes come before the shape rules
        loadgen.sample_tokens(lg.float()[0], u, t, k, p)
    with pytest.raises(TypeError, match="fp32 u"):
        loadgen.sample_tokens(lg, u.double(), t, k, p)
    with pytest.raises(TypeError, match="fp32 temperature"):
        loadgen.sample_tokens(lg, u, t.to(BF), k, p)
    with pytest.raises(TypeError, match="fp32 top_p"):
        loadgen.sample_tokens(lg, u, t, k, p.half())
    for bad in (k.long(), k.float(), k.to(torch.int16)):
        with pytest.raises(TypeError, match="int32 top_k"):
            loadgen.sample_tokens(lg, u, t, bad, p)
    with pytest.raises(TypeError, match="int32 out"):
        loadgen.sample_tokens(lg, u, t, k, p, out=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(TypeError, match="int32 out"):                 # before the stride rule of the logits
        loadgen.sample_tokens(torch.zeros(3, 20, dtype=BF)[:, :16], u, t, k, p, out=torch.zeros(3))
    for bad in (lg[0], lg[None]):
        with pytest.raises(ValueError, match="logits must be 2-D"):
            loadgen.sample_tokens(bad, u, t, k, p)
    with pytest.raises(ValueError, match="contiguous rows"):
        loadgen.sample_tokens(torch.zeros(3, 32, dtype=BF)[:, ::2], u, t, k, p)
    with pytest.raises(ValueError, match="logits row stride 20"):
        loadgen.sample_tokens(torch.zeros(3, 20, dtype=BF)[:, :16], u, t, k, p)
    with pytest.raises(ValueError, match="logits row stride 8"):      # rows overlap
        loadgen.sample_tokens(torch.zeros(64, dtype=BF).as_strided((3, 16), (8, 1)), u, t, k, p)
    with pytest.raises(ValueError, match="logits must be 16-byte aligned"):
        loadgen.sample_tokens(torch.zeros(3 * 16 + 8, dtype=BF)[4:4 + 48].view(3, 16), u, t, k, p)
    with pytest.raises(ValueError, match="logits row stride 20"):     # the stride rule comes before the V rule
        loadgen.sample_tokens(torch.zeros(3, 20, dtype=BF)[:, :12], u, t, k, p)


def test_wrapper_rejects_vocabularies(host_operands_pass):
    for V in (0, 4, 12, 131080, 262144):
        with pytest.raises(ValueError, match=r"multiple of 8 in \[8, 131072\]"):
            loadgen.sample_tokens(torch.zeros(1, V, dtype=BF), torch.zeros(1), torch.ones(1), torch.ones(1, dtype=torch.int32),
                                  torch.ones(1))
    with pytest.raises(ValueError, match=r"multiple of 8 in \[8, 131072\]"):      # before the vectors' lengths
        loadgen.sample_tokens(torch.zeros(1, 12, dtype=BF), torch.zeros(2), torch.ones(1), torch.ones(1, dtype=torch.int32),
                              torch.ones(1))
    for V in (8, 131072):
        with pytest.raises(AssertionError, match="native module was touched"):     # every check passed
            loadgen.sample_tokens(torch.zeros(1, V, dtype=BF), torch.zeros(1), torch.ones(1), torch.ones(1, dtype=torch.int32),
                                  torch.ones(1))
    with pytest.raises(ValueError, match="more than 2\\^31 - 1 rows"):
        loadgen.sample_tokens(torch.empty(2 ** 31, 8, dtype=BF, device="meta"), torch.zeros(1), torch.ones(1),
                              torch.ones(1, dtype=torch.int32), torch.ones(1))


def test_wrapper_rejects_vectors_and_out(host_operands_pass):
    lg, u, t, k, p = _args()
    names = ("u", "temperature", "top_k", "top_p")
    for i, nm in enumerate(names):
        good = [u, t, k, p]
        for bad in (good[i][:2], good[i][None], good[i].repeat(2)[::2], good[i].repeat(2)):
            args = list(good)
            args[i] = bad
            with pytest.raises(ValueError, match=f"{nm} must be a contiguous vector of length S = 3"):
                loadgen.sample_tokens(lg, *args)
    with pytest.raises(ValueError, match="u must be"):                # in the order u, temperature, top_k, top_p
        loadgen.sample_tokens(lg, u[:2], t[:2], k[:2], p[:2])
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)                 # noqa: E731
    for bad in (i32(2), i32(4), i32(6)[::2], i32(3)[None]):
        with pytest.raises(ValueError, match="out must be a contiguous vector of length S = 3"):
            loadgen.sample_tokens(lg, u, t, k, p, out=bad)
    with pytest.raises(ValueError, match="u must be"):                # the vectors come before out
        loadgen.sample_tokens(lg, u[:2], t, k, p, out=i32(2))
    with pytest.raises(ValueError, match="out overlaps top_k"):
        loadgen.sample_tokens(lg, u, t, k, p, out=k)
    both = i32(6)
    with pytest.raises(ValueError, match="out overlaps top_k"):      # interleaved in one allocation
        loadgen.sample_tokens(lg, u, t, both[1:4], p, out=both[:3])
    for nm, view in (("u", u), ("temperature", t), ("top_p", p)):
        with pytest.raises(ValueError, match=f"out overlaps {nm}"):
            loadgen.sample_tokens(lg, u, t, k, p, out=view.view(torch.int32))
    wide = torch.zeros(3, 32, dtype=BF)
    with pytest.raises(ValueError, match="out overlaps logits"):     # in the gap a padded row stride leaves
        loadgen.sample_tokens(wide[:, :16], u, t, k, p, out=wide.view(torch.int32)[0, 8:11])
    with pytest.raises(AssertionError, match="native module was touched"):
        loadgen.sample_tokens(lg, u, t, k, p, out=both[:3])           # every check passed
    with pytest.raises(AssertionError, match="native module was touched"):
        loadgen.sample_tokens(wide[:, 8:24], u, t, k, p, check=False)


def test_the_empty_launch(host_operands_pass):
    lg, u, t, k, p = _args(S=0)
    out = loadgen.sample_tokens(lg, u, t, k, p)
    assert out.shape == (0,) and out.dtype == torch.int32
    given = torch.zeros(0, dtype=torch.int32)
    assert loadgen.sample_tokens(lg, u, t, k, p, out=given) is given
    assert loadgen.sample_tokens(lg, u, t, k, p, check=False).shape == (0,)
    with pytest.raises(ValueError, match="u must be"):                # still validated
        loadgen.sample_tokens(lg, torch.zeros(1), t, k, p)


# ------------------------------------------------------------------------------------------------
# executor
# ------------------------------------------------------------------------------------------------
def test_enqueue_ops_dispatches_the_kind(monkeypatch):
    from k8s_gpu_scheduler_amd.parallel import executor
    calls = []
    monkeypatch.setattr(loadgen, "sample_tokens", lambda *a, **k: calls.append(("sample_tokens", a, k)))

    class Stub:
        ops = [(W.Op("sample", 2, 16, 5), ("out", "logits", "u", "temperature", "top_k", "top_p"))]

    executor.enqueue_ops(Stub(), 2, "stream", 64)
    assert calls == [("sample_tokens", ("logits", "u", "temperature", "top_k", "top_p"),
                      {"out": "out", "stream": "stream", "check": False})] * 2
    assert executor.op_output(*Stub.ops[0]) == "out" and executor.OP_KINDS["sample"][2] == 0
    assert {o.kind for w in W.LLM_HEAD.values() for o in w.ops} <= set(executor.OP_KINDS)
    with pytest.raises(ValueError, match="unknown op kind"):
        executor.enqueue_op(W.Op("sampel", 2, 16, 5), (), "stream", 0)


def test_buffers_build_the_operands_reproducibly():
    from k8s_gpu_scheduler_amd.parallel.executor import _Buffers
    w = W.Workload("t_sample", "test", "hip", 5, (W.Op("add_rmsnorm", 5, 64), W.Op("sample", 5, 8200, 40)), 0.0)
    cpu = torch.device("cpu")
    a, b = _Buffers(w, cpu), _Buffers(w, cpu)
    out, logits, u, t, k, p = a.ops[1][1]
    assert logits.shape == (5, 8200) and logits.dtype == BF and logits.is_contiguous()
    assert out.shape == (5,) and out.dtype == torch.int32
    assert all(x.shape == (5,) and x.dtype == torch.float32 for x in (u, t, p)) and k.shape == (5,) and k.dtype == torch.int32
    assert 1.3 < logits.float().std() < 1.7 and abs(logits.float().mean()) < 0.05
    assert bool(((u >= 0) & (u < 1)).all()) and len(u.unique()) == 5
    assert t.tolist() == [torch.tensor(0.8).item()] * 5 and k.tolist() == [40] * 5 and p.tolist() == [torch.tensor(0.9).item()] * 5
    for x, y in zip(a.ops[1][1][1:], b.ops[1][1][1:]):
        assert torch.equal(x, y) and x.data_ptr() != y.data_ptr()
    loadgen_args_pass = dict(zip(("logits", "u", "temperature", "top_k", "top_p"), (logits, u, t, k, p)))
    assert all(not loadgen._overlap(out, x) for x in loadgen_args_pass.values())


# ------------------------------------------------------------------------------------------------
# the GPU tests' reference
# ------------------------------------------------------------------------------------------------
def test_the_reference_asserts_its_preconditions():
    import test_gpu_sample_exact as S
    S.test_the_shapes_cover_the_walk()
    row = torch.tensor([0.5, 3.0, -1.0, 3.0, 2.0, -0.0, 0.0, 1.0]).to(BF)
    assert S.ranking(row, 8).tolist() == [1, 3, 4, 7, 0, 5, 6, 2]                     # ties, +-0 included, to the lowest index
    assert S.clamp_k(0, 100) == S.clamp_k(-5, 100) == 1 and S.clamp_k(65, 100) == S.clamp_k(2 ** 31 - 1, 100) == 64
    assert S.clamp_k(50, 8) == 8
    tok, sep = S.reference_sample(row, 0.1, 1.0, 3, 1.0)
    w = [1.0, 1.0, torch.e ** -1]                                                      # ranks 0, 1, 2: indices 1, 3, 4
    assert tok == 1 and abs(sep - w[2] / sum(w)) < 1e-12               # cum_1 is the nearest to top_p * Z = Z, cum_2 == Z aside
    assert abs(S.reference_sample(row, 0.1, 1.0, 2, 1.0)[1] - 0.4) < 1e-12             # the target 0.2 from cum_0 = 1, of Z = 2
    assert S.reference_sample(row, 0.5, 1.0, 3, 1.0)[0] == 3 and S.reference_sample(row, 0.99, 1.0, 3, 1.0)[0] == 4
    assert S.reference_sample(row, 0.99, 1.0, 3, 0.5)[0] == 3                         # the cut keeps two: 2 / 2.37 >= 0.5 > 1 / 2.37
    assert S.reference_sample(row, 0.99, 1.0, 3, 0.3)[0] == 1                         # ... and one
    assert S.reference_sample(row, 0.0, 1.0, 100, 1.0)[0] == 1
    for bad in (dict(u=1.0), dict(u=-0.1), dict(temperature=0.0), dict(temperature=S.INF), dict(top_k=1), dict(top_p=0.0),
                dict(top_p=1.5)):
        kw = dict(u=0.5, temperature=1.0, top_k=3, top_p=1.0)
        kw.update(bad)
        with pytest.raises(AssertionError):
            S.reference_sample(row, **kw)
    nan = row.clone()
    nan[2] = S.NAN
    with pytest.raises(AssertionError):
        S.reference_sample(nan, 0.5, 1.0, 3, 1.0)
    with pytest.raises(AssertionError):
        S.reference_sample(torch.full((8,), S.INF).to(BF), 0.5, 1.0, 3, 1.0)
    with pytest.raises(AssertionError, match="exponent below -64"):
        S.reference_sample(torch.tensor([0.0, -100.0] * 4).to(BF), 0.5, 1.0, 8, 1.0)
    assert S.order_keys(torch.tensor([0.0, -0.0, S.INF, -S.INF, 1.0, -1.0]).to(BF)).tolist() == [0x8000, 0x8000, 0xFF80, 0x0080,
                                                                                                0xBF80, 0x4080]
    assert S.SEP == 8 * S.E == 2.0 ** -11


def test_the_builders_of_the_exact_cases():
    import test_gpu_sample_exact as S
    for V in S.VS:
        b = S.boundary_indices(V)
        assert b == sorted(set(b)) and b[0] == 0 and b[-1] == V - 1
        where = S.spread_indices(V, min(70, V), 1)
        assert len(set(where)) == min(70, V) and set(b[:min(70, V)]) <= set(where) | set(b[70:]) and where == sorted(where)
        for name, row in S.hostile_rows(V, 9500 + V).items():
            assert row.shape == (V,) and row.dtype == BF and not bool(row.isnan().any()), name
            for k in (64, 7):
                exp, u = S.flat_expectation(row, k)
                n = len(exp)
                assert 1 <= n <= min(k, V) and len(set(exp.tolist())) == n and bool(row[exp.long()].float().isfinite().all())
                # the candidates past the n finite ones are -Inf (weight exactly 0), or there are none
                rest = S.ranking(row, S.clamp_k(k, V))[n:]
                assert bool((row[rest].float() == -S.INF).all())
                assert bool((u * n - torch.arange(n) == 0.5).all())
        stairs = S.hostile_rows(V, 9500 + V)["staircase"]
        keys = S.order_keys(stairs).sort(descending=True).values[:min(64, V)]
        assert int((keys[:-1] - keys[1:]).min()) > 256                                 # no two of the top 64 share a window
        assert int(keys[0] - keys[-1]) > 256 * (min(64, V) - 1)
    zeros = S.hostile_rows(8200, 1)["around-zero"]
    assert {0, -32768} <= set(zeros.view(torch.int16).tolist())                        # both zero signs
    row = S.plateau_row(1016, [3, 5], -196.0)
    assert row[3] == -196 and row[0] == -300
    with pytest.raises(AssertionError):
        S.plateau_row(1016, [3, 5], -200.0)                                            # the background's weight would not be 0


@pytest.mark.parametrize("V", (1016, 8200, 128256))
def test_the_margin_cases_keep_the_separation(V):
    """Every rank of every (T, top_k, top_p) case: the interval of every kept rank is at least 2^-10 of Z wide, and u
    and top_p, after their rounding to fp32, sit at least 8 E from the nearest boundary."""
    import test_gpu_sample_exact as S
    base, which, u, t, k, p, tokens, seps = S.margin_case(V)
    assert base.shape == (3, V) and len(which) == len(u) == len(tokens) == len(seps)
    assert bool((seps >= S.SEP).all()), seps.min().item()
    narrowest = 1.0
    for i, T in enumerate(S.TS):
        l = base[i][S.ranking(base[i], 64)].double()
        w = torch.exp2((l - l[0]) * (S.LOG2E / T))
        for kk in S.KS:
            narrowest = min(narrowest, (w[:kk].min() / w[:kk].sum()).item())
        assert abs(base[i].float().std().item() / (1.5 * T) - 1) < 0.1
    print(f"margin cases V = {V}: {len(u)} rows, narrowest interval 2^{torch.tensor(narrowest).log2().item():.2f} of Z, "
          f"smallest separation 2^{seps.min().log2().item():.2f}")
    assert narrowest >= 2.0 ** -10
    # every (T, top_k, mode) is there, with every kept rank: n rows per case, distinct tokens within a case
    cases = {}
    for r in range(len(u)):
        cases.setdefault((t[r].item(), k[r].item(), p[r].item() == 1.0), []).append(tokens[r].item())
    assert len(cases) == 24 and {c[:2] for c in cases} == {(T, kk) for T in S.TS for kk in S.KS}
    for (T, kk, whole), toks in cases.items():
        assert len(set(toks)) == len(toks) == (kk if whole else max(kk // 2, 1) + 1), (T, kk, whole)
        assert toks == base[S.TS.index(T)].double().sort(descending=True, stable=True).indices[:len(toks)].tolist()


@pytest.mark.parametrize("workload", ["llm_head_decode_8", "llm_head_decode_256"])
def test_the_executors_sampling_rows_keep_the_separation(workload):
    """What the GPU module's pod-path test relies on: fewer than 1/4 of the executor's rows of the sample op sit
    closer than 8 E to a boundary (they are left out of its comparison).
    Counted: llm_head_decode_256 leaves 40 of 256 rows out, llm_head_decode_8 none of its 8.  (With the logits drawn
    before u the same seeds left 41 of 256 and 2 of 8 out -- separations 2^-13.96 and 2^-13.41 of Z against the
    required 2^-11 -- and 2 of 8 is not fewer than 1/4: about one row in six is left out, so an 8-row workload meets
    the condition with some seeds and not with others.  E and the fraction stayed as they were.)"""
    import test_gpu_sample_exact as S
    from k8s_gpu_scheduler_amd.parallel.executor import _Buffers
    a = _Buffers(W.get(workload), torch.device("cpu"))
    out, logits, u, t, k, p = a.ops[2][1]
    rows, toks = S.admitted_rows(logits, u, t, k, p)
    left_out = logits.shape[0] - len(rows)
    print(f"{workload}: {left_out} of {logits.shape[0]} rows left out")
    assert len(rows) == len(toks) and bool(((toks >= 0) & (toks < 128256)).all())
    assert 4 * left_out < logits.shape[0], f"{left_out} of {logits.shape[0]} rows are closer than 8 E to a boundary"
