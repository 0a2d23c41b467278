"""The LM-head projection's shape through the bf16 GEMM path, bit-exact (run with `-m gpu` on an MI355X).

N = 128,256 (Llama-3's vocabulary) is new ground for the GEMM path: 501 column tiles of 256 or 1,002 of 128, far
more than any pinned shape has, and -- 128256 = 2^8 * 3 * 167 -- no multiple of 512.  The operands are the
integer ones of test_gpu_kernels_exact.py (every product and sum exact, so the expectation is independent of
the summation order), run through its guarded path: NaN-guarded, offset A and Bt, and C as a window (column
offset 8, row stride N + 8) of a sentinel-filled allocation compared bitwise afterwards.  K is short: it is
the column walk that is new, not the K loop, which test_gpu_kernels_exact.py covers at every ring length.

  (64, 128256, 64)    the rows of llm_head_decode_8's projection: the 64 x 128 tile under both budgets, 1,002 workgroups
  (256, 128256, 128)  the rows of llm_head_decode_256's: the 256 x 256 tile, 501
                      workgroups

each under cu_budget 0 and 64, with the default policy and knobs, both regimes and all four (relu, bias) pairs.
"""
import pytest

from test_gpu_kernels_exact import WIDE_C, hip, default_knobs, run_exact          # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

# MEASURED on an MI355X (printed by the tests):
MEASURED = """
  All four (shape, budget) cases bit-exact in both regimes and all four (relu, bias) pairs, guards intact: no fault
  in the GEMM path at N = 128,256.  Grids: 1,002 workgroups (the 64 x 128 tile) at 64 rows and 501 (256 x 256) at 256
  rows, for K = 64 / 128 and for the workloads' K = 4,096, under both budgets.  The module: 5 tests in 1 s.
"""

SHAPES = ((64, 128256, 64), (256, 128256, 128))
WORKLOAD_SHAPES = ((64, 128256, 4096), (256, 128256, 4096))


@pytest.mark.parametrize("cu_budget", (0, 64))
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_lm_head_gemm_exact(hip, M, N, K, cu_budget):
    assert hip.knobs() == hip.knob_defaults()
    run_exact(M, N, K, cu_budget, pad=WIDE_C)


def test_lm_head_gemm_workgroups_match_the_python_rule(hip):
    from k8s_gpu_scheduler_amd.models import workloads as W
    got = {}
    for M, N, K in WORKLOAD_SHAPES + SHAPES:
        for budget in (0, 64):
            got[(M, K, budget)] = hip.gemm_workgroups(M, N, K, budget, False, False)
            assert got[(M, K, budget)] == W.default_gemm_workgroups(M, N, K, budget), (M, N, K, budget)
    print(f"LM-head GEMM workgroups (M, K, budget): {got}")
    assert got[(64, 4096, 64)] == 1002 and got[(256, 4096, 64)] == 501
    for w in W.LLM_HEAD.values():
        gemm = w.ops[1]
        assert (gemm.N, gemm.K) == (128256, 4096) and (gemm.M, gemm.N, gemm.K) in WORKLOAD_SHAPES
