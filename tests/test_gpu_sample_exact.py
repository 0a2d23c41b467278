"""Exact, guarded-buffer tests of top-k / top-p token sampling (run with `-m gpu` on an MI355X), in the style of
test_gpu_swiglu_exact.py and of test_gpu_kernels_exact.py, whose guard helpers and sentinels are used.

Every launch runs guarded: logits is a window (column offset 8, row stride V + 8) of a NaN-filled allocation,
out a window (16 cells in) of a SENT32-filled int32 allocation that is compared whole afterwards.

Shapes (S, V) of SHAPES -- the vocabularies are what matters, the tests bring their own row counts.  A workgroup
of 1,024 threads takes a row, thread t the 16-byte chunks t, t + 1024, .. of it ("rounds" of 1,024 chunks):
(1, 8) and (1, 64) hold fewer elements than candidates (k = min(top_k, V)); (3, 1016) has a ragged last chunk
inside the first round; (2, 8192) exactly one chunk per thread; (2, 8200) one chunk into the second round;
(1, 128256) is the real vocabulary, 15 full rounds and a partial one; (1, 131072) the cap.
test_the_shapes_cover_the_walk asserts this.

Expectations:

  greedy    the lowest index of the maximum, planted at the boundaries of the walk; bit-exact.
  plateau   background -300, a plateau of equal values, temperature 1: the background's weights are exactly 0
            ((-300 - h) * log2 e <= -150 for h >= -196) and the plateau's exactly 1, so cum_j = j + 1 whatever the
            scan's association, and u_j = (j + 0.5) / k must give the plateau's j-th lowest index.  No exponential
            in the expectation.
  hostile   rows that are hard for the SELECTION (a staircase over 128 binades, one value far above a crowd,
            -Inf among the candidates, negative-only rows, signed zeros and subnormals), with plateau-style
            weights: temperature 2^100, so every a_j = (l_j - l_0) * c has magnitude below 2^-80 and every finite
            candidate's weight is 1 to within the exponential's last place; cum_j is j + 1 to within 2^-17, and
            u_j = (j + 0.5) / n sits half a unit from either boundary.  The ranking comes from a stable sort on
            the CPU.  -Inf candidates have weight exactly 0.
  margin    bf16(1.5 * T * randn) logits against the float64 reference (`reference_sample`), T in {0.5, 1, 2},
            top_k in {2, 5, 40, 64}, top_p 1 or the midpoint between two consecutive cumulative fractions, and for
            EVERY kept rank j a row whose u is the midpoint of rank j's interval; all cases of a vocabulary in one
            launch (a per-row mix of temperatures, top_k and top_p).  The tokens must match exactly, given the
            separation below.

The fp32 error bound E of the kernel's cum_j and target, relative to Z.  l_j - l_0 is one fp32 subtraction of two
bf16 values (2^-24 relative), c = 1.44269504f / temperature carries the constant's 2^-25 and the division's
2^-24, the product another 2^-24: a_j is within 2^-22 |a_j| of the true exponent, which changes 2^a_j by
ln 2 * 2^-22 |a_j| <= 2^-16.5 relative for |a_j| <= 64 (asserted by the reference).  v_exp_f32 is documented at
1 ulp: 2^-23.  The prefix sum is at most 64 additions of non-negative terms, each 2^-24 of its partial sum <= Z:
2^-18 Z.  So |cum_j - true| <= (2^-16.5 + 2^-23 + 2^-18) Z < 2^-16 Z; the products u * cum_{n-1} and top_p * Z add
2^-24.  A comparison between two such quantities is decided as in exact arithmetic when they are at least
2^-15 Z apart; E = 2^-14 rounds that up.  Every tested u and top_p must sit at least 8 E = 2^-11 of Z from the
nearest boundary -- the factor of 8 for the reason given in test_gpu_swiglu_exact.py: the instruction's accuracy is
taken from documentation, not from a measurement.  That is a CONDITION on the test's inputs, asserted for every
case and every rank, not a tolerance: no case is dropped for failing it.
"""
import functools
import time

import pytest
import torch

import test_gpu_corun_exact as CO
from test_gpu_kernels_exact import NAN, SENT32, guarded_input

pytestmark = pytest.mark.gpu

# MEASURED on an MI355X (printed by the tests):
MEASURED = """
  Margin regime: 510 of 510 tokens match at each of V = 1016, 8200 and 128256; the smallest separation used was
  2^-8.27, 2^-7.92 and 2^-8.03 of Z (required: 2^-11).  Every greedy, plateau, hostile-row, degenerate-row, clamp,
  replay, large-address and co-run token bit-exact.
  Pod path: llm_head_decode_8 -- 8 of 8 rows admitted, 8 of 8 tokens match; llm_head_decode_256 -- 216 of 256 rows
  admitted, 40 left out, 216 of 216 tokens match.  (The executor draws u before the logits.  Drawn after them, the
  same seeds left 2 of 8 and 41 of 256 rows out, and 2 of 8 is not fewer than 1/4; the admitted tokens matched
  there too, 6 of 6 and 215 of 215.)  Building a workload's operands takes 2.6 to 2.9 s, nearly all of it the
  128,256 x 4,096 LM-head weight drawn on the host.
  The module: 71 tests in 12 s, 7 s of them the two pod-path tests.
"""

BF = torch.bfloat16
C0 = 8                                  # column offset of the logits window
GB, GA = 16, 48                         # sentinel cells before and after out's window
SHAPES = ((1, 8), (1, 64), (3, 1016), (2, 8192), (2, 8200), (1, 128256), (1, 131072))
VS = tuple(v for _, v in SHAPES)
THREADS, ROUND = 1024, 8192             # threads of a workgroup; elements of a round (1,024 chunks of 8)
WAVE_ELEMS = 512                        # elements a wave's load instruction covers
MAX_K = 64
LOG2E = 1.44269504088896340736
E = 2.0 ** -14
SEP = 8 * E
INF = float("inf")
FLAT = 2.0 ** 100                       # the hostile rows' temperature: every finite candidate's weight is 1
TS, KS = (0.5, 1.0, 2.0), (2, 5, 40, 64)
MARGIN_VS = (1016, 8200, 128256)


@pytest.fixture(scope="module")
def hip():
    from k8s_gpu_scheduler_amd import _native
    return _native.hip(required=True)


# ------------------------------------------------------------------------------------------------
# the references (also imported by test_sample_cpu.py)
# ------------------------------------------------------------------------------------------------
def boundary_indices(V):
    """Indices at the edges of the walk: the row's first and last column, a chunk's first and last element, a
    thread boundary (7 | 8), a wave boundary (511 | 512), a round boundary (8191 | 8192), and the same one and
    fifteen rounds in."""
    cand = [0, 7, 8, 15, 16, WAVE_ELEMS - 1, WAVE_ELEMS, WAVE_ELEMS + 7, ROUND - 8, ROUND - 1, ROUND, ROUND + 7,
            ROUND + WAVE_ELEMS - 1, ROUND + WAVE_ELEMS, 2 * ROUND - 1, 2 * ROUND, 15 * ROUND - 1, 15 * ROUND,
            15 * ROUND + WAVE_ELEMS, V // 2, V - 9, V - 8, V - 1]
    return sorted({i for i in cand if 0 <= i < V})


def ranking(row, k):
    """The k candidates of a row (1-D, no NaN) ranked by (value descending, index ascending): a stable sort on the
    values, for which +0.0 == -0.0."""
    assert not bool(row.isnan().any())
    return torch.sort(row.double(), descending=True, stable=True).indices[:k]


def clamp_k(top_k, V):
    return min(max(min(int(top_k), MAX_K), 1), V)


def reference_sample(row, u, temperature, top_k, top_p, order=None):
    """(token, separation) of one sampled row in float64: the contract with exact arithmetic in the place of fp32
    (order: ranking(row, 64), for callers that sample one row many times).
    separation: the distance of u * cum_{n-1} and of top_p * Z from the nearest cum_j, as a fraction of Z (the
    boundary cum_{k-1} == Z of top_p == 1 is exact in the kernel too and not counted)."""
    V = row.numel()
    assert row.dtype == BF and row.dim() == 1 and not bool(row.isnan().any())
    assert bool(row.float().max().isfinite()), "the maximum must be finite"
    assert 0 < temperature < INF and top_k != 1, "a greedy row has no reference here"
    assert 0 < top_p <= 1 and 0 <= u < 1
    k = clamp_k(top_k, V)
    c = ranking(row, k) if order is None else order[:k]
    l = row[c].double()
    a = (l - l[0]) * (LOG2E / float(temperature))
    assert bool((a >= -64).all()), "an exponent below -64: the error bound E does not cover it"
    cum = torch.exp2(a).cumsum(0)
    Z = cum[-1].item()
    cut = float(top_p) * Z
    n = int((cum >= cut).nonzero()[0]) + 1
    d = (cum - cut).abs() / Z
    if top_p == 1:
        d[k - 1] = INF
    target = float(u) * cum[n - 1].item()
    over = (cum[:n] > target).nonzero()
    assert len(over), "u < 1: some cum_j is above the target"
    j = int(over[0])
    sep = min(d.min().item(), ((cum[:n] - target).abs() / Z).min().item())
    return int(c[j]), sep


def f32(x):
    return torch.tensor(x, dtype=torch.float32).item()


def margin_rows(row, temperature, top_k, cut, order=None):
    """The (u, top_p) pairs that probe every kept rank of one row: top_p is 1 (cut False) or the fp32 midpoint
    between the cumulative fractions of ranks k // 2 - 1 and k // 2; u the fp32 midpoint of rank j's interval,
    for every j < n."""
    k = clamp_k(top_k, row.numel())
    l = row[ranking(row, k) if order is None else order[:k]].double()
    cum = torch.exp2((l - l[0]) * (LOG2E / temperature)).cumsum(0)
    Z = cum[-1].item()
    if cut:
        m = max(k // 2, 1)
        top_p = f32((cum[m - 1].item() + cum[min(m, k - 1)].item()) / 2 / Z)
    else:
        top_p = 1.0
    n = int((cum >= top_p * Z).nonzero()[0]) + 1
    edges = [0.0] + cum[:n].tolist()
    return [(f32((edges[j] + edges[j + 1]) / 2 / edges[n]), top_p) for j in range(n)]


@functools.lru_cache(maxsize=None)
def margin_case(V):
    """Every (T, top_k, top_p mode, kept rank) of a vocabulary as the rows of ONE launch: (base, which, u, temperature,
    top_k, top_p, tokens, separations) -- base bf16 [len(TS), V], which the base row of every launch row."""
    g = torch.Generator().manual_seed(9800 + V)
    base = torch.stack([(1.5 * T * torch.randn(V, generator=g)).to(BF) for T in TS])
    which, us, ts, ks, ps, toks, seps = [], [], [], [], [], [], []
    for i, T in enumerate(TS):
        order = ranking(base[i], MAX_K)
        for k in KS:
            for cut in (False, True):
                for u, p in margin_rows(base[i], T, k, cut, order):
                    tok, sep = reference_sample(base[i], u, T, k, p, order)
                    which.append(i), us.append(u), ts.append(T), ks.append(k), ps.append(p), toks.append(tok), seps.append(sep)
    return (base, torch.tensor(which), torch.tensor(us, dtype=torch.float32), torch.tensor(ts, dtype=torch.float32),
            torch.tensor(ks, dtype=torch.int32), torch.tensor(ps, dtype=torch.float32),
            torch.tensor(toks, dtype=torch.int32), torch.tensor(seps, dtype=torch.float64))


def plateau_row(V, where, h, background=-300.0):
    row = torch.full((V,), background).to(BF)
    row[torch.as_tensor(where)] = h
    assert (background - h) * LOG2E <= -150 and torch.equal(row.float().unique(), torch.tensor(sorted({background, h})))
    return row


def spread_indices(V, n, seed):
    """n distinct indices of [0, V), the boundary indices first, sorted."""
    b = boundary_indices(V)
    g = torch.Generator().manual_seed(seed)
    rest = [i for i in torch.randperm(V, generator=g).tolist() if i not in set(b)]
    return sorted((b + rest)[:n])


def staircase_row(V, seed):
    """64 values 3 binades (384 codes) apart from one another, 2^6 .. 2^-87 and -2^-87 .. -2^6, at spread indices in
    a shuffled order, over a crowd near -1000: the window walk has to cross the whole middle of the key space."""
    steps = [2.0 ** (6 - 3 * i) for i in range(32)] + [-(2.0 ** (-87 + 3 * i)) for i in range(32)]
    g = torch.Generator().manual_seed(seed)
    n = min(64, V)
    where = torch.tensor(spread_indices(V, n, seed))[torch.randperm(n, generator=g)]
    row = (-1000 - 50 * torch.rand(V, generator=g)).to(BF)
    row[where] = torch.tensor(steps[:n]).to(BF)
    keys = order_keys(row).sort(descending=True).values
    assert int((keys[:n - 1] - keys[1:n]).min()) > 256                               # also the top of the crowd, where there is one
    return row


def order_keys(row):
    """The 16-bit order keys of bf16 values (no NaN): code + 0x8000 without the sign bit, 0x10000 - code with it --
    monotonic in the value, +0.0 and -0.0 both 0x8000."""
    code = row.contiguous().view(torch.int16).int() & 0xFFFF
    return torch.where(code >= 0x8000, 0x10000 - code, code + 0x8000)


def hostile_rows(V, seed):
    """name -> row (bf16 [V]) for the selection's hard cases."""
    g = torch.Generator().manual_seed(seed)
    rows = {"staircase": staircase_row(V, seed)}
    crowd = (1.5 * torch.randn(V, generator=g)).to(BF)
    crowd[spread_indices(V, 1, seed + 1)[-1]] = 2.0 ** 20
    rows["one-over-a-crowd"] = crowd
    few = torch.full((V,), -INF).to(BF)
    keep = spread_indices(V, min(10, V - 1), seed + 2)
    few[torch.tensor(keep)] = (4 * torch.randn(len(keep), generator=g)).to(BF)
    rows["minus-inf-candidates"] = few
    rows["negative-only"] = (-1 - 3 * torch.randn(V, generator=g).abs()).to(BF)
    small = torch.tensor([0.0, -0.0, 2.0 ** -133, -(2.0 ** -133), 2.0 ** -126, -(2.0 ** -126), 2.0 ** -130, 1e-30, -1e-30])
    rows["around-zero"] = small[torch.randint(len(small), (V,), generator=g)].to(BF)
    return rows


def flat_expectation(row, k):
    """(tokens, u) of S = n identical rows at temperature FLAT, top_p 1: the n candidates of finite value in rank
    order, u_j = (j + 0.5) / n."""
    c = ranking(row, clamp_k(k, row.numel()))
    c = c[row[c].float().isfinite()]
    n = len(c)
    assert n >= 1 and bool((row.float()[c].abs() <= 2.0 ** 21).all())
    return c.to(torch.int32), ((torch.arange(n) + 0.5) / n).float()


# ------------------------------------------------------------------------------------------------
# guarded launches
# ------------------------------------------------------------------------------------------------
def vec(x, n, dtype):
    return x.to(dtype).cuda() if torch.is_tensor(x) else torch.full((n,), x, dtype=dtype, device="cuda")


class Launch:
    """logits [S, V] (host or device, possibly an expanded view) in a NaN-guarded window, out in a sentinel-guarded
    one; u, temperature, top_k, top_p tensors of length S or one value for every row."""

    def __init__(self, logits, u, temperature, top_k, top_p):
        self.S, self.V = logits.shape
        self.logits = guarded_input(logits.cuda(), self.V + C0, c0=C0)
        assert self.logits.data_ptr() % 16 == 0 and (self.S == 1 or self.logits.stride(0) == self.V + C0)
        self.u, self.t, self.p = (vec(x, self.S, torch.float32) for x in (u, temperature, top_p))
        self.k = vec(top_k, self.S, torch.int32)
        self.raw, self.out = self.new_output()

    def new_output(self):
        raw = torch.full((GB + self.S + GA,), SENT32, dtype=torch.int32, device="cuda")
        return raw, raw[GB:GB + self.S]

    def launch(self, out=None, **kw):
        from k8s_gpu_scheduler_amd.ops import loadgen
        return loadgen.sample_tokens(self.logits, self.u, self.t, self.k, self.p, out=self.out if out is None else out, **kw)

    def run(self, **kw):
        self.raw.fill_(SENT32)
        return self.launch(**kw)

    def tokens(self, raw=None):
        torch.cuda.synchronize()
        raw = (self.raw if raw is None else raw).cpu()
        assert bool((raw[:GB] == SENT32).all()) and bool((raw[GB + self.S:] == SENT32).all()), "write outside out's window"
        return raw[GB:GB + self.S]

    def check(self, exp, what, raw=None):
        got = self.tokens(raw)
        exp = torch.as_tensor(exp, dtype=torch.int32)
        bad = (got != exp).nonzero().flatten()
        if len(bad):
            r = int(bad[0])
            raise AssertionError((what, f"{len(bad)} of {self.S} tokens differ, first at row {r}: got {int(got[r])}, "
                                        f"expected {int(exp[r])}"))


def rows_of(row, n):
    return row.cuda()[None, :].expand(n, -1)


# ------------------------------------------------------------------------------------------------
# 1. shapes
# ------------------------------------------------------------------------------------------------
def test_the_shapes_cover_the_walk():
    chunks = {v: v // 8 for v in VS}
    assert all(v % 8 == 0 and 8 <= v <= 131072 for v in VS)
    assert any(v < MAX_K for v in VS) and MAX_K in VS                               # fewer elements than candidates; exactly as many
    assert any(c < THREADS and c % 64 for c in chunks.values())                      # a ragged last chunk inside the first round
    assert any(c == THREADS for c in chunks.values()) and any(c == THREADS + 1 for c in chunks.values())
    assert any(c // THREADS == 15 and c % THREADS for c in chunks.values())          # 15 full rounds and a partial one
    assert any(c == 16 * THREADS for c in chunks.values())                           # the cap
    assert 128256 in VS
    for v in VS:
        b = boundary_indices(v)
        assert b[0] == 0 and b[-1] == v - 1 and all(0 <= i < v for i in b)
    b = boundary_indices(131072)
    assert {7, 8, 511, 512, 8191, 8192, 15 * 8192 - 1, 15 * 8192}.issubset(b)


# ------------------------------------------------------------------------------------------------
# 2. greedy
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def greedy_case(V):
    """Rows with the maximum planted at every boundary index, rows with it repeated, rows whose maximum is a tie of
    +0.0 and -0.0; every row twice: temperature 0 (top_k 50) and top_k 1 (temperature 1)."""
    g = torch.Generator().manual_seed(9700 + V)
    b = boundary_indices(V)
    rows, exp = [], []
    for i in b:
        r = torch.randn(V, generator=g).to(BF)
        r[i] = 100.0
        rows.append(r), exp.append(i)
    for lo in range(0, len(b) - 1, 3):                                               # the maximum at several indices
        r = torch.randn(V, generator=g).to(BF)
        r[torch.tensor(b[lo:])] = 7.5
        rows.append(r), exp.append(b[lo])
    for first, second in ((0.0, -0.0), (-0.0, 0.0)):                                 # +0.0 == -0.0: the lowest index wins
        if len(b) < 3:
            continue
        r = (-1 - torch.randn(V, generator=g).abs()).to(BF)
        r[b[1]], r[b[-2]] = first, second
        if b[1] != b[-2]:
            rows.append(r), exp.append(b[1])
    logits = torch.stack(rows + rows)
    n = len(rows)
    t = torch.tensor([0.0] * n + [1.0] * n)
    k = torch.tensor([50] * n + [1] * n)
    return Launch(logits, NAN, t, k, NAN), torch.tensor(exp + exp)


@pytest.mark.parametrize("V", VS)
def test_greedy(hip, V):
    c, exp = greedy_case(V)
    c.run()                                                                          # check=True: u and top_p are NaN
    c.check(exp, ("greedy", V))


# ------------------------------------------------------------------------------------------------
# 3. plateaus
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("h", (0.5, -3.0))
def test_plateau_larger_than_k(hip, V, h):
    """k <= n: S = k identical rows, u_j = (j + 0.5) / k, must give the plateau's k lowest indices in order."""
    n = min(70, V)
    where = spread_indices(V, n, 9600 + V)
    row = plateau_row(V, where, h) if n < V else torch.full((V,), h).to(BF)
    for k in (5, 64):
        kk = clamp_k(k, V)
        c = Launch(rows_of(row, kk), (torch.arange(kk) + 0.5) / kk, 1.0, k, 1.0)
        c.run()
        c.check(where[:kk], ("plateau", V, h, k))


@pytest.mark.parametrize("V", VS[1:])
def test_plateau_smaller_than_k(hip, V):
    """k > n: every u lands on the plateau, u close to 1 on its last index, never on a background index."""
    n = 10
    where = spread_indices(V, n, 9650 + V)[-n:] if V > 64 else list(range(V - n, V))
    row = plateau_row(V, where, 2.0)
    u = torch.cat([(torch.arange(n) + 0.5) / n, torch.tensor([1 - 2.0 ** -24, 1 - 2.0 ** -12])])
    c = Launch(rows_of(row, n + 2), u, 1.0, 64, 1.0)
    c.run()
    c.check(where + [where[-1]] * 2, ("plateau below k", V))


@pytest.mark.parametrize("V", VS)
def test_a_whole_row_of_one_value(hip, V):
    k = min(64, V)
    for value in (1.25, -0.0, -77.0):
        c = Launch(rows_of(torch.full((V,), value).to(BF), k), (torch.arange(k) + 0.5) / k, 1.0, 64, 1.0)
        c.run()
        c.check(list(range(k)), ("one value", V, value))


# ------------------------------------------------------------------------------------------------
# 4. hostile rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", VS)
def test_selection_on_hostile_rows(hip, V):
    for name, row in hostile_rows(V, 9500 + V).items():
        for k in (64, 7):
            exp, u = flat_expectation(row, k)
            c = Launch(rows_of(row, len(exp)), u, FLAT, k, 1.0)
            c.run()
            c.check(exp, ("hostile", name, V, k))


# ------------------------------------------------------------------------------------------------
# 5. the margin regime
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", MARGIN_VS)
def test_margin_regime(hip, V):
    base, which, u, t, k, p, tokens, seps = margin_case(V)
    assert bool((seps >= SEP).all()), (V, seps.min().item())                          # a condition on the inputs
    c = Launch(base.cuda()[which.cuda()], u, t, k, p)
    c.run()
    got = c.tokens()
    same = int((got == tokens).sum())
    print(f"sample, margin regime V = {V}: {same} of {len(tokens)} tokens match; smallest separation 2^{seps.min().log2().item():.2f} of Z"
          f" (required 2^{torch.tensor(SEP).log2().item():.0f})")
    c.check(tokens, ("margin", V))


# ------------------------------------------------------------------------------------------------
# 6. degenerate rows, the clamp
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", (8, 1016, 8200, 131072))
def test_degenerate_rows_touch_only_themselves(hip, V):
    g = torch.Generator().manual_seed(9400 + V)
    b = boundary_indices(V)
    clean = (1.5 * torch.randn(V, generator=g)).to(BF)
    u, _ = margin_rows(clean, 1.0, 5, False)[1]                                      # rank 1's midpoint
    want, sep = reference_sample(clean, u, 1.0, 5, 1.0)
    top = int(ranking(clean, 1)[0])
    assert sep >= SEP and want != top
    rows, exp = [], []                                                               # exp: a token, or None for a clean row
    for i in b:                                                                      # a NaN at a boundary index, a clean neighbour
        r = clean.clone()
        r[i] = NAN
        rows += [r, clean]
        exp += [-1, None]
    rows += [torch.full((V,), -INF).to(BF), clean]
    exp += [-1, None]
    r = clean.clone()
    r[torch.tensor(b[1:])] = INF                                                     # +Inf: its lowest index
    rows.append(r), exp.append(b[1])
    r = clean.clone()
    r[b[-1]], r[b[0]] = INF, -INF
    rows += [r, clean]
    exp += [b[-1], None]
    logits = torch.stack(rows)
    for t, k in ((1.0, 5), (0.0, 5), (1.0, 1)):                                      # sampled, and both greedy forms
        c = Launch(logits, u, t, k, 1.0)
        c.run()
        c.check([(want if t and k != 1 else top) if x is None else x for x in exp], ("degenerate", V, t, k))


def test_top_k_is_clamped_in_the_kernel(hip):
    V = 8200
    where = spread_indices(V, 70, 9300)
    row = plateau_row(V, where, 1.0)
    ks = torch.tensor([0, -5, 65, 2 ** 31 - 1, 1, 64, -2 ** 31, 1000])
    c = Launch(rows_of(row, len(ks)), 63.5 / 64, 1.0, ks, 1.0)
    with pytest.raises(ValueError, match="top_k"):
        c.run()                                                                      # check=True refuses them
    assert bool((c.tokens() == SENT32).all())
    c.run(check=False)
    c.check([where[0], where[0], where[63], where[63], where[0], where[63], where[0], where[63]], "clamp")


# ------------------------------------------------------------------------------------------------
# 7. other launch paths
# ------------------------------------------------------------------------------------------------
def test_two_launches_and_graph_replays_are_identical(hip):
    V = 128256
    base, which, u, t, k, p, tokens, _ = margin_case(V)
    c = Launch(base.cuda()[which.cuda()], u, t, k, p)
    a, b = c.new_output(), c.new_output()
    c.launch(out=a[1])
    c.launch(out=b[1])
    assert torch.equal(c.tokens(a[0]), c.tokens(b[0]))
    c.check(tokens, "second output", b[0])
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        c.launch(stream=s, check=False)
    for r in range(3):
        if r != 1:                       # the second replay writes over the first: idempotent
            c.raw.fill_(SENT32)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        s.synchronize()
        c.check(tokens, ("replay", r))


@pytest.mark.parametrize("breakage", ["fp64-logits", "int64-top_k", "odd-V", "big-V", "odd-stride", "misaligned", "short-u",
                                      "out-dtype", "out-overlaps", "bad-top_p", "bad-u", "bad-temperature"])
def test_a_bad_call_raises_and_launches_nothing(hip, breakage):
    from k8s_gpu_scheduler_amd.ops import loadgen
    V = 1016
    row = plateau_row(V, spread_indices(V, 70, 9301), 1.0)
    c = Launch(rows_of(row, 3), 0.5, 1.0, 5, 1.0)
    lg, u, t, k, p, out = c.logits, c.u, c.t, c.k, c.p, c.out
    if breakage == "fp64-logits":
        lg = lg.double()
    elif breakage == "int64-top_k":
        k = k.long()
    elif breakage == "odd-V":
        lg = lg[:, :V - 4]
    elif breakage == "big-V":
        lg = torch.zeros(1, 131080, dtype=BF, device="cuda").expand(3, -1)
    elif breakage == "odd-stride":
        lg = torch.zeros(3, V + 4, dtype=BF, device="cuda")[:, :V]
    elif breakage == "misaligned":
        lg = torch.zeros(3 * V + 8, dtype=BF, device="cuda")[4:4 + 3 * V].view(3, V)
    elif breakage == "short-u":
        u = u[:2]
    elif breakage == "out-dtype":
        out = torch.zeros(3, dtype=torch.int64, device="cuda")
    elif breakage == "out-overlaps":
        out = k
    elif breakage == "bad-top_p":
        p = torch.tensor([1.0, 0.0, 1.0], device="cuda")
    elif breakage == "bad-u":
        u = torch.tensor([0.5, 0.5, 1.0], device="cuda")
    else:
        t = torch.tensor([1.0, INF, 1.0], device="cuda")
    c.raw.fill_(SENT32)
    with pytest.raises((ValueError, TypeError)):
        loadgen.sample_tokens(lg, u, t, k, p, out=out)
    assert bool((c.tokens() == SENT32).all())


def test_workgroups_match_the_python_rule(hip):
    from k8s_gpu_scheduler_amd.models import workloads as W
    for S in (0, 1, 8, 256, 4096, 2 ** 31 - 1):
        assert hip.sample_workgroups(S) == W.default_sample_workgroups(S) == S
    with pytest.raises(RuntimeError):
        hip.sample_workgroups(-1)


# ------------------------------------------------------------------------------------------------
# 8. row offsets beyond 4 GiB
# ------------------------------------------------------------------------------------------------
BIG_LD = 2 ** 30


def test_row_offsets_beyond_4_gib(hip):
    """3 rows of 1,016 logits at a row stride of 2^30 elements inside one UNINITIALISED allocation of which only
    the three windows are written: the last row starts past 4 GiB."""
    from k8s_gpu_scheduler_amd.ops import loadgen
    S, V = 3, 1016
    g = torch.Generator().manual_seed(9302)
    host = (1.5 * torch.randn(S, V, generator=g)).to(BF)
    exp, us = [], []
    for r in range(S):
        u, _ = margin_rows(host[r], 1.0, 40, False)[3 * r + 1]
        tok, sep = reference_sample(host[r], u, 1.0, 40, 1.0)
        assert sep >= SEP
        exp.append(tok), us.append(u)
    raw = torch.empty(((S - 1) * BIG_LD + V + 2 * C0,), dtype=torch.int16, device="cuda")
    logits = raw.view(BF).as_strided((S, V), (BIG_LD, 1), C0)
    assert 2 * BIG_LD * 2 >= 2 ** 32 and logits.data_ptr() % 16 == 0
    logits.copy_(host.cuda())
    c = Launch(host, torch.tensor(us), 1.0, 40, 1.0)
    c.raw.fill_(SENT32)
    loadgen.sample_tokens(logits, c.u, c.t, c.k, c.p, out=c.out)
    c.check(exp, "row stride 2^30")
    del raw, logits
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------
# 9. beside a co-running load
# ------------------------------------------------------------------------------------------------
class SampleLaunch:
    """One launch on a Launch's inputs into an output of its own (reset / enqueue / check, as the co-run module's
    CaseLaunch has)."""

    def __init__(self, c, exp, what):
        self.c, self.exp, self.what = c, exp, what
        self.raw, self.out = c.new_output()

    def reset(self):
        self.raw.fill_(SENT32)

    def enqueue(self, st):
        self.c.launch(out=self.out, stream=st, check=False)

    def check(self, tag):
        self.c.check(self.exp, (tag, self.what), self.raw)


@pytest.mark.parametrize("aggressor,mode", [pytest.param(a, m, id=f"{a}-{m}") for a, m in CO.BASE_PAIRS])
def test_sample_corun(hip, aggressor, mode):
    """The margin regime's launch of the real vocabulary, the same tokens while another stream runs GEMMs or triads."""
    base, which, u, t, k, p, tokens, _ = margin_case(128256)
    c = Launch(base.cuda()[which.cuda()], u, t, k, p)
    victim = CO.Load("sample-margin", {}, [SampleLaunch(c, tokens, ("margin", 128256, r)) for r in range(CO.R)])
    try:
        CO.corun(hip, victim, CO.aggressor_for(aggressor, mode), mode)
    finally:
        CO.restore_knobs(hip)


# ------------------------------------------------------------------------------------------------
# 10. pod path
# ------------------------------------------------------------------------------------------------
def admitted_rows(logits, u, temperature, top_k, top_p):
    """(rows, tokens): the rows of the executor's sample operands (host tensors) whose u and top_p keep the
    separation, and their reference tokens."""
    rows, toks = [], []
    for r in range(logits.shape[0]):
        tok, sep = reference_sample(logits[r], u[r].item(), temperature[r].item(), int(top_k[r]), top_p[r].item())
        if sep >= SEP:
            rows.append(r), toks.append(tok)
    return torch.tensor(rows), torch.tensor(toks, dtype=torch.int32)


@pytest.mark.parametrize("workload", ["llm_head_decode_8", "llm_head_decode_256"])
def test_executor_llm_head_tokens(hip, workload):
    """One iteration of the workload through _Buffers + enqueue_ops; the sample op's tokens against the reference
    on the rows the separation admits (fewer than 1/4 may be left out)."""
    from k8s_gpu_scheduler_amd.models import workloads as W
    from k8s_gpu_scheduler_amd.parallel.executor import _Buffers, enqueue_ops, op_output
    dev = torch.device("cuda", 0)
    t0 = time.time()
    a = _Buffers(W.get(workload), dev)
    t_build = time.time() - t0
    (o, t), = [(o, t) for o, t in a.ops if o.kind == "sample"]
    out, logits, u, temperature, top_k, top_p = t
    assert a.ops[2][0] is o and op_output(o, t) is out
    assert logits.shape == (o.M, o.N) and logits.dtype == BF and out.shape == (o.M,) and out.dtype == torch.int32
    out.fill_(SENT32)
    enqueue_ops(a, 1, torch.cuda.current_stream(), 0)
    torch.cuda.synchronize()
    rows, toks = admitted_rows(logits.cpu(), u.cpu(), temperature.cpu(), top_k.cpu(), top_p.cpu())
    got = out.cpu()
    left_out = o.M - len(rows)
    print(f"{workload}: operands built in {t_build:.1f} s; {len(rows)} of {o.M} rows admitted, {left_out} left out; "
          f"{int((got[rows] == toks).sum())} of {len(rows)} tokens match")
    assert torch.equal(got[rows], toks)
    assert bool(((got >= 0) & (got < o.N)).all())                                    # every row was written with a token
    gemm_out = op_output(*a.ops[1])
    assert bool(gemm_out.float().isfinite().all()) and bool(op_output(*a.ops[0]).float().isfinite().all())
    del a, t, out, logits, gemm_out
    torch.cuda.empty_cache()
    assert 4 * left_out < o.M, f"{left_out} of {o.M} rows are closer than 8 E to a boundary"
