"""Exact-input probes for the GEMM and attention kernels (a plain helper module, imported like gpu_util).

The inputs are chosen so that the exact result is known and representable: small integers (the counting regime) or
dyadic fractions i/8, j/16 (the dyadic regime) for the GEMMs, saturated softmax rows for attention.  fp32 accumulation of
such inputs is exact in any order, so a kernel must reproduce the fp64 result, cast once with round-to-nearest-even,
bit for bit; one dropped, doubled or misplaced product changes an integer by at least 1.  Everything here is plain torch
on whatever device the tensors live on: tests/test_exact_probes_cpu.py checks the generators and the checkers themselves.
"""
import itertools
import math

import torch

BF = torch.bfloat16
GUARD_ROWS = 256      # rows of sentinel behind every output: a 256-row tile that overruns M lands in them
BF_SENTINEL = 0x7FC1  # quiet NaNs with a payload no kernel produces: an unwritten element can never pass
F32_SENTINEL = 0x7FC00ABC
EXACT_LIMIT = 2.0 ** 24


def gpu():
    """gpu_util (raw C-ABI calls), imported only by the GPU tests that call it"""
    import gpu_util
    return gpu_util


def collect(cases, fn, label=""):
    """run fn(case) for every case and report every failing one in one message"""
    fails = []
    for c in cases:
        try:
            fn(c)
        except AssertionError as e:
            fails.append(f"{label}{c}: {e}")
    assert not fails, f"{len(fails)} of {len(cases)} cases failed:\n" + "\n".join(fails[:12])


def gen(seed, device="cpu"):
    return torch.Generator(device=device).manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------- inputs
def counting(shape, g, lo=-1, hi=1, density=1.0):
    """integers uniform in [lo, hi] (fp64, on the generator's device); each kept with probability `density` (else 0)"""
    x = torch.randint(lo, hi + 1, shape, generator=g, device=g.device).double()
    if density < 1.0:
        x = x * (torch.rand(shape, generator=g, device=g.device) < density).double()
    return x


def dyadic(shape, g, den, lim, density=1.0):
    """i / den with i uniform in [-lim, lim]"""
    return counting(shape, g, -lim, lim, density) / den


def check_exact_gemm(A, B, extra=(), out_dtype=BF, what="gemm"):
    """preconditions of a bitwise GEMM check, C = A @ B + sum(extra):
    every partial sum, in any order, stays below 2^24 in magnitude (so fp32 accumulation is exact), and for a bf16
    output every result is exactly representable (|y| <= 256 for integers).  Returns the fp64 result."""
    A, B = A.double(), B.double()
    bound = A.abs() @ B.abs()
    for e in extra:
        bound = bound + e.double().abs()
    assert float(bound.max()) < EXACT_LIMIT, f"{what}: a partial sum can reach {float(bound.max())} >= 2^24"
    y = A @ B
    for e in extra:
        y = y + e.double()
    assert torch.equal(y, y.float().double()), f"{what}: result not exact in fp32"
    if out_dtype == BF:
        assert torch.equal(y, y.to(BF).double()), f"{what}: result not exactly representable in bf16 (max |y| {float(y.abs().max())})"
    return y


# ------------------------------------------------------------------------------------------------------- expectations
def rne(x64, dtype):
    """fp64 -> dtype with ONE round-to-nearest-even.  bf16 goes through fp32, which is exact for every value it is given here
    (asserted): a double rounding would otherwise hide in it."""
    x64 = x64.double()
    x32 = x64.float()
    if dtype == torch.float32:
        return x32
    assert torch.equal(x32.double(), x64), "rne: value not exact in fp32 (double rounding)"
    return x32.to(dtype)


def bits(t):
    """integer bit patterns; -0 folded onto +0 (the sign of an exact zero sum depends on the accumulator's start value)"""
    t = t.detach().contiguous()
    if t.dtype == BF:
        b = t.view(torch.int16).int() & 0xFFFF
        return torch.where(b == 0x8000, torch.zeros_like(b), b)
    if t.dtype == torch.float32:
        b = t.view(torch.int32).long() & 0xFFFFFFFF
        return torch.where(b == 0x80000000, torch.zeros_like(b), b)
    if t.dtype == torch.uint8:
        return t.int()
    raise TypeError(t.dtype)


def assert_bitwise(got, want, what):
    """got == want bit for bit (want already in got's dtype)"""
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    bad = bits(got) != bits(want.to(got.device))
    n = int(bad.sum())
    if n:
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what}: {n} of {bad.numel()} elements differ; first at {idx}: got {float(got[idx])!r} "
                             f"want {float(want[idx])!r}")


def bf16_ulp(x64):
    """spacing of bf16 at |x| (normal range; the subnormal spacing below 2^-126)"""
    e = torch.floor(torch.log2(x64.abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, e - 7)


def assert_ulps(got, ref64, what, ulps=1.0, floor=0.0):
    """|got - ref| <= ulps * ulp_bf16(ref) + floor, elementwise, ref in fp64"""
    got64 = got.detach().double().to(ref64.device)
    assert got64.shape == ref64.shape, (what, tuple(got64.shape), tuple(ref64.shape))
    err = (got64 - ref64).abs()
    lim = ulps * bf16_ulp(ref64) + floor
    bad = ~(err <= lim)
    n = int(bad.sum())
    if n:
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what}: {n} of {bad.numel()} elements off by more than {ulps} bf16 ulp; first at {idx}: "
                             f"got {float(got64[idx])!r} want {float(ref64[idx])!r}")


# ------------------------------------------------------------------------------------------------------------ canaries
def guarded(rows, cols, dtype, device, guard=GUARD_ROWS):
    """[rows + guard, cols] filled with the sentinel; the kernel gets buf[:rows]"""
    if dtype == BF:
        return torch.full((rows + guard, cols), BF_SENTINEL, dtype=torch.int16, device=device).view(BF)
    if dtype == torch.float32:
        return torch.full((rows + guard, cols), F32_SENTINEL, dtype=torch.int32, device=device).view(torch.float32)
    if dtype == torch.uint8:
        return torch.full((rows + guard, cols), 0xA5, dtype=torch.uint8, device=device)
    raise TypeError(dtype)


def sentinel_bits(dtype):
    return {BF: BF_SENTINEL, torch.float32: F32_SENTINEL, torch.uint8: 0xA5}[dtype]


def assert_guard(buf, rows, what):
    """the guard rows behind `rows` still hold the sentinel"""
    g = bits(buf[rows:]) != sentinel_bits(buf.dtype)
    n = int(g.sum())
    if n:
        idx = tuple(int(i) for i in g.nonzero()[0])
        raise AssertionError(f"{what}: {n} guard elements overwritten; first at row {rows + idx[0]} col {idx[1]}")


def assert_written(buf, rows, what):
    """no in-range element still holds the sentinel"""
    s = bits(buf[:rows]) == sentinel_bits(buf.dtype)
    n = int(s.sum())
    if n:
        idx = tuple(int(i) for i in s.nonzero()[0])
        raise AssertionError(f"{what}: {n} elements never written; first at {idx}")


# ---------------------------------------------------------------------------------------- saturated-softmax attention
CODE = 64.0  # the key code c (e_a + e_b): target score 2 c^2, every other score <= c^2
MIN_GAP = 110.0  # c^2 * scale >= 110: exp(-gap) underflows to 0 in fp32 even with denormals (e^-103.3 is the last one)


class AttnProbe:
    """one saturated-softmax probe of B images x H heads x S tokens (head dim HE), with its exact consequences.

    kind: 'perm'   query q carries the code of key pi(q): O[q] = V[pi(q)], dQ = dK = 0
          'tie2'   key `ties[1]` duplicates the code of key `ties[0]`: the queries on that code see a 2-way tie
          'tie4'   four keys share one code (4-way tie); with either tie, query 0 carries the tied code
          'sum'    some queries carry the sum of two keys' codes (4 distinct dims, no third key inside them): nonzero dQ
    P is the exact softmax (1/t on the t tied maxima, 0 elsewhere); everything else follows from it in fp64."""

    def __init__(self, B, H, S, HE, kind="perm", ties=None, seed=0, vlim=3, dolim=1):
        assert S >= 1 and HE >= 4
        self.B, self.H, self.S, self.HE, self.kind = B, H, S, HE, kind
        g = gen(seed * 7919 + S * 131 + HE)
        pairs = torch.tensor(list(itertools.combinations(range(HE), 2)))
        assert len(pairs) >= S, "not enough codes"
        Q = torch.zeros(B, H, S, HE, dtype=torch.float64)
        K = torch.zeros(B, H, S, HE, dtype=torch.float64)
        keys = torch.arange(S)
        self.designed = torch.zeros(B, H, S, S, dtype=torch.bool)  # [b, h, q, k]: key k is one of query q's maxima by design
        tied = kind in ("tie2", "tie4") and S >= len(ties)
        for b in range(B):
            for h in range(H):
                sel = torch.randperm(len(pairs), generator=g)[:S]
                if tied:
                    sel[list(ties[1:])] = sel[ties[0]].clone()
                kp = pairs[sel]  # key k's two dims
                K[b, h, keys, kp[:, 0]] = CODE
                K[b, h, keys, kp[:, 1]] = CODE
                pi = torch.randperm(S, generator=g)
                Q[b, h] = K[b, h, pi]
                self.designed[b, h, keys, pi] = True
                if tied:
                    Q[b, h, 0] = K[b, h, ties[0]]  # query 0 (the CLS row) is always on the tie
                    on_tie = [q for q in range(S) if q == 0 or int(pi[q]) in ties]
                    self.designed[b, h, on_tie] = False
                    for q in on_tie:
                        self.designed[b, h, q, list(ties)] = True
                if kind == "sum":
                    for q, a, c in self._sum_queries(Q[b, h], [tuple(p) for p in kp.tolist()], g):
                        self.designed[b, h, q] = False
                        self.designed[b, h, q, [a, c]] = True
        self.V = counting((B, H, S, HE), g, -vlim, vlim)
        self.dO = counting((B, H, S, HE), g, -dolim, dolim)
        self.Q, self.K = Q, K
        self.qkv = torch.cat([self.flat(t) for t in (Q, K, self.V)], 1)

    @staticmethod
    def _sum_queries(Qh, kp, g):
        """replace up to S/4 queries by code_a + code_b for key pairs (a, b) on 4 distinct dims whose 4 cross pairs are
        nobody's code (so only a and b reach 2 c^2); returns the (query, a, b) triples"""
        S = len(kp)
        used = set(kp)
        order = torch.randperm(S, generator=g).tolist()
        nq, made = 0, []
        for a, b in itertools.combinations(order, 2):
            if nq >= max(1, S // 4):
                break
            (i, j), (k, l) = kp[a], kp[b]
            if len({i, j, k, l}) < 4:
                continue
            if any(tuple(sorted(p)) in used for p in ((i, k), (i, l), (j, k), (j, l))):
                continue
            Qh[nq].zero_()
            Qh[nq, [i, j, k, l]] = CODE
            made.append((nq, a, b))
            nq += 1
        return made

    # ---- exact consequences
    def scores(self):
        return self.Q @ self.K.transpose(-1, -2)  # exact integers (fp64)

    def P(self):
        s = self.scores()
        top = s == s.amax(-1, keepdim=True)
        return top.double() / top.sum(-1, keepdim=True)

    def ties_per_query(self):
        s = self.scores()
        return (s == s.amax(-1, keepdim=True)).sum(-1)

    def forward(self):
        P = self.P()
        return P @ self.V

    def backward(self, scale, dO=None):
        dO = self.dO if dO is None else dO
        P = self.P()
        O = P @ self.V
        dV = P.transpose(-1, -2) @ dO
        dP = dO @ self.V.transpose(-1, -2)
        D = (dO * O).sum(-1, keepdim=True)
        dS = P * (dP - D)
        dQ = scale * dS @ self.K
        dK = scale * dS.transpose(-1, -2) @ self.Q
        return dQ, dK, dV, dS

    def lse_exact(self, scale, queries=slice(None)):
        """fp32 m (the kernels' scale * score in fp32) and log t of each query's t-way tie, [B, H, len(queries)]"""
        m = torch.tensor(2 * CODE * CODE, dtype=torch.float32) * torch.tensor(scale, dtype=torch.float32)
        s = self.scores()[:, :, queries]
        top = s.amax(-1)
        assert bool((top == 2 * CODE * CODE).all()), "every query's maximum is 2 c^2"
        return m.double(), torch.log((s == top.unsqueeze(-1)).sum(-1).double())

    def flat(self, t):
        """[B, H, S, HE] -> [B*S, H*HE] (the kernels' row layout)"""
        return t.permute(0, 2, 1, 3).reshape(self.B * self.S, self.H * self.HE)

    def check_preconditions(self, scales):
        """every query's maximum is 2 c^2 and its maxima are exactly the designed keys (its target, the designed tie or the
        pair it is the sum of: no unintended tie anywhere), every other score is far enough below
        it that its exp underflows to 0 in fp32 at each scale, and the backward's dS is exact in bf16"""
        s = self.scores()
        top = s.amax(-1, keepdim=True)
        assert bool((top == 2 * CODE * CODE).all()), "a query's maximum is not 2 c^2"
        rest = torch.where(s == top, torch.full_like(s, -1.0), s).amax(-1)  # scores are >= 0: -1 marks "no other key"
        for scale in scales:
            gap = (top.squeeze(-1) - rest) * scale
            if bool((rest >= 0).any()):
                assert float(gap[rest >= 0].min()) >= MIN_GAP, f"score gap {float(gap[rest >= 0].min())} < {MIN_GAP} at scale {scale}"
        wrong = (s == top) != self.designed
        if bool(wrong.any()):
            b, h, q, k = (int(v) for v in wrong.nonzero()[0])
            raise AssertionError(f"query {q} of head ({b}, {h}): key {k} is {'not ' if self.designed[b, h, q, k] else ''}"
                                 f"a maximum, against the design")
        dP = self.dO @ self.V.transpose(-1, -2)
        spread = float((dP.amax(-1) - dP.amin(-1)).max())
        assert spread <= 256, f"|dO.(V_a - V_b)| reaches {spread} > 256: dS would not survive its bf16 packing"
        dS = self.backward(1.0)[3]
        assert torch.equal(dS, dS.to(BF).double()), "dS not exact in bf16"

    def check_fp8_preconditions(self):
        """the fp8 (OCP e4m3) kernels quantise Q and K for the scores and 256 p and V for P.V: every one of those values
        survives the round trip through e4m3 here, so every fp8 product and fp32 sum is exact and the mode-0 expectations
        hold bit for bit"""
        assert_e4m3_exact(self.Q, "Q")
        assert_e4m3_exact(self.K, "K")
        assert_e4m3_exact(self.V, "V")
        assert_e4m3_exact(256.0 * self.P(), "256 p")


def e4m3(x):
    """x (any float dtype) rounded to OCP e4m3 and back, in x's dtype"""
    return x.float().to(torch.float8_e4m3fn).float().to(x.dtype)


def assert_e4m3_exact(x, what):
    bad = e4m3(x) != x
    if bool(bad.any()):
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what}: {float(x[idx])!r} at {idx} does not survive the round trip through e4m3")


def assert_lse(got, m, logt, what):
    """LSE of a saturated probe: exactly m (fp32, as fp64) where the query has one maximum (log t = 0), m + log t within
    one fp32 ulp on a t-way tie"""
    got = got.detach().double().cpu()
    want = m + logt
    ulp = torch.pow(2.0, torch.floor(torch.log2(want.abs())) - 23)
    bad = torch.where(logt == 0, got != want, ~((got - want).abs() <= ulp))
    n = int(bad.sum())
    if n:
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {n} LSE values wrong; first at {i}: got {float(got[i])!r} want {float(want[i])!r}")


def assert_bitwise_or_slack(got, want64, slack, what):
    """got == rne(want) bit for bit wherever want is nonzero; where want is exactly 0, |got| <= slack (elementwise, fp64;
    slack 0 demands an exact zero)"""
    got64 = got.detach().double().cpu()
    want = rne(want64, got.dtype).double()
    assert got64.shape == want.shape, (what, tuple(got64.shape), tuple(want.shape))
    bad = torch.where(want64 != 0, got64 != want, ~(got64.abs() <= slack))
    n = int(bad.sum())
    if n:
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what}: {n} of {bad.numel()} elements differ; first at {idx}: got {float(got64[idx])!r} "
                             f"want {float(want64[idx])!r} (slack {float(slack[idx]) if torch.is_tensor(slack) else slack!r})")


# ------------------------------------------------------------------------- saturated softmax of L2-distance scores
DO_NZ = 8  # expected nonzeros of a dO row in an L2Probe (see its docstring)
class L2Probe:
    """the saturated-softmax probe of the L2-distance kernels, scores = +|q - k| * scale (mode 1 of csrc/attention.hip).

    Key k carries c (e_a + e_b + e_c + e_d) on a distinct 4-subset of the head dims and query q carries -K[pi(q)], so
    |q|^2 = |k|^2 = 4 c^2 and q . k_target = -4 c^2: the kernel's qn + kn - 2 qk is 16 c^2 and its root exactly 4 c.  A key
    sharing j <= 3 dims with the target is at c sqrt(8 + 2 j) <= c sqrt(14), (4 - sqrt(14)) c scale below the maximum.
    kind: 'perm'  O[q] = V[pi(q)], dS = 0, so dQ = dK = 0
          'tie2' / 'tie4'  the keys `ties` share one code (query 0 always carries it): P = 1/t on them, dK nonzero on the
          tied keys; q - k is the same vector for every tied key of a query and sum_k dS = 0, so dQ = 0.
    There is no 'sum' kind (a query at equal distance from two distinct codes would need 20 c^2 to be a square): a nonzero
    dQ is covered by the element-wise budget of tests/attn_modes_ref.py.  Everything is fp64 and exact.  dO is sparse (about
    do_nonzeros of the HE entries of a row are +-1): dK on a tied key is 2 c colsum(W) = sum_q (dP - delta) / t, which a dense
    dO pushes past the 8 significant bits of bf16."""

    def __init__(self, B, H, S, HE, kind="perm", ties=None, seed=0, code=CODE, vlim=3, dolim=1, do_nonzeros=DO_NZ):
        assert S >= 1 and HE >= 8
        self.B, self.H, self.S, self.HE, self.kind, self.code = B, H, S, HE, kind, float(code)
        g = gen(seed * 7919 + S * 131 + HE + 5)
        Q = torch.zeros(B, H, S, HE, dtype=torch.float64)
        K = torch.zeros(B, H, S, HE, dtype=torch.float64)
        keys = torch.arange(S)
        self.designed = torch.zeros(B, H, S, S, dtype=torch.bool)  # [b, h, q, k]: key k is one of query q's maxima by design
        tied = kind in ("tie2", "tie4") and S >= len(ties)
        for b in range(B):
            for h in range(H):
                sub = self._subsets(S, HE, g)
                if tied:
                    sub[list(ties[1:])] = sub[ties[0]].clone()
                K[b, h, keys.unsqueeze(1), sub] = self.code
                pi = torch.randperm(S, generator=g)
                Q[b, h] = -K[b, h, pi]
                self.designed[b, h, keys, pi] = True
                if tied:
                    Q[b, h, 0] = -K[b, h, ties[0]]
                    on_tie = [q for q in range(S) if q == 0 or int(pi[q]) in ties]
                    self.designed[b, h, on_tie] = False
                    for q in on_tie:
                        self.designed[b, h, q, list(ties)] = True
        self.V = counting((B, H, S, HE), g, -vlim, vlim)
        self.dO = counting((B, H, S, HE), g, -dolim, dolim, min(1.0, do_nonzeros / HE))
        self.Q, self.K = Q, K
        self.qkv = torch.cat([self.flat(t) for t in (Q, K, self.V)], 1)

    @staticmethod
    def _subsets(S, HE, g):
        """S distinct sorted 4-subsets of range(HE), [S, 4]"""
        seen, rows = set(), []
        while len(rows) < S:
            cand = torch.rand(2 * S + 8, HE, generator=g).argsort(-1)[:, :4].sort(-1).values
            for r in cand.tolist():
                if tuple(r) not in seen and len(rows) < S:
                    seen.add(tuple(r))
                    rows.append(r)
        return torch.tensor(rows)

    flat = AttnProbe.flat

    # ---- exact consequences
    def dist2(self):
        """|q - k|^2 as the kernel forms it, qn + kn - 2 qk: exact integers (fp64), [B, H, q, k]"""
        qn = (self.Q * self.Q).sum(-1, keepdim=True)
        kn = (self.K * self.K).sum(-1).unsqueeze(-2)
        return qn + kn - 2.0 * (self.Q @ self.K.transpose(-1, -2))

    def P(self):
        d = self.dist2()
        top = d == d.amax(-1, keepdim=True)
        return top.double() / top.sum(-1, keepdim=True)

    def forward(self):
        return self.P() @ self.V

    def backward(self, scale):
        """dQ, dK, dV and W = dS / dist, with dS = P (dP - delta) scale: dQ = rowsum(W) q - W K, dK = colsum(W) k - W^T Q"""
        P = self.P()
        O = P @ self.V
        dV = P.transpose(-1, -2) @ self.dO
        dP = self.dO @ self.V.transpose(-1, -2)
        D = (self.dO * O).sum(-1, keepdim=True)
        dist = self.dist2().sqrt()
        W = torch.where(dist > 0, P * (dP - D) * scale / dist.clamp_min(1e-300), torch.zeros_like(dist))
        dQ = W.sum(-1, keepdim=True) * self.Q - W @ self.K
        dK = W.sum(-2).unsqueeze(-1) * self.K - W.transpose(-1, -2) @ self.Q
        return dQ, dK, dV, W

    def zero_slack(self, scale):
        """what an exactly-zero element of dQ and of dK may hold instead, [B, H, S, HE] each.  The kernel keeps rowsum(W) and
        colsum(W) in fp32, and on a tie its p = exp(m - lse) carries the rounding of lse = m + log t: at m = 4 c scale = 2048
        one fp32 ulp is 2^-12, relative to p.  That factor multiplies one operand element (q_d or k_d: c on the row's code, 0
        off it), so the element is off by at most 2^-12 sum |W| |q_d|; with W = 0 (every 'perm' row) or off the code the
        bound is 0."""
        W = self.backward(scale)[3].abs()
        ulp = 2.0 ** (math.floor(math.log2(4 * self.code * scale)) - 23)
        return ulp * W.sum(-1, keepdim=True) * self.Q.abs(), ulp * W.sum(-2).unsqueeze(-1) * self.K.abs()

    def lse_exact(self, scale, queries=slice(None)):
        """fp32(4 c) * fp32(scale), the kernel's fp32 product (as fp64), and log t of each query's tie"""
        m = torch.tensor(4 * self.code, dtype=torch.float32) * torch.tensor(scale, dtype=torch.float32)
        d = self.dist2()[:, :, queries]
        top = d.amax(-1)
        assert bool((top == 16 * self.code ** 2).all()), "every query's maximum is (4 c)^2"
        return m.double(), torch.log((d == top.unsqueeze(-1)).sum(-1).double())

    def check_preconditions(self, scales, bwd_scale=None):
        """every query's largest squared distance is 16 c^2, reached at exactly the designed keys; every other distance is
        far enough below 4 c that its exp underflows to 0 in fp32 at each scale; every squared distance is exact in fp32; and
        (bwd_scale given) O, W, dQ and dK are exact in bf16"""
        c = self.code
        d = self.dist2()
        assert float(d.max()) < EXACT_LIMIT * c * c and torch.equal(d, d.float().double()), "qn + kn - 2 qk not exact in fp32"
        top = d.amax(-1, keepdim=True)
        assert bool((top == 16 * c * c).all()), "a query's largest distance is not 4 c"
        rest = torch.where(d == top, torch.full_like(d, -1.0), d).amax(-1)
        has = rest >= 0
        assert float(rest.max()) <= 14 * c * c
        for scale in scales:
            if bool(has.any()):
                gap = float(((4 * c - rest[has].sqrt()) * scale).min())
                assert gap >= MIN_GAP, f"score gap {gap} < {MIN_GAP} at scale {scale}"
        wrong = (d == top) != self.designed
        if bool(wrong.any()):
            b, h, q, k = (int(v) for v in wrong.nonzero()[0])
            raise AssertionError(f"query {q} of head ({b}, {h}): key {k} is {'not ' if self.designed[b, h, q, k] else ''}"
                                 f"a maximum, against the design")
        O = self.forward()
        assert torch.equal(O, O.to(BF).double()), "O not exact in bf16"
        if bwd_scale is not None:
            dQ, dK, dV, W = self.backward(bwd_scale)
            for t, name in ((W, "W"), (dQ, "dQ"), (dK, "dK"), (dV, "dV")):
                assert torch.equal(t, t.to(BF).double()), f"{name} not exact in bf16"
            assert float(dQ.abs().max()) == 0.0, "dQ is zero by construction"


# ---------------------------------------------------------------------------------- which GEMM kernel a shape reaches
# A mirror of the dispatch in csrc/gemm.hip (vg_gemm_launch), gemm_wr.hip (vg_gemm_wr_try) and gemm_tn.hip (vg_gemm_tn384_try),
# for naming the kernel in a failure message and for checking (tests/test_exact_probes_cpu.py) that the shape tables below
# reach every one of them.
def fwd_target(M, N, K, act=0, pre=None, res=False):
    """vg_linear_fwd (pre: None / 'f32' / 'bf16' pre-activation output) and vg_linear_gelu_fwd (act 1, pre 'bf16': its byte
    codes take the second-output slot)"""
    c2 = pre == "bf16"
    wr_epilogue = (act == 0 and not c2) or (act == 1 and c2 and not res) or (act == 3 and not c2 and not res)
    if K == 384 and N % 128 == 0 and M >= 256 and M % 32 == 0 and pre != "f32" and N // 128 <= 64 and wr_epilogue:
        return "wr"
    light = act in (0, 1)
    return "tiled256" if light and -(-M // 256) * -(-N // 128) >= 96 else "tiled128"


def dgrad_target(M, N, K):
    """vg_linear_dgrad: dX[M,K] = dY[M,N] W[N,K] (NN, contraction N)"""
    if N == 384 and K % 128 == 0 and M >= 256 and M % 32 == 0 and K // 128 <= 64:
        return "wr"
    return "tiled256" if -(-M // 256) * -(-K // 128) >= 96 else "tiled128"


def wgrad_target(M, N, K):
    """vg_linear_wgrad: dW[N,K] = dY[M,N]^T X[M,K] (TN, contraction M)"""
    if N % 128 == 0 and M % 32 == 0 and M >= 64 and (K % 384 == 0 or K % 512 == 0):
        return "tn384" if K % 384 == 0 else "tn512"
    return "tiled_tn"


def wr_runs(M, N):
    """(nfull, rem) of every run of the weights-in-registers kernel: units of 32 rows dealt to 8 * (64 / (N / 128)) runs"""
    units, nruns = M // 32, 8 * (64 // (N // 128))
    out = set()
    for r in range(nruns):
        n = (r + 1) * units // nruns - r * units // nruns
        if n:
            out.add((n >> 2, n & 3))
    return out


M_RESIDUES = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 288, 383, 384, 385, 511, 512, 513, 1040]
# (M list, N, K) for vg_linear_fwd in the counting regime
FWD_SHAPES = (
    [(M_RESIDUES, N, K) for K in (48, 96, 384, 768, 1536) for N in (136, 256)]  # tiled128 (N % 128 != 0) and, at K = 384, wr
    + [(M_RESIDUES, 136, 40), (M_RESIDUES, 256, 56)]                             # tiled128 with K tails of 8 and 24 (BK = 32)
    + [([4100], 768, 96), ([3073], 1032, 48), ([8192], 384, 768)]                # tiled256: >= 96 tiles of 256 x 128
    + [([256, 512, 768, 1024, 1280, 2560, 2816, 3328, 1120], 8192, 384)]         # wr with 8 runs: nfull 0 / 1 / many, rem 0..3
    + [([16640], 1152, 384), ([16640], 384, 384), ([16640], 1536, 384)]          # wr at the step's shapes (QKV, out-proj, fc1)
)
# (M list, N, K) for vg_linear_dgrad (dX[M,K] = dY[M,N] W[N,K]); wr needs N = 384 (the contraction) and K % 128 == 0
DGRAD_SHAPES = (
    [(M_RESIDUES, 136, 200), (M_RESIDUES, 384, 256), (M_RESIDUES, 1536, 384)]
    + [([4100], 96, 768), ([256, 1024, 2816], 384, 8192), ([16640], 384, 384), ([16640], 1536, 384)]
)


# ------------------------------------------------------------------------ the full-row kernel (csrc/gemm_row.hip)
# A mirror of its dispatch: vg_row_nwg deals units = M / 16 over min(256, ceil(units / 2)) workgroups, workgroup w owns the units
# [w units / nwg, (w + 1) units / nwg), and the `while (n > 0)` loop at the end of the kernel cuts them into tiles of at most
# MAXMT m-tiles.  tests/test_exact_probes_cpu.py holds the workgroup count against vg_row_parts and proves that ROW_M
# reaches every tile height the kernel is instantiated for.
ROW_MAXMT = {384: 9, 512: 6}
ROW_MINUNITS = 2


def row_tiles(M, E):
    """per workgroup of the row kernel at [M, E]: (first row, [heights of its tiles, in m-tiles of 16 rows])"""
    assert M >= 16 and M % 16 == 0, M
    maxmt = ROW_MAXMT[E]
    units = M // 16
    nwg = min(256, -(-units // ROW_MINUNITS))
    out = []
    for w in range(nwg):
        u0, u1 = w * units // nwg, (w + 1) * units // nwg
        n, tiles = u1 - u0, []
        while n > 0:
            mt = n if n <= maxmt else (8 if maxmt == 9 else (maxmt if n >= 2 * maxmt else (n + 1) // 2))
            tiles.append(mt)
            n -= mt
        out.append((16 * u0, tiles))
    return out


def row_owner(M, E, device="cpu"):
    """(rows per workgroup [nwg], workgroup of every row [M]) as int64 tensors"""
    tiles = row_tiles(M, E)
    rows = torch.tensor([16 * sum(t) for _, t in tiles], device=device)
    assert int(rows.sum()) == M and [f for f, _ in tiles] == (rows.cumsum(0) - rows).tolist()
    return rows, torch.repeat_interleave(torch.arange(len(tiles), device=device), rows)


# row counts that reach every height: 1 (16 rows), 1 + 2 (48 rows), h = 1..MAXMT alone (4096 h rows: 256 workgroups of h units), and
# workgroups of several tiles (384: 8 + 2 | 9, 8 + 2 | 8 + 3, 8 + 8 | 8 + 9;  512: 4 + 3 | 6, 5 + 5 | 6 + 5, 6 + 5 + 5 | 6 + 6 + 5)
ROW_M = {384: [16, 48] + [4096 * k for k in range(1, 10)] + [38912, 43008, 66560],
         512: [16, 48] + [4096 * k for k in range(1, 7)] + [26624, 43008, 66560]}
ROW_K = (128, 192, 320)                # 4, 6 and 10 stages of the 4-slot ring: exactly the ring, a wrap, a wrap that is no multiple of 4
ROW_TALL = {384: 38912, 512: 26624}    # the tall row count that runs at every K: several tiles per workgroup and the tallest tile


def row_cases(E):
    """(M, K) of the exact row probes: K cycles over ROW_M; 16, 48 and ROW_TALL run at every K"""
    cases = [(M, ROW_K[i % 3]) for i, M in enumerate(ROW_M[E])]
    return cases + [(M, K) for M in (16, 48, ROW_TALL[E]) for K in ROW_K if (M, K) not in cases]


def grid_of(t, what="value"):
    """the largest 2^-k (k <= 16) that every element of t is a multiple of"""
    for k in range(17):
        s = t * 2.0 ** k
        if torch.equal(s, torch.round(s)):
            return 2.0 ** -k
    raise AssertionError(f"{what}: not on a dyadic grid of 2^-16 or coarser")


def assert_f32_exact(t, what):
    assert torch.equal(t, t.float().double()), f"{what}: not exact in fp32"
    return t


def assert_exact_sum(terms, dims, what, limit=EXACT_LIMIT):
    """an fp32 sum of `terms` over `dims` is exact in any order: the terms lie on a grid 2^-k and sum |terms| < 2^24 grid steps"""
    q = grid_of(terms, what)
    top = float(terms.abs().sum(dims).max()) / q
    assert top < limit, f"{what}: sum |terms| reaches {top} >= {limit} steps of {q}"


def row_bwd_terms(d, h, rstd, gamma, gres=None, lb=None, wmod=None, gs=None, bs=None):
    """The backward of Linear <- LayerNorm (wmod None) or Linear <- self-modulated LayerNorm, from d = dY W [M, E], the
    normalised rows h = (x - mean) rstd, rstd [M] and the LayerNorm's weight gamma (lw), as the kernels' epilogue forms it; plain
    torch in the dtype of its inputs.  Returns the terms whose column sums are d gamma (d lw) and d beta (d lb), the terms of d gs
    and d bs and d w (self-modulated form only), dx, and the magnitudes that dx's fp32 arithmetic rounds relative to."""
    rs = rstd[:, None]
    o = {}
    if wmod is not None:
        o["l"] = l = h * gamma + lb
        o["gl"] = gs * l + bs
        o["dw"] = d * o["gl"]
        o["dwm"] = dwm = d * wmod
        o["t_gs"], o["t_bs"] = dwm * l, dwm
        d = dwm * gs
    o["t_gamma"], o["t_beta"] = d * h, d
    o["gg"] = gg = d * gamma
    o["ggh"] = ggh = gg * h
    c1, c2 = gg.mean(1, keepdim=True), ggh.mean(1, keepdim=True)
    core = rs * (gg - c1 - h * c2)
    mag = rs * (gg.abs() + c1.abs() + (h * c2).abs())
    o["dx"] = core if gres is None else core + gres
    o["dx_mag"] = mag if gres is None else mag + gres.abs()
    return o


class RowBwdProbe:
    """Exact inputs of vg_linear_dgrad_ln_bwd / vg_linear_dgrad_sln_bwd at [M, K] -> [M, E], with their exact consequences (fp64, on
    the generator's device).  The caller of these kernels supplies mean and rstd, so the probe chooses them: integers x in [-4, 4],
    per-row mean in {-1, 0, 1} and rstd in {0.5, 1} (drawn per row: a statistic read from the wrong row shows), so that
    h = (x - mean) rstd is a multiple of 1/2.  d = bf16(dY W) is an integer (counting regime); gamma (lw), lb, wmod, gs and bs are
    dyadic with small numerators.  Every product of the epilogue is then exact in fp32 and every sum of them exact in any order
    (asserted here, on the fp64 values), which leaves the five roundings of dx as the kernel's only freedom.
    sln: the self-modulated form, d_eff = d wmod gs;  bcast > 0: x has that many rows, broadcast over the batch."""

    GS, BS = 1.5, -0.25
    DX_FLOOR = 2.0 ** -20  # the kernel forms dx with five fp32 roundings of at most 2^-24 each, relative to dx_mag: 3x headroom

    def __init__(self, M, K, E, g, sln=False, bcast=0, density=0.5, limit=EXACT_LIMIT):
        self.M, self.K, self.E, self.sln, self.bcast, self.limit = M, K, E, sln, bcast, limit
        self.dY = counting((M, K), g, -1, 1, density)
        self.W = counting((K, E), g, -1, 1, density)   # nn.Linear(E, K).weight: the Linear the LayerNorm feeds
        self.x = counting((bcast or M, E), g, -4, 4)
        self.mean = counting((M,), g, -1, 1)
        self.rstd = 0.5 * (1.0 + counting((M,), g, 0, 1))
        self.gres = counting((M, E), g, -8, 8)
        self.lb = self.wmod = None
        if sln:
            self.gamma = dyadic((E,), g, 2, 3)         # lw
            self.lb = dyadic((E,), g, 4, 4)
            self.wmod = dyadic((M, E), g, 2, 2)
        else:
            self.gamma = 1.0 + dyadic((E,), g, 16, 4)
        self.d = check_exact_gemm(self.dY, self.W, out_dtype=BF, what="d")
        xf = self.x.repeat(-(-M // bcast), 1)[:M] if bcast else self.x
        self.h = (xf - self.mean[:, None]) * self.rstd[:, None]
        sl = dict(lb=self.lb, wmod=self.wmod, gs=self.GS, bs=self.BS) if sln else {}
        self.t = t = row_bwd_terms(self.d, self.h, self.rstd, self.gamma, **sl)
        assert_f32_exact(self.h, "h")
        for name in ("l", "gl", "dw", "dwm", "t_gs", "t_gamma", "t_beta", "gg", "ggh"):
            if name in t:
                assert_f32_exact(t[name], name)
        for name, dims in (("t_gamma", 0), ("t_beta", 0), ("gg", 1), ("ggh", 1)):
            assert_exact_sum(t[name], dims, name, limit)

    def dx(self, with_gres):
        """(fp64 dx, the floor of its fp32 arithmetic)"""
        if with_gres:
            return self.t["dx"] + self.gres, self.DX_FLOOR * (self.t["dx_mag"] + self.gres.abs())
        return self.t["dx"], self.DX_FLOOR * self.t["dx_mag"]

    def check_scalar_budget(self, owner, nwg, limit=EXACT_LIMIT):
        """d gs / d bs: a workgroup's sum over its rows AND all columns stays exact (it does not grow with M)"""
        for name in ("t_gs", "t_bs"):
            q = grid_of(self.t[name], name)
            top = float(per_workgroup(self.t[name].abs(), owner, nwg).sum(1).max()) / q
            assert top < limit, f"{name}: a workgroup's sum |terms| reaches {top} >= {limit} steps of {q}"


def per_workgroup(terms, owner, nwg):
    """[nwg, E]: column sums of terms [M, E] over each workgroup's rows, in fp64"""
    return torch.zeros(nwg, terms.shape[1], dtype=torch.float64, device=terms.device).index_add_(0, owner, terms.double())


def assert_colsum(part_w, stored, owner, rows, what):
    """part_w [nwg, E], the kernel's fp32 column sums per workgroup, against the fp64 sums of the kernel's own stored bf16 rows:
    |err| <= rows_w 2^-24 sum_w |o| per column, the standard bound of an fp32 sum of rows_w terms in any order"""
    s64 = stored.double()
    want, mag = per_workgroup(s64, owner, rows.numel()), per_workgroup(s64.abs(), owner, rows.numel())
    err = (part_w.double() - want).abs()
    bad = ~(err <= rows[:, None].double() * 2.0 ** -24 * mag)
    n = int(bad.sum())
    if n:
        w, c = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {n} column sums outside the fp32 summation bound; first at workgroup {w} column {c}: got "
                             f"{float(part_w[w, c])!r} want {float(want[w, c])!r}")
