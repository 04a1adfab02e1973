"""The probes, budgets and checkers of test_attn_modes_gpu.py, checked without a GPU.

  * X.L2Probe and the e4m3 round trip of X.AttnProbe meet their preconditions at every S in 1..80, for each head dim and kind;
  * a plain-torch emulation of the kernels' arithmetic (fp32 scores and softmax, bf16 / e4m3 roundings where the kernel comments
    name them, fp32 rowsum(W) / colsum(W)) passes the exact checkers and stays inside the element-wise budget at every shape of
    the GPU tests: the tolerances admit a correct kernel;
  * the same emulation with a defect planted is rejected by them.
"""
import math

import pytest
import torch

import attn_modes_ref as R
import exact_util as X
import test_attn_modes_gpu as G

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
B, H = G.B, G.H
DEFECTS = ["mask_last", "drop_pair", "pad_norm", "kn_shift", "zero_branch", "zero_div", "unscaled_p"]
MODE_DEFECTS = {"l2": ["mask_last", "drop_pair", "pad_norm", "kn_shift", "zero_branch", "zero_div"], "fp8": ["mask_last", "drop_pair", "unscaled_p"]}


def _mm(a, b):
    """an fp32 matrix product with an ideal accumulator: fp64 sum, rounded once (exact wherever the sum is exact in fp32)"""
    return (a.double() @ b.double()).float()


def _sum(x, dim):
    return x.double().sum(dim).float()


def _bf(x):
    return x.to(BF).float()


class Emulation:
    """vg_attn_fwd_kernel / vg_attn_bwd_kernel (and, for fp8, the arithmetic-identical vg_attn_bwd2_kernel) in plain torch.
    Inputs fp64 [B, H, S, HE] holding bf16 values.  defect: None or one of DEFECTS; `pair` = the (q, k) of 'drop_pair'."""

    def __init__(self, mode, Q, K, V, dO, scale, defect=None, pair=(0, 0)):
        self.mode, self.defect, self.pair = mode, defect, pair
        self.q, self.k, self.v, self.do = (t.float() for t in (Q, K, V, dO))
        self.scale = torch.tensor(scale, dtype=F32)
        self.S = Q.shape[2]

    def _raw(self):
        """fp32 scores before the scale: e4m3 dot products, or the distance from q.k and the fp32 squared norms"""
        q, k = self.q, self.k
        if self.mode == "fp8":
            return _mm(X.e4m3(q), X.e4m3(k).transpose(-1, -2))
        qn = _sum(q * q, -1).unsqueeze(-1)
        kn = _sum(k * k, -1)
        if self.defect == "pad_norm":  # the norm of a padded row (nonzero) leaks into the last key's score
            kn = kn.clone()
            kn[..., -1] = 4 * kn[..., -1] + 1
        if self.defect == "kn_shift":  # kn indexed one row off: key j reads |k_{j+1}|^2, the last one a padded row's 0
            kn = torch.cat([kn[..., 1:], torch.zeros_like(kn[..., :1])], -1)
        qk = _mm(q, k.transpose(-1, -2))
        return torch.sqrt(torch.clamp_min(qn + kn.unsqueeze(-2) - 2.0 * qk, 0.0))

    def _dead(self, like):
        """[.., q, k] pairs the defect leaves out of the softmax"""
        dead = torch.zeros_like(like, dtype=torch.bool)
        if self.defect == "mask_last":
            dead[..., -1] = True
        if self.defect == "drop_pair":
            dead[..., self.pair[0], self.pair[1]] = True
        return dead

    def forward(self):
        """O [B*S, E] bf16, lse [B, H, S] fp32"""
        raw = self._raw()
        sv = torch.where(self._dead(raw), torch.full_like(raw, -math.inf), raw * self.scale)
        m = sv.amax(-1, keepdim=True)
        p = torch.exp(sv - m)
        l = _sum(p, -1).unsqueeze(-1)
        inv_l = 1.0 / l
        lse = (m + torch.log(l)).squeeze(-1)
        if self.mode == "fp8":
            if self.defect == "unscaled_p":
                acc, mul = _mm(X.e4m3(p), X.e4m3(self.v)), inv_l
            else:
                acc, mul = _mm(X.e4m3(p * 256.0), X.e4m3(self.v)), inv_l * torch.tensor(1.0 / 256.0, dtype=F32)
        else:
            acc, mul = _mm(_bf(p), self.v), inv_l
        return R.flat(acc * mul).to(BF), lse

    def backward(self, O, lse):
        """dQKV [B*S, 3E] bf16 from O [B*S, E] bf16 and lse [B, H, S] fp32"""
        q, k, v, do = self.q, self.k, self.v, self.do
        Bn, Hn, S, HE = q.shape
        o = O.float().reshape(Bn, S, Hn, HE).permute(0, 2, 1, 3)
        delta = _sum(do * o, -1).unsqueeze(-1)
        raw = self._raw()
        p = torch.exp(raw * self.scale - lse.unsqueeze(-1))
        p = torch.where(self._dead(raw), torch.zeros_like(p), p)
        dp = _mm(do, v.transpose(-1, -2))
        ds = p * (dp - delta) * self.scale
        if self.mode == "l2":
            if self.defect == "zero_div":  # no zero-distance branch at all: 0 / 0
                w = ds / raw
            else:                          # 'zero_branch': the branch hands back ds instead of 0
                w = torch.where(raw > 0, ds / raw, ds if self.defect == "zero_branch" else torch.zeros_like(ds))
            wb = _bf(w)
            dq = _sum(w, -1).unsqueeze(-1) * q - _mm(wb, k)
            dk = _sum(w, -2).unsqueeze(-1) * k - _mm(wb.transpose(-1, -2), q)
        else:
            dq = _mm(_bf(ds), k)
            dk = _mm(_bf(ds).transpose(-1, -2), q)
        dv = _mm(_bf(p).transpose(-1, -2), do)
        return torch.cat([R.flat(t) for t in (dq, dk, dv)], 1).to(BF)


def _guard(t):
    """the tensor as a guarded buffer, sentinel rows behind it (the checkers take what the GPU tests hand them)"""
    t = t.reshape(t.shape[0], -1)
    buf = X.guarded(t.shape[0], t.shape[1], t.dtype, "cpu")
    buf[:t.shape[0]] = t
    return buf


def _run_exact(mode, p, scale, backward=True, defect=None, pair=(0, 0)):
    """what test_attn_modes_gpu.py::_exact_bwd / _exact_fwd do, on the emulation"""
    e = Emulation(mode, p.Q, p.K, p.V, p.dO, scale, defect, pair)
    O, lse = e.forward()
    R.check_exact_fwd(p, scale, _guard(O), _guard(lse.reshape(-1, 1)))
    if backward:
        R.check_exact_bwd(p, scale, _guard(e.backward(O, lse)))


# ------------------------------------------------------------------------------------------------------ exact probes
@pytest.mark.parametrize("kind", list(G.POW2))
@pytest.mark.parametrize("HE", [32, 64, 96])
def test_fp8_probe_and_emulation_every_S(HE, kind):
    """AttnProbe survives e4m3 at every S of the GPU test, and the emulated fp8 kernels reproduce its expectations bit for bit"""
    def one(S):
        p = G.fp8_probe(S, HE, kind)
        p.check_preconditions([G.POW2[kind], 1 / math.sqrt(HE)])
        p.check_fp8_preconditions()
        _run_exact("fp8", p, G.POW2[kind])
        _run_exact("fp8", p, 1 / math.sqrt(HE), backward=False)
    X.collect(list(range(1, 81)), one, "S=")


@pytest.mark.parametrize("kind", ["perm", "tie2a", "tie2b", "tie2c", "tie4"])
@pytest.mark.parametrize("HE", [32, 64, 96])
def test_l2_probe_and_emulation_every_S(HE, kind):
    """L2Probe's preconditions (designed maxima only, gap >= 110 at both scales, exact W / dQ / dK) at every S, its P against
    an fp64 softmax of the distances, and the emulated L2 kernels against its checkers"""
    v1 = 1 / math.sqrt(H * HE)

    def one(S):
        p = G.l2_probe(S, HE, kind)
        p.check_preconditions([G.L2_SCALE], bwd_scale=G.L2_SCALE)
        P = torch.softmax(p.dist2().sqrt() * G.L2_SCALE, -1)
        assert float((P - p.P()).abs().max()) < 1e-40, "softmax is not saturated"
        r = R.reference("l2", p.Q, p.K, p.V, p.dO, G.L2_SCALE)  # the written-out operator agrees with the probe's consequences
        dQ, dK, dV, W = p.backward(G.L2_SCALE)
        assert float((r["O"] - p.forward()).abs().max()) < 1e-9
        for a, b_ in ((r["dV"], dV), (r["dK"], dK), (r["dQ"], dQ)):  # the reference's P carries the fp32 rounding of LSE (2^-12 at 2048)
            assert float((a - b_).abs().max()) <= 2.0 ** -12 * max(1.0, float(p.backward(G.L2_SCALE)[3].abs().sum(-2).max()) * X.CODE)
        _run_exact("l2", p, G.L2_SCALE)
        w = G.l2_probe(S, HE, kind, code=G.L2_V1_CODE)
        w.check_preconditions([v1])
        _run_exact("l2", w, v1, backward=False)
        if p.kind != "perm":
            assert float(dK.abs().max()) > 0, "a tie without a nonzero dK"
    X.collect(list(range(1, 81)), one, "S=")


def test_l2_probe_gaps():
    """(4 - sqrt(14)) c scale at both scales in use, against MIN_GAP; c = 64 would not do at v1's scale"""
    assert (4 - math.sqrt(14)) * X.CODE * G.L2_SCALE >= X.MIN_GAP
    for HE in (32, 64, 96):
        assert (4 - math.sqrt(14)) * G.L2_V1_CODE / math.sqrt(H * HE) >= X.MIN_GAP
        assert (4 - math.sqrt(14)) * X.CODE / math.sqrt(H * HE) < X.MIN_GAP
    assert (4 * G.L2_V1_CODE) ** 2 < 2.0 ** 31  # 16 c^2 = 2^30 and every qn + kn - 2 qk below it: exact in fp32


def test_fp8_precondition_rejects_a_value_outside_e4m3():
    p = G.fp8_probe(20, 32, "perm")
    p.check_fp8_preconditions()
    p.V[0, 0, 3, 5] = 2.0625  # 1.00001b x 2: five mantissa bits
    with pytest.raises(AssertionError, match="e4m3"):
        p.check_fp8_preconditions()


@pytest.mark.parametrize("HE", [32, 64, 96])
@pytest.mark.parametrize("S", [1, 15, 16, 17, 32, 33, 80])
def test_exact_checkers_reject_defects(S, HE):
    """each planted defect changes a saturated probe's result and is caught.  The defects that need a zero distance or a small
    p are invisible to these probes by construction and are asserted to be: no distance in an L2Probe is 0 (zero_branch,
    zero_div), and p in {1, 1/2, 1/4} is exact in e4m3 with or without the factor 256 (unscaled_p).  The budget test below
    is the one that sees them (see _inert for zero_branch)."""
    p8, pl = G.fp8_probe(S, HE, "perm", 1), G.l2_probe(S, HE, "perm", 1)
    last = int(p8.P()[0, 0, :, S - 1].argmax()), int(pl.P()[0, 0, :, S - 1].argmax())  # the query whose target is key S - 1
    for mode, p, scale, ql in (("fp8", p8, 1 / 8, last[0]), ("l2", pl, G.L2_SCALE, last[1])):
        _run_exact(mode, p, scale)
        for defect in MODE_DEFECTS[mode]:
            if defect in ("zero_branch", "zero_div", "unscaled_p"):
                _run_exact(mode, p, scale, defect=defect)
                continue
            with pytest.raises(AssertionError):
                _run_exact(mode, p, scale, defect=defect, pair=(ql, S - 1))
    if S >= 4:  # a tie with one of its keys dropped for one query
        for mode, p, scale in (("fp8", G.fp8_probe(S, HE, "tie4", 1), 1 / 8), ("l2", G.l2_probe(S, HE, "tie4", 1), G.L2_SCALE)):
            _run_exact(mode, p, scale)
            with pytest.raises(AssertionError):
                _run_exact(mode, p, scale, defect="drop_pair", pair=(0, S - 1))


# -------------------------------------------------------------------------------------------------- the moderate regime
def _budget_case(mode, S, HE):
    Q, K, V, dO = R.dyadic_inputs(B, H, S, HE, mode)
    r = R.reference(mode, Q, K, V, dO, G.mode_scale(mode, HE))
    return (Q, K, V, dO), r, R.budget(r)


def _run_budget(mode, inputs, r, bud, defect=None, pair=(0, 0)):
    """what test_attention_modes_within_budget does with the kernels, on the emulation; returns the two budget fractions"""
    e = Emulation(mode, *inputs, r["scale"], defect, pair)
    O, lse = e.forward()
    f = R.check_budget_fwd(r, bud, O, lse)
    dQKV = e.backward(R.flat(r["O_bf"]).to(BF), r["lse_f32"].float())
    return f, R.check_budget_bwd(r, bud, dQKV)


def test_reference_matches_autograd():
    """the written-out operators and gradients against fp64 autograd of the same formulas (cdist for l2), away from zero
    distances, where autograd's subgradient is also 0"""
    for mode in ("l2", "fp8"):
        Q, K, V, dO = R.dyadic_inputs(B, H, 33, 64, mode, seed=3)
        scale = G.mode_scale(mode, 64)
        r = R.reference(mode, Q, K, V, dO, scale)
        q, k, v = (t.clone().requires_grad_(True) for t in (Q, K, V))
        s = (torch.cdist(q, k, p=2) if mode == "l2" else q @ k.transpose(-1, -2)) * scale
        O = torch.softmax(s, -1) @ v
        O.backward(dO)
        assert float((O.detach() - r["O"]).abs().max()) < 1e-12
        # the reference backward takes the rounded O and LSE: compare within what those roundings can move it
        for got, want in ((r["dQ"], q.grad), (r["dK"], k.grad), (r["dV"], v.grad)):
            assert float((got - want).abs().max()) < 2.0 ** -7 * float(want.abs().max())


@pytest.mark.parametrize("HE", [32, 64, 96])
@pytest.mark.parametrize("mode", ["fp8", "l2"])
def test_emulation_within_budget_and_defects_outside(mode, HE):
    """at every shape of the GPU test: the emulated kernel is inside every element's budget, and every planted defect that
    changes the operator at that shape is outside someone's"""
    worst = [0.0, 0.0]

    def one(S):
        inputs, r, bud = _budget_case(mode, S, HE)
        f, b_ = _run_budget(mode, inputs, r, bud)
        worst[0], worst[1] = max(worst[0], f), max(worst[1], b_)
        for defect in MODE_DEFECTS[mode]:
            if _inert(defect, mode, S, r):
                continue
            try:
                _run_budget(mode, inputs, r, bud, defect, pair=(S // 3, (2 * S) // 3))
            except AssertionError:
                continue
            raise AssertionError(f"defect {defect} passes the budget")
    X.collect(R.S_LIST, one, "S=")
    print(f"{mode} HE={HE}: emulation uses at most {worst[0]:.3f} (forward) and {worst[1]:.3f} (backward) of the budget")
    assert max(worst) <= 1.0


def _inert(defect, mode, S, r):
    """where a defect does not change the operator, so that no checker can or should object.
    zero_branch, everywhere: at zero distance q = k, so whatever W the branch returns multiplies q - k = 0 in both
    rowsum(W) q - W K and colsum(W) k - W^T Q; all that is left of it is the bf16 rounding of that W, 2^-9 |dS| |k_d|, a term
    of the size the budget grants every other key.  What the branch is there for is the 0 / 0 without it: zero_div.
    zero_div at S = 1, where no row is planted on a key (the one distance is not 0).
    unscaled_p where no numerator lies below e4m3's normal range, 2^-6 (above it e4m3(p) = e4m3(256 p) / 256 exactly)."""
    if defect == "zero_branch":
        return True
    if defect == "zero_div":
        return S == 1
    if defect == "unscaled_p":
        return not bool((r["pn"] < 2.0 ** -6).any())
    return False
