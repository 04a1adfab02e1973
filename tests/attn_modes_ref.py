"""fp64 references, per-element error budgets and checkers for the fp8 (mode 2) and L2-distance (mode 1) attention kernels of
csrc/attention.hip (a plain helper module, imported like exact_util).  Plain torch, no autograd: every intermediate is kept.

mode 'l2'   s = |q - k| scale, P = softmax(s), O = P V.  dP = dO V^T, delta = dO . O, dS = P (dP - delta) scale, W = dS / |q - k|
            (0 at zero distance: the subgradient torch.cdist and the kernel both take), dQ = rowsum(W) q - W K,
            dK = colsum(W) k - W^T Q, dV = P^T dO.
mode 'fp8'  s = e4m3(q) . e4m3(k) scale, O = P e4m3(V); the backward recomputes P from the same quantised scores and uses the
            bf16 Q, K, V in every gradient product: dQ = dS K, dK = dS^T Q, dV = P^T dO.  Q, K and V are inputs, so their e4m3
            images are part of the operator (the model of test_ops_gpu.py::test_attention_fp8); the dyadic inputs used here
            are exact in e4m3 anyway.

The budget of an output element is first order in the roundings the kernel makes on COMPUTED quantities:
  * half a bf16 ulp, relative 2^-9, on every quantity rounded to an MFMA operand: p (forward P.V of mode l2, P^T dO of both
    backwards), dS (fp8) or W (l2), and the stored bf16 O inside delta = dO . O (the backward is given the reference O rounded
    once to bf16, and the reference LSE rounded to fp32, so that is the whole error of delta);
  * half an e4m3 step on 256 p in the fp8 forward: relative 2^-4 for a normal number, 2^-10 absolute (of 256 p) below 2^-6;
  * each propagated to the output through sums of absolute values;
  * plus one bf16 ulp of the result (the output rounding, with half an ulp to spare);
  * and the whole times MARGIN = 2.  The factor 2 is for what nobody has characterised on this hardware: the order of the fp32
    accumulations and the error of __expf / __logf.  Both are of relative size 2^-21 or so against terms of 2^-9; the factor is
    generous for them, and a defect that moves one p or one W by a rounding step more than the budget allows still fails.
LSE stays fp32: |lse - ref| <= 2^-18 max(1, |ref|) (half a dozen fp32 roundings and the two fast-math calls, each <= 2^-21
relative on values of order 1 to 8; scores here are exact in fp32 for the dyadic inputs).
"""
import torch

import exact_util as X

BF, F32 = torch.bfloat16, torch.float32
MARGIN = 2.0
HALF_BF = 2.0 ** -9
LSE_TOL = 2.0 ** -18
S_LIST = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65, 79, 80]


def dyadic_inputs(B, H, S, HE, mode, seed=0):
    """Q, K, V, dO = i / 8, |i| <= 16 (fp64; exact in bf16 and in e4m3; fp32 norms and dot products of them are exact).  For
    l2 and S >= 2, a few query rows equal a key row: that distance is exactly 0 and the zero-distance branch is reached.
    For fp8, the last head is peaked: on its first n dims every query and key 0 hold 2 and every other key -2, with n chosen so
    that key 0 leads every other score by 8 n scale ~ 7, and V[0] = 0.  Its output is then made of numerators around 2^-10
    alone, the ones the factor 256 on p exists for, with no large p V term beside them to hide what becomes of them."""
    g = X.gen(seed * 104729 + S * 389 + HE + (1 if mode == "l2" else 2))
    Q, K, V, dO = (X.dyadic((B, H, S, HE), g, 8, 16) for _ in range(4))
    if mode == "fp8":
        n = round(7.0 * HE ** 0.5 / 8.0)
        Q[:, -1, :, :n] = 2.0
        K[:, -1, :, :n] = -2.0
        K[:, -1, 0, :n] = 2.0
        V[:, -1, 0] = 0.0
    if mode == "l2" and S >= 2:
        for q, k in [(0, S - 1), (S - 1, 0)] + ([(S // 2, S // 2)] if S >= 3 else []):
            Q[:, :, q] = K[:, :, k]
    return Q, K, V, dO


def reference(mode, Q, K, V, dO, scale):
    """every intermediate of forward and backward, fp64, [B, H, ...]"""
    r = {"mode": mode, "scale": scale, "Q": Q, "K": K, "V": V, "dO": dO}
    if mode == "l2":
        qn = (Q * Q).sum(-1, keepdim=True)
        kn = (K * K).sum(-1).unsqueeze(-2)
        r["dist"] = (qn + kn - 2.0 * (Q @ K.transpose(-1, -2))).clamp_min(0.0).sqrt()
        s = r["dist"] * scale
        Vf = V
    else:
        s = (X.e4m3(Q) @ X.e4m3(K).transpose(-1, -2)) * scale
        Vf = X.e4m3(V)
    m = s.amax(-1, keepdim=True)
    pn = torch.exp(s - m)  # the numerators the fp8 forward quantises
    l = pn.sum(-1, keepdim=True)
    P = pn / l
    r.update(s=s, pn=pn, l=l, P=P, lse=(m + torch.log(l)).squeeze(-1), O=P @ Vf)
    r["O_bf"] = r["O"].float().to(BF).double()   # what the backward is given
    r["lse_f32"] = r["lse"].float().double()
    Pb = torch.exp(s - r["lse_f32"].unsqueeze(-1))
    dP = dO @ V.transpose(-1, -2)
    delta = (dO * r["O_bf"]).sum(-1, keepdim=True)
    dS = Pb * (dP - delta) * scale
    r.update(Pb=Pb, dP=dP, delta=delta, dS=dS, dV=Pb.transpose(-1, -2) @ dO)
    if mode == "l2":
        W = torch.where(r["dist"] > 0, dS / r["dist"].clamp_min(1e-300), torch.zeros_like(dS))
        r["W"] = W
        r["dQ"] = W.sum(-1, keepdim=True) * Q - W @ K
        r["dK"] = W.sum(-2).unsqueeze(-1) * K - W.transpose(-1, -2) @ Q
    else:
        r["dQ"] = dS @ K
        r["dK"] = dS.transpose(-1, -2) @ Q
    return r


def budget(r):
    """per-element bounds for O, dQ, dK, dV (see the module docstring)"""
    mode, scale = r["mode"], r["scale"]
    Q, K, V, dO = (r[n].abs() for n in ("Q", "K", "V", "dO"))
    if mode == "l2":
        ep = HALF_BF * r["P"]
        Vf = V
    else:
        ep = torch.maximum(2.0 ** -4 * r["pn"], torch.full_like(r["pn"], 2.0 ** -10 / 256.0)) / r["l"]
        Vf = X.e4m3(r["V"]).abs()
    out = {"O": MARGIN * (ep @ Vf + X.bf16_ulp(r["O"]))}
    e_delta = (dO * HALF_BF * r["O_bf"].abs()).sum(-1, keepdim=True)  # [.., q, 1]
    e_ds = r["Pb"] * e_delta * scale                                    # through delta, before the operand rounding
    out["dV"] = MARGIN * ((HALF_BF * r["Pb"]).transpose(-1, -2) @ dO + X.bf16_ulp(r["dV"]))
    if mode == "l2":
        inv = torch.where(r["dist"] > 0, 1.0 / r["dist"].clamp_min(1e-300), torch.zeros_like(e_ds))
        e_w = e_ds * inv                          # the fp32 W, as it enters rowsum / colsum
        e_wb = e_w + HALF_BF * r["W"].abs()       # the bf16 W of the W.K and W^T.Q products
        out["dQ"] = MARGIN * (e_w.sum(-1, keepdim=True) * Q + e_wb @ K + X.bf16_ulp(r["dQ"]))
        out["dK"] = MARGIN * (e_w.sum(-2).unsqueeze(-1) * K + e_wb.transpose(-1, -2) @ Q + X.bf16_ulp(r["dK"]))
    else:
        e_dsb = e_ds + HALF_BF * r["dS"].abs()
        out["dQ"] = MARGIN * (e_dsb @ K + X.bf16_ulp(r["dQ"]))
        out["dK"] = MARGIN * (e_dsb.transpose(-1, -2) @ Q + X.bf16_ulp(r["dK"]))
    return out


def flat(t):
    """[B, H, S, HE] -> [B*S, H*HE] (the kernels' row layout)"""
    B, H, S, HE = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * S, H * HE)


def assert_within(got, ref, bound, what):
    """|got - ref| <= bound for every element (all in the kernels' row layout or all [B, H, S, HE]); returns the largest
    fraction of its bound any element uses (elements with a zero bound must match exactly and count as 0)"""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs()
    bad = ~(err <= bound)
    n = int(bad.sum())
    if n:
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what}: {n} of {bad.numel()} elements outside their budget; first at {idx}: got {float(got[idx])!r} "
                             f"want {float(ref[idx])!r} budget {float(bound[idx]):.3e}")
    frac = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    return float(frac.max())


def check_budget_fwd(r, bud, O, lse):
    """O [B*S, E] bf16 and lse [B, H, S] fp32 against the reference; returns the largest budget fraction of O"""
    got = lse.detach().double().cpu()
    tol = LSE_TOL * r["lse"].abs().clamp_min(1.0)
    assert bool(((got - r["lse"]).abs() <= tol).all()), f"LSE off by {float((got - r['lse']).abs().max()):.3e}"
    return assert_within(O, flat(r["O"]), flat(bud["O"]), "O")


def check_budget_bwd(r, bud, dQKV):
    """dQKV [B*S, 3E] bf16; returns the largest budget fraction over dQ, dK, dV"""
    E = dQKV.shape[1] // 3
    return max(assert_within(dQKV[:, i * E:(i + 1) * E], flat(r[n]), flat(bud[n]), n) for i, n in enumerate(("dQ", "dK", "dV")))


# ------------------------------------------------------------------------------ checkers of the exact (saturated) probes
def check_exact_fwd(p, scale, O, L):
    """guarded O [B*S (+guard), E] and LSE [B*H*S (+guard), 1] of a forward on probe p (AttnProbe or L2Probe)"""
    B, H, S = p.B, p.H, p.S
    for buf, rows, name in ((O, B * S, "O"), (L, B * H * S, "LSE")):
        X.assert_written(buf, rows, name)
        X.assert_guard(buf, rows, name)
    X.assert_bitwise(O[:B * S], X.rne(p.flat(p.forward()), O.dtype), "O")
    m, logt = p.lse_exact(scale)
    X.assert_lse(L[:B * H * S, 0].reshape(B, H, S), m, logt, "LSE")


def check_exact_bwd(p, scale, dQKV):
    """guarded dQKV [B*S (+guard), 3E] of a backward on probe p at `scale`: bit for bit, except that an exactly-zero dQ / dK
    element of an L2Probe may hold up to its zero_slack (0 wherever W is 0)"""
    B, S, E = p.B, p.S, p.H * p.HE
    X.assert_written(dQKV, B * S, "dQKV")
    X.assert_guard(dQKV, B * S, "dQKV")
    dQ, dK, dV = p.backward(scale)[:3]
    if isinstance(p, X.L2Probe):
        sq, sk = p.zero_slack(scale)
        slack = [p.flat(sq), p.flat(sk), 0.0]
    else:
        slack = [0.0, 0.0, 0.0]
    for i, (name, t) in enumerate((("dQ", dQ), ("dK", dK), ("dV", dV))):
        X.assert_bitwise_or_slack(dQKV[:B * S, i * E:(i + 1) * E], p.flat(t), slack[i], name)
