"""Spectral normalisation (include/vitgan_hip.h, vg_spectral_*): the float64 restatement, the bounds the GPU tests hold the kernels
to, and a float32 emulation of the kernels' arithmetic in their own operation order.

Bounds.  u = 2^-24.  A sum evaluated as fma chains of length c per thread followed by a tree of depth d has every term pass through at
most c + d roundings, so |sum - exact| <= (c + d) u sum|terms| (first order).  From csrc/spectral.hip as written:
  t = W^T u     chains over rows r, r + 16, ... (c = ceil(N / 16)), then the 16 slot sums in order (15 adds)     kappa_t = ceil(N/16) + 15
  w = W v       chains over 4 columns per 256 (c = 4 ceil(K / 256)), then a 6-level butterfly                   kappa_w = 4 ceil(K/256) + 6
  |x|^2         chains x[i], x[i + 256], .. (c = ceil(n / 256)), butterfly (6), four wave sums (3)              kappa_n = ceil(n/256) + 9
                positive terms: a RELATIVE error; the square root halves it and adds one rounding
  <G, W>        32-term chains, butterfly (6), wave sums (3), then the chunk sums in order (nchunk - 1)         kappa_d = 40 + nchunk
  v = t * (1 / max(|t|, eps)), u likewise: one division, one product on top of the norm                          + 2 roundings
  shadow        fp32(sigma0 / sigma) * W: one division, one product, then the bf16 rounding (half an ulp: 2^-8 relative)
  projection    coef = dot / sigma, cu = coef * u_n, fma, s = sigma0 / sigma, product                           kappa_p = 5
Errors of an input a stage receives from the stage before are not its own: every stage is compared with the restatement FED THE
KERNEL'S OWN INPUTS (v from (W, u_in); w, sigma, u from the kernel's v; the shadow from the kernel's sigma; the projection from the
state it read), and a norm's bound carries the 2-norm of its vector's bound.
"""
import math

import numpy as np
import torch

U32 = 2.0 ** -24
EPS = 1e-12
CHUNK, COLS, ROWS = 8192, 64, 16
F8 = torch.float64

SHAPES = sorted({(E * a, E * b) for E in (128, 384, 512, 768) for a, b in ((1, 1), (2, 1), (1, 2))}
                | {(1, 384), (10, 384), (1, 768), (384, 48), (512, 192), (768, 768)})


def make_matrix(N, K, scale="init", seed=0):
    """"init": trunc_normal(std 0.02), vit_init_weights' scale.  "trained": that plus a few dominant directions and a heavier bulk, the
    spectrum a trained layer has (a spectral gap, sigma_max of order 1 to 10)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * N + K)
    W = torch.nn.init.trunc_normal_(torch.empty(N, K), std=0.02, generator=g)
    if scale == "trained":
        W = 4.0 * W
        for j, amp in enumerate((6.0, 3.5, 2.0)):
            a, b = torch.randn(N, generator=g), torch.randn(K, generator=g)
            W = W + amp / (j + 1) * torch.outer(a / a.norm(), b / b.norm())
    return W.float().contiguous()


# ------------------------------------------------------------------------------------------ the float64 restatement
def power_step(W, u):
    """One iteration as the header states it: (v, sigma, u')."""
    W, u = W.to(F8), u.to(F8)
    t = W.t() @ u
    v = t / max(float(t.norm()), EPS)
    w = W @ v
    sigma = float(w.norm())
    return v, sigma, w / max(sigma, EPS)


def top_pair(W):
    U, S, Vh = torch.linalg.svd(W.to(F8), full_matrices=False)
    return U[:, 0], float(S[0]), Vh[0]


def effective(W, sigma, sigma0):
    return (sigma0 / max(sigma, EPS)) * W.to(F8)


def project(G, W, u, v, sigma, sigma0):
    """dL/dW from G = dL/dW_eff, W_eff = sigma0 W / sigma, sigma = u^T W v with u, v constants."""
    G, W, u, v = G.to(F8), W.to(F8), u.to(F8), v.to(F8)
    sg = max(sigma, EPS)
    return (sigma0 / sg) * (G - (float((G * W).sum()) / sg) * torch.outer(u, v))


# ------------------------------------------------------------------------------------------ bounds
def kappa(N, K):
    nchunk = -(-N * K // CHUNK)
    return {"t": -(-N // 16) + 15, "w": 4 * (-(-K // 256)) + 6, "nK": -(-K // 256) + 9, "nN": -(-N // 256) + 9, "dot": 40 + nchunk, "proj": 5}


def _frac(err, bound):
    return float((err / bound.clamp_min(1e-300)).max()) if torch.is_tensor(err) else err / max(bound, 1e-300)


def check_update(W, u_in, sigma0, v, sigma, u, shadow, what=""):
    """The kernel's (v, sigma, u, shadow) after one update of W [N, K] from u_in with sigma0.  Returns the worst fraction of each bound
    used; raises AssertionError outside."""
    N, K = W.shape
    k = kappa(N, K)
    W8, u8 = W.to(F8), u_in.to(F8)
    # v against (W, u_in)
    t = W8.t() @ u8
    bt = k["t"] * U32 * (W8.abs().t() @ u8.abs())
    tn = float(t.norm())
    v_ref = t / max(tn, EPS)
    bv = (bt + v_ref.abs() * float(bt.norm())) / max(tn, EPS) + (k["nK"] / 2 + 4) * U32 * v_ref.abs()
    fr = {"v": _frac((v.to(F8) - v_ref).abs(), bv + 1e-300)}
    # w, sigma, u against the kernel's own v
    v8 = v.to(F8)
    w = W8 @ v8
    bw = k["w"] * U32 * (W8.abs() @ v8.abs())
    wn = float(w.norm())
    bs = float(bw.norm()) + (k["nN"] / 2 + 1) * U32 * wn
    fr["sigma"] = abs(float(sigma) - wn) / max(bs, 1e-300)
    u_ref = w / max(wn, EPS)
    bu = (bw + u_ref.abs() * float(bw.norm())) / max(wn, EPS) + (k["nN"] / 2 + 4) * U32 * u_ref.abs()
    fr["u"] = _frac((u.to(F8) - u_ref).abs(), bu + 1e-300)
    # the shadow against the kernel's own sigma: only a bf16 rounding boundary may flip
    ref = effective(W, float(sigma), float(sigma0))
    bsh = (2.0 ** -8 + 2 * U32) * ref.abs()
    fr["shadow"] = _frac((shadow.to(F8) - ref).abs(), bsh + 1e-300)
    check_update.last = {"bs": bs, "bv2": float(bv.norm())}  # absolute bounds of sigma and |v - v_ref|_2, for callers that chain them
    for name, f in fr.items():
        assert math.isfinite(f) and f <= 1.0, f"{what}: {name} off: {f:.3f} of its bound (kappa {k})"
    return fr


def check_project(G, W, u, v, sigma, sigma0, out, what=""):
    N, K = W.shape
    k = kappa(N, K)
    G8, W8, u8, v8 = G.to(F8), W.to(F8), u.to(F8), v.to(F8)
    sg = max(float(sigma), EPS)
    s = float(sigma0) / sg
    uv = torch.outer(u8, v8)
    dot = float((G8 * W8).sum())
    bdot = k["dot"] * U32 * float((G8 * W8).abs().sum())
    ref = s * (G8 - (dot / sg) * uv)
    bound = s * (bdot / sg) * uv.abs() + k["proj"] * U32 * (s * G8.abs() + abs(s * dot / sg) * uv.abs())
    f = _frac((out.to(F8) - ref).abs(), bound + 1e-300)
    assert math.isfinite(f) and f <= 1.0, f"{what}: projected gradient off: {f:.3f} of its bound (kappa {k})"
    return f


# ------------------------------------------------------------------------------------------ float32 emulation, the kernels' order
def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _butterfly(a):
    """a [..., 64]: v += shfl_xor(v, o) for o = 32 .. 1"""
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = (a + a[..., idx ^ o]).astype(np.float32)
    return a


def _norm32(x):
    n = len(x)
    pad = np.zeros(-(-n // 256) * 256, np.float32)
    pad[:n] = x
    acc = np.zeros(256, np.float32)
    for row in pad.reshape(-1, 256):
        acc = _fma(row, row, acc)
    w = _butterfly(acc.reshape(4, 64))[:, 0]
    return np.sqrt(np.float32(np.float32(np.float32(w[0] + w[1]) + w[2]) + w[3]))


def emulate_update(W, u, sigma0, transpose_bug=False, inverse_scale_bug=False):
    """(v, sigma, u', shadow) in float32 as csrc/spectral.hip computes them.  The two switches plant mistakes."""
    W = np.ascontiguousarray(W.numpy(), dtype=np.float32)
    u = u.numpy().astype(np.float32)
    N, K = W.shape
    A = W.T.copy() if transpose_bug else W  # (square matrices only)
    part = np.zeros((16, K), np.float32)
    for r in range(N):
        part[r % 16] = _fma(A[r], np.full(K, u[r], np.float32), part[r % 16])
    t = part[0].copy()
    for r in range(1, 16):
        t = (t + part[r]).astype(np.float32)
    inv = np.float32(1.0) / max(_norm32(t), np.float32(EPS))
    v = (t * inv).astype(np.float32)
    Kp = -(-K // 256) * 256
    Wp, vp = np.zeros((N, Kp), np.float32), np.zeros(Kp, np.float32)
    Wp[:, :K], vp[:K] = A, v
    acc = np.zeros((N, 64), np.float32)
    lane4 = np.arange(64) * 4
    for base in range(0, Kp, 256):
        for j in range(4):
            cols = base + lane4 + j
            acc = _fma(Wp[:, cols], np.broadcast_to(vp[cols], (N, 64)), acc)
    w = _butterfly(acc)[:, 0]
    sigma = _norm32(w)
    un = (w * (np.float32(1.0) / max(sigma, np.float32(EPS)))).astype(np.float32)
    s = np.float32(sigma0) / max(sigma, np.float32(EPS))
    if inverse_scale_bug:
        s = max(sigma, np.float32(EPS)) / np.float32(sigma0)
    shadow = torch.from_numpy((s * W).astype(np.float32)).to(torch.bfloat16)
    return torch.from_numpy(v), float(sigma), torch.from_numpy(un), shadow


def emulate_project(G, W, u, v, sigma, sigma0, no_sigma_bug=False):
    G = np.ascontiguousarray(G.numpy(), dtype=np.float32)
    W = np.ascontiguousarray(W.numpy(), dtype=np.float32)
    u, v = u.numpy().astype(np.float32), v.numpy().astype(np.float32)
    N, K = W.shape
    NK = N * K
    nchunk = -(-NK // CHUNK)
    g, w = np.zeros(nchunk * CHUNK, np.float32), np.zeros(nchunk * CHUNK, np.float32)
    g[:NK], w[:NK] = G.reshape(-1), W.reshape(-1)
    g, w = g.reshape(nchunk, CHUNK // 1024, 256, 4), w.reshape(nchunk, CHUNK // 1024, 256, 4)  # [chunk, iteration, thread, j]
    acc = np.zeros((nchunk, 256), np.float32)
    for it in range(CHUNK // 1024):
        for j in range(4):
            acc = _fma(g[:, it, :, j], w[:, it, :, j], acc)
    ws = _butterfly(acc.reshape(nchunk, 4, 64))[:, :, 0]
    parts = ((ws[:, 0] + ws[:, 1]).astype(np.float32) + ws[:, 2]).astype(np.float32)
    parts = (parts + ws[:, 3]).astype(np.float32)
    dot = parts[0]
    for c in range(1, nchunk):
        dot = np.float32(dot + parts[c])
    sg = max(np.float32(sigma), np.float32(EPS))
    coef = dot if no_sigma_bug else np.float32(dot / sg)
    s = np.float32(np.float32(sigma0) / sg)
    cu = (coef * u).astype(np.float32)
    out = _fma(-np.broadcast_to(cu[:, None], (N, K)), np.broadcast_to(v[None, :], (N, K)), G)
    return torch.from_numpy((s * out).astype(np.float32))
