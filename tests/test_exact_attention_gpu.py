"""The attention kernels on saturated-softmax probes (tests/exact_util.py AttnProbe), bit for bit, at every S.

Every key carries a distinct code c (e_a + e_b) (c = 64); a query carrying key k's code scores 2 c^2 against it and at most
c^2 against any other key, a gap of c^2 * scale >= 110 at every scale used, so every other exp underflows to exactly 0 in
fp32 and the target's is exp(0) = 1.  Then O[q] = V[pi(q)], dV[k] = dO[pi^-1(k)], dQ = dK = 0 and LSE = fp32(2 c^2 scale),
all exact; 2- and 4-way ties (duplicated key codes, queries carrying the sum of two codes) exercise P.V over several keys,
the online-softmax rescale and a nonzero dS / dQ / dK, exact with a power-of-two scale.  S runs over 1..256 inside one test
per (head dim, probe), so both short kernels (S <= 32, S <= 80), the long kernel and every padding case of its 32-key pairs
and 16-row tiles are reached, and every failing S is reported in one message.
"""
import math

import pytest
import torch

import exact_util as X

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
CUDA = "cuda"
B, H = 2, 2


def _probe(S, HE, kind, seed=0):
    """the probe of `kind` at S; tie positions: 'tie2a' first + last key, 'tie2b' the first two keys of the last 32-key
    pair - or, where that pair holds a single key (S % 32 == 1), the last two keys, which straddle the last two pairs -,
    'tie2c' two keys 16 apart (different 16-row tiles), 'tie4' first, two inner and last"""
    if kind == "tie2a" and S >= 2:
        return X.AttnProbe(B, H, S, HE, "tie2", (0, S - 1), seed)
    if kind == "tie2b" and S >= 2:
        a = 32 * ((S - 1) // 32)
        return X.AttnProbe(B, H, S, HE, "tie2", (a, a + 1) if a + 1 < S else (a - 1, a), seed)
    if kind == "tie2c" and S >= 17:
        return X.AttnProbe(B, H, S, HE, "tie2", (S - 17, S - 1), seed)
    if kind == "tie4" and S >= 4:
        return X.AttnProbe(B, H, S, HE, "tie4", (0, S // 3, (2 * S) // 3, S - 1), seed)
    if kind == "sum":
        return X.AttnProbe(B, H, S, HE, "sum", None, seed)
    return X.AttnProbe(B, H, S, HE, "perm", None, seed)


def _check_lse(got, p, scale, what, queries=slice(None)):
    """t = 1: exactly fp32(2 c^2 * scale); a t-way tie: that + log t within one fp32 ulp"""
    m, logt = p.lse_exact(scale, queries)
    got = got.detach().double().cpu()
    want = m + logt
    ulp = torch.pow(2.0, torch.floor(torch.log2(want.abs())) - 23)
    exact = logt == 0
    bad = torch.where(exact, got != m, (got - want).abs() > ulp)
    n = int(bad.sum())
    if n:
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {n} LSE values wrong; first at {i}: got {float(got[i])!r} want {float(want[i])!r}")


def _fwd(p, scale, f32=False):
    u = X.gpu()
    S, HE, E = p.S, p.HE, p.H * p.HE
    dt = F32 if f32 else BF
    qkv = p.qkv.to(CUDA).to(dt)
    O = X.guarded(B * S, E, dt, CUDA)
    L = X.guarded(B * H * S, 1, F32, CUDA)
    u.call("vg_attention_f32_fwd" if f32 else "vg_attention_fwd", u.ptr(qkv), u.ptr(O), u.ptr(L), B, H, S, HE, scale, u.stream())
    u.sync()
    X.assert_written(O, B * S, "O")
    X.assert_guard(O, B * S, "O")
    X.assert_written(L, B * H * S, "LSE")
    X.assert_guard(L, B * H * S, "LSE")
    X.assert_bitwise(O[:B * S], X.rne(p.flat(p.forward()), dt), "O")
    _check_lse(L[:B * H * S, 0].reshape(B, H, S), p, scale, "LSE")
    return qkv, O, L


def _bwd(p, scale, f32=False):
    u = X.gpu()
    S, HE, E = p.S, p.HE, p.H * p.HE
    dt = F32 if f32 else BF
    qkv, O, L = _fwd(p, scale, f32)
    dO = p.flat(p.dO).to(CUDA).to(dt)
    dQKV = X.guarded(B * S, 3 * E, dt, CUDA)
    u.call("vg_attention_f32_bwd" if f32 else "vg_attention_bwd", u.ptr(qkv), u.ptr(O), u.ptr(dO), u.ptr(L), u.ptr(dQKV),
           B, H, S, HE, scale, u.stream())
    u.sync()
    dQ, dK, dV, _ = p.backward(scale)
    X.assert_written(dQKV, B * S, "dQKV")
    X.assert_guard(dQKV, B * S, "dQKV")
    want = torch.cat([p.flat(t) for t in (dQ, dK, dV)], 1)
    for i, name in enumerate(("dQ", "dK", "dV")):
        X.assert_bitwise(dQKV[:B * S, i * E:(i + 1) * E], X.rne(want[:, i * E:(i + 1) * E], dt), name)


POW2 = {"perm": 1 / 8, "tie2a": 1 / 16, "tie2b": 1 / 8, "tie2c": 1 / 16, "tie4": 1 / 8, "sum": 1 / 16}
KINDS = list(POW2)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("HE", [32, 64, 96])
def test_attention_every_S(HE, kind):
    """vg_attention_fwd + _bwd at S = 1..256 with a power-of-two scale (exact dS), and the forward at 1/sqrt(HE)"""
    def one(S):
        p = _probe(S, HE, kind)
        p.check_preconditions([POW2[kind], 1 / math.sqrt(HE)])
        _bwd(p, POW2[kind])
        _fwd(p, 1 / math.sqrt(HE))
    X.collect(list(range(1, 257)), one, "S=")


def test_attention_generator_scale():
    """the v1 generator's 1/sqrt(H * HE) = 1/sqrt(128) (gap 362): forward at every S of its patch grids"""
    def one(S):
        p = _probe(S, 32, "perm", 1)
        p.check_preconditions([1 / math.sqrt(128)])
        _fwd(p, 1 / math.sqrt(128))
    X.collect(list(range(1, 257)), one, "S=")


# ----------------------------------------------------------------------------------------------------------- CLS query
def _cls(p, scale):
    u = X.gpu()
    S, HE, E = p.S, p.HE, p.H * p.HE
    qkv = p.qkv.to(CUDA).to(BF)
    O = X.guarded(B, E, BF, CUDA)
    L = X.guarded(B * H, 1, F32, CUDA)
    u.call("vg_attention_cls_fwd", u.ptr(qkv), u.ptr(O), u.ptr(L), B, H, S, HE, scale, u.stream())
    u.sync()
    o = p.flat(p.forward()).reshape(B, S, E)[:, 0]
    X.assert_written(O, B, "O_cls")
    X.assert_guard(O, B, "O_cls")
    X.assert_written(L, B * H, "LSE_cls")
    X.assert_guard(L, B * H, "LSE_cls")
    X.assert_bitwise(O[:B], X.rne(o, BF), "O_cls")
    _check_lse(L[:B * H, 0].reshape(B, H, 1), p, scale, "LSE_cls", slice(0, 1))
    dO = torch.zeros_like(p.dO)
    dO[:, :, 0] = p.dO[:, :, 0]
    dOc = p.flat(dO).reshape(B, S, E)[:, 0].contiguous().to(CUDA).to(BF)
    dQKV = X.guarded(B * S, 3 * E, BF, CUDA)
    u.call("vg_attention_cls_bwd", u.ptr(qkv), u.ptr(O), u.ptr(dOc), u.ptr(L), u.ptr(dQKV), B, H, S, HE, scale, u.stream())
    u.sync()
    dQ, dK, dV, _ = p.backward(scale, dO)
    X.assert_written(dQKV, B * S, "dQKV")
    X.assert_guard(dQKV, B * S, "dQKV")
    want = torch.cat([p.flat(t) for t in (dQ, dK, dV)], 1)
    for i, name in enumerate(("dQ", "dK", "dV")):
        X.assert_bitwise(dQKV[:B * S, i * E:(i + 1) * E], X.rne(want[:, i * E:(i + 1) * E], BF), name)


@pytest.mark.parametrize("kind", ["perm", "tie2a", "sum"])
@pytest.mark.parametrize("HE", [32, 64, 96])
def test_attention_cls_every_S(HE, kind):
    """vg_attention_cls_fwd + _bwd at S = 1..256: the 128-key instance up to 128, the 256-key one above"""
    def one(S):
        p = _probe(S, HE, kind, 2)
        p.check_preconditions([POW2[kind]])
        _cls(p, POW2[kind])
    X.collect(list(range(1, 257)), one, "S=")


# ------------------------------------------------------------------------------------------------------------ fp32 mode
@pytest.mark.parametrize("HE", [32, 64, 96])
def test_attention_f32_every_S(HE):
    """vg_attention_f32_fwd + _bwd at S = 1..80: the permutation probe forward and backward (P is exactly 0 or 1, so even
    the fp32 dS is exact), 2- and 4-way ties forward (P = 1/2, 1/4 only up to the rounding of log t in LSE: backward not
    bitwise in fp32)"""
    def one(S):
        p = _probe(S, HE, "perm", 3)
        p.check_preconditions([1 / 8])
        _bwd(p, 1 / 8, f32=True)
        for kind in ("tie2a", "tie2c", "tie4", "sum"):
            q = _probe(S, HE, kind, 3)
            q.check_preconditions([1 / 16, 1 / math.sqrt(HE)])
            _fwd(q, 1 / 16, f32=True)
            _fwd(q, 1 / math.sqrt(HE), f32=True)
    X.collect(list(range(1, 81)), one, "S=")
