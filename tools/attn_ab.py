#!/usr/bin/env python3
"""A/B of attention builds in ONE process (cdna_hip_programming.md rule 24): the libraries given on the command line are loaded
side by side, each by path, and timed in interleaved rounds at the attention shapes of the step; prints the median / min us per
launch per line and build.  Give the parent's library, a byte copy of it and the new one (the gap between the two copies is the
noise figure), and run it in three orders of the three.  With ROLES naming the libraries in the order given (parent, copy, new) every
line also gets its limit - the slower parent copy's median + the A/A gap |parent - copy| - a "+x" where the new median is above it,
and the run ends with the lines above their limit.

    ROLES=parent,copy,new ROUNDS=21 REPS=40 python tools/attn_ab.py parent.so parent_copy.so vit-gan_amd/libvitgan_hip.so
Only the single-operator attention entry points are called (their signatures are stable since ABI 7)."""
import ctypes as C
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (first: one HIP runtime for torch and the libraries)
import vit_gan_amd  # noqa: F401,E402
from vit_gan_amd import _lib  # noqa: E402

BF = torch.bfloat16
libs = []
for path in sys.argv[1:]:
    h = _lib.bind(C.CDLL(os.path.abspath(path)), [stem + end for stem in ("vg_attention", "vg_attention_fp8", "vg_attention_l2", "vg_attention_cls")
                                                  for end in ("_fwd", "_bwd")] + ["vg_attention_bwd_bwd"])
    libs.append((f"{len(libs)}:{path}", h))  # (the position keeps two paths with the same tail apart)
st, p = _lib.stream(), _lib.ptr
ROUNDS, REPS = int(os.environ.get("ROUNDS", "7")), int(os.environ.get("REPS", "20"))
ONLY = os.environ.get("ONLY", "")  # time only the lines whose name contains this
ROLES = os.environ.get("ROLES", "").split(",") if os.environ.get("ROLES") else None
assert ROLES is None or sorted(ROLES) == ["copy", "new", "parent"] and len(libs) == 3, "ROLES names three libraries: parent, copy, new"
above = []


def bench(name, make):
    """make(h) -> the launch of library h; every launch must return 0"""
    if ONLY not in name:
        return
    calls = [(n, make(h)) for n, h in libs]
    res = {n: [] for n, _ in libs}
    for n, fn in calls:
        for _ in range(3):
            rc = fn()
            assert rc == 0, (name, n, rc)
    for _ in range(ROUNDS):
        for n, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[n].append(e0.elapsed_time(e1) / REPS * 1e3)
    line = f"{name:30s}"
    for n, _ in libs:
        line += f" | {n[-28:]:>28s} {statistics.median(res[n]):7.2f} us (min {min(res[n]):6.2f})"
    if ROLES:
        med = {r: statistics.median(res[n]) for r, (n, _) in zip(ROLES, libs)}
        limit = max(med["parent"], med["copy"]) + abs(med["parent"] - med["copy"])
        over = med["new"] - limit
        line += f" | limit {limit:7.2f}" + (f" +{over:.2f}" if over > 0 else "")
        if over > 0:
            above.append(name)
    print(line, flush=True)


def pair(name, stem, B, H, S, HE, cls=False):
    """forward and backward of one entry-point pair at one shape"""
    E, scale = H * HE, 1.0 / math.sqrt(HE)
    g = torch.Generator().manual_seed(B + S)
    rows = B if cls else B * S
    qkv = torch.randn(B * S, 3 * E, generator=g).to(BF).cuda()
    d_o = torch.randn(rows, E, generator=g).to(BF).cuda()
    o = torch.empty(rows, E, device="cuda", dtype=BF)
    lse = torch.empty(rows * H, device="cuda")
    dqkv = torch.empty_like(qkv)
    shape = f"B{B} H{H} S{S} HE{HE}"
    assert getattr(libs[0][1], stem + "_fwd")(p(qkv), p(o), p(lse), B, H, S, HE, scale, st) == 0  # o and lse for the backward, whatever ONLY is
    bench(f"{name} fwd {shape}", lambda h: lambda: getattr(h, stem + "_fwd")(p(qkv), p(o), p(lse), B, H, S, HE, scale, st))
    bench(f"{name} bwd {shape}", lambda h: lambda: getattr(h, stem + "_bwd")(p(qkv), p(o), p(d_o), p(lse), p(dqkv), B, H, S, HE, scale, st))
    return qkv, d_o, lse, scale


HOT = (512, 4, 65, 96)  # the step's hot shape
qkv, d_o, lse, scale = pair("dot", "vg_attention", *HOT)  # (kept for the double backward below)
pair("dot", "vg_attention", 512, 4, 32, 96)      # the four-image backward at two tiles
pair("fp8", "vg_attention_fp8", *HOT)
pair("l2 ", "vg_attention_l2", *HOT)             # the four-image backward at five tiles
pair("l2 ", "vg_attention_l2", 512, 8, 65, 64)
pair("long", "vg_attention", 64, 12, 197, 64)
pair("cls", "vg_attention_cls", *HOT, cls=True)
B, H, S, HE = HOT
uqkv = torch.randn(B * S, 3 * H * HE, generator=torch.Generator().manual_seed(7)).to(BF).cuda()
d_do, d_qkv = torch.empty_like(d_o), torch.empty_like(qkv)
bench(f"bwd_bwd B{B} H{H} S{S} HE{HE}",
      lambda h: lambda: h.vg_attention_bwd_bwd(p(qkv), p(d_o), p(lse), p(uqkv), p(d_do), p(d_qkv), B, H, S, HE, scale, st))
if ROLES:
    print(f"lines above their limit: {len(above)}" + (": " + "; ".join(above) if above else ""))
