"""Byte pins of the attention entry points (a plain helper module, imported like host_pins).

Every case of ``digest_cases()`` makes one call per entry point through the raw C ABI on inputs built on the CPU from a seeded
generator (randn rounded to bf16, as tools/micro/attn_bwd_sum.py builds them), with every output pre-filled with the byte 0xA5 so
that bytes nobody writes are pinned too, and yields the SHA-256 of the raw bytes of each output: ``o`` and ``lse`` of the forward,
``dqkv`` of the backward, ``d_do`` and ``d_qkv`` of the double backward.
``python tests/attn_pins.py --write-gpu [commit id]`` runs every case three times, refuses a digest that differs between runs, and
records tests/golden/attn_digest.json with the commit and the hipcc version; select the library of that commit with VITGAN_HIP_LIB.
tests/test_attn_digest_gpu.py recomputes with the tree's library and compares with no tolerance.

B = 9 (not a multiple of 8: the ``b < B`` tail of the padded grid) and H = 2 (two heads share cache lines) throughout, every head
dim, scale 1 / sqrt(HE).  The sequence lengths are the smallest at which each branch can go wrong:
  short kernels (dot-product, fp8, L2)  1: a single key; 17: one key in the second tile of the 2-tile instance; 32: that instance
      full; 33, 65: one key in a tile of the 5-tile instance, an odd tile count whose last pair is half zero; 80: that instance full
  long kernels  81: the first long S, 6 waves, last pair half padding; 129: 9 tiles on 8 waves (wave 0 takes two); 256: the maximum
  CLS kernels   65, 128: the 128-key instance and its last S; 129: the first S of the 256-key instance
"""
import hashlib
import math
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:  # run as a script: the package is found like under pytest
    sys.path.insert(0, os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "golden", "attn_digest.json")

B, H = 9, 2
HEAD_DIMS = (32, 64, 96)
SHORT_S = (1, 17, 32, 33, 65, 80)
LONG_S = (81, 129, 256)
CLS_S = (65, 128, 129)
BWD_BWD_S = (17, 65, 80)
PAIRS = {"dot": ("vg_attention_fwd", "vg_attention_bwd"), "fp8": ("vg_attention_fp8_fwd", "vg_attention_fp8_bwd"),
         "l2": ("vg_attention_l2_fwd", "vg_attention_l2_bwd"), "cls": ("vg_attention_cls_fwd", "vg_attention_cls_bwd")}


def digest_cases():
    """{case id: (kind, S, HE)}; kind is a key of PAIRS or "bwd_bwd" """
    cases = {}
    for kind, lengths in (("dot", SHORT_S), ("fp8", SHORT_S), ("l2", SHORT_S), ("dot", LONG_S), ("cls", CLS_S), ("bwd_bwd", BWD_BWD_S)):
        for S in lengths:
            for HE in HEAD_DIMS:
                cases[f"{kind}/S{S}/HE{HE}"] = (kind, S, HE)
    return cases


def _sha(t):
    import torch
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _sentinel(n, dtype):
    """n elements of dtype whose every byte is 0xA5"""
    import torch
    return torch.full((n * torch.empty(0, dtype=dtype).element_size(),), 0xA5, dtype=torch.uint8, device="cuda").view(dtype)


def digest(case_id):
    import torch
    import gpu_util as u
    kind, S, HE = digest_cases()[case_id]
    E, scale = H * HE, 1.0 / math.sqrt(HE)
    g = torch.Generator().manual_seed(1000 * S + HE)
    bf = torch.bfloat16
    qkv = torch.randn(B * S, 3 * E, generator=g).to(bf).cuda()
    rows = B if kind == "cls" else B * S  # the CLS kernels see one query per image
    d_o = torch.randn(rows, E, generator=g).to(bf).cuda()
    o, lse, dqkv = _sentinel(rows * E, bf), _sentinel(rows * H, torch.float32), _sentinel(B * S * 3 * E, bf)
    fwd, bwd = PAIRS["dot" if kind == "bwd_bwd" else kind]
    u.call(fwd, u.ptr(qkv), u.ptr(o), u.ptr(lse), B, H, S, HE, scale, u.stream())
    if kind == "bwd_bwd":
        uqkv = torch.randn(B * S, 3 * E, generator=g).to(bf).cuda()
        d_do = _sentinel(B * S * E, bf)
        u.call("vg_attention_bwd_bwd", u.ptr(qkv), u.ptr(d_o), u.ptr(lse), u.ptr(uqkv), u.ptr(d_do), u.ptr(dqkv), B, H, S, HE, scale, u.stream())
        u.sync()
        return {"d_do": _sha(d_do), "d_qkv": _sha(dqkv)}
    u.call(bwd, u.ptr(qkv), u.ptr(o), u.ptr(d_o), u.ptr(lse), u.ptr(dqkv), B, H, S, HE, scale, u.stream())
    u.sync()
    return {"o": _sha(o), "lse": _sha(lse), "dqkv": _sha(dqkv)}


def main(argv):
    if argv[:1] != ["--write-gpu"]:
        raise SystemExit("usage: python tests/attn_pins.py --write-gpu [commit id]")
    import host_pins as hp
    if len(argv) < 2 and os.environ.get("VITGAN_HIP_LIB"):
        raise SystemExit("VITGAN_HIP_LIB selects another build's library: name the commit it was built from")
    commit = argv[1] if len(argv) > 1 else hp.head_commit()
    hipcc = subprocess.run(["hipcc", "--version"], capture_output=True, text=True).stdout
    version = next((ln.strip() for ln in hipcc.splitlines() if "HIP version" in ln), "")
    doc = {"commit": commit, "hipcc": version, "digests": {}}
    for case_id in digest_cases():
        runs = [digest(case_id) for _ in range(3)]
        if runs[1] != runs[0] or runs[2] != runs[0]:
            raise SystemExit(f"{case_id}: digests differ between runs at the recording commit: {runs}")
        doc["digests"][case_id] = runs[0]
        print(case_id, "ok", flush=True)
    hp._dump(doc, FIXTURE, "digests")


if __name__ == "__main__":
    main(sys.argv[1:])
