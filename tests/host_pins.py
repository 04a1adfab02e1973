"""Pins of the C host code that sequences the two networks (a plain helper module, imported like step_trace).

Pin A, the carve table (no GPU): for every geometry below and every batch of ``BATCHES`` the three workspace sizes, every field of
``vg_vit_ws_map`` / ``vg_gen_ws_map`` and every field of ``vg_vit_layout`` / ``vg_gen_layout``.
``python tests/host_pins.py --write`` records tests/golden/host_carve.json; tests/test_host_pins_cpu.py recomputes and compares.

Pin B, byte digests (GPU): every case of ``digest_cases()`` runs forward and backward (or the penalty) through the raw C ABI on
inputs built on the CPU from seeded generators, with every workspace pre-filled with the byte 0xA5 and the gradient buffer
pre-filled with seeded values of size 1e-3, and yields the SHA-256 of the raw bytes of each output and of each WHOLE workspace
after the last call.  The workspace digest is what makes this a launch-level pin: a dropped, added or reordered launch, a wrong
block stride or a wrong scratch set changes some saved activation or scratch tensor.
``python tests/host_pins.py --write-gpu`` runs every case three times, refuses a digest that differs between runs, and records
tests/golden/host_digest.json; tests/test_host_digest_gpu.py recomputes and compares.

The generator lines G1-G3 are legal geometries as given (``vg_gen_layout`` returns 0); their ``CW`` is the one the geometry
determines, C * IH without a patch grid and C * patch^2 with one, as in tests/test_net_gpu.py.
"""
import ctypes as C
import functools
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:  # run as a script: the package is found like under pytest
    sys.path.insert(0, os.path.dirname(HERE))
CARVE_FIXTURE = os.path.join(HERE, "golden", "host_carve.json")
DIGEST_FIXTURE = os.path.join(HERE, "golden", "host_digest.json")

# (C, IH, P, E, H, L, R, Kc): the smallest shapes at which each branch of the host code is taken
VIT = {
    "V1": (3, 32, 4, 384, 4, 3, 2, 1),    # S = 65: fused embedding, full-row path and tail, an odd block left over from the pairing
    "V2": (3, 28, 4, 384, 4, 2, 2, 1),    # S = 50: full-row path whose tail takes the tiled form at B = 8
    "V3": (3, 64, 8, 512, 8, 2, 4, 10),   # unfused embedding, width-512 full-row kernels, mlp ratio 4, ten classes
    "V4": (3, 32, 4, 128, 4, 2, 2, 20),   # tiled everywhere, Kc > 16 (no head partial rows)
    "V5": (3, 32, 4, 384, 4, 1, 2, 1),    # one block
    "V6": (3, 36, 4, 384, 4, 2, 2, 1),    # S = 82: the long-attention kernels
}
# (Z, T, E, H, L, O, CW, omega0, patch, C, IH)
GEN = {
    "G1": (1024, 32, 384, 4, 3, 768, 96, 30.0, 0, 3, 32),
    "G2": (256, 64, 256, 4, 2, 256, 48, 30.0, 4, 3, 32),  # tiled, patch-grid output
    "G3": (1024, 32, 512, 8, 3, 768, 96, 30.0, 0, 3, 32),
}
BATCHES = (1, 4, 8, 16, 256)
SEED, STEP = 11, 3  # dropout seed and the value of the device dropout counter


def _L():
    import vit_gan_amd  # noqa: F401
    from vit_gan_amd import _lib
    return _lib


def _fields(s):
    return {n: (list(getattr(s, n)) if isinstance(getattr(s, n), C.Array) else getattr(s, n)) for n, _ in s._fields_}


def head_commit():
    return subprocess.run(["git", "-C", HERE, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()


# ------------------------------------------------------------------ pin A: the carve table
def carve_table():
    """{"V1/B4": {...}, "G1/B4": {...}, ...} in the form json.load gives back"""
    L = _L()
    lib = L.lib()
    out = {}
    for name, geo in VIT.items():
        d = L.VgVitDims(*geo)
        lay = L.VgVitLayout()
        assert lib.vg_vit_layout(C.byref(d), C.byref(lay)) == 0, name
        for B in BATCHES:
            m = L.VgVitWsMap()
            assert lib.vg_vit_ws_map(C.byref(d), B, C.byref(m)) == 0, (name, B)
            out[f"{name}/B{B}"] = {"ws_bytes": lib.vg_vit_ws_bytes(C.byref(d), B), "penalty_ws_bytes": lib.vg_vit_penalty_ws_bytes(C.byref(d), B),
                                   "ws_map": _fields(m), "layout": _fields(lay)}
    for name, geo in GEN.items():
        d = L.VgGenDims(*geo)
        lay = L.VgGenLayout()
        assert lib.vg_gen_layout(C.byref(d), C.byref(lay)) == 0, name
        for B in BATCHES:
            m = L.VgGenWsMap()
            assert lib.vg_gen_ws_map(C.byref(d), B, C.byref(m)) == 0, (name, B)
            out[f"{name}/B{B}"] = {"ws_bytes": lib.vg_gen_ws_bytes(C.byref(d), B), "ws_map": _fields(m), "layout": _fields(lay)}
    return json.loads(json.dumps(out))


# ------------------------------------------------------------------ pin B: the digest cases
def digest_cases():
    """{case id: (kind, parameters)}; kind is "vit", "pen" or "gen" """
    cases = {}

    def vit(geo, B, drop, dense=0, fp8=0, wgrad=1, dimg=1, bf16=1, ctx=0, mode="one"):
        key = f"vit/{geo}/B{B}/p{drop}/dense{dense}/fp8{fp8}/wgrad{wgrad}/dimg{dimg}/bf16{bf16}/ctx{ctx}/{mode}"
        cases[key] = ("vit", dict(geo=geo, B=B, drop=drop, dense=dense, fp8=fp8, wgrad=wgrad, dimg=dimg, bf16=bf16, ctx=ctx, mode=mode))

    # V1 at B = 16: dropout x dense_top x attn_fp8 x ctx x backward form in full; each of want_wgrad = 0, d_img = null and an fp32
    # image crossed with dropout x dense_top x ctx (the three change launches the other options do not touch)
    for drop in (0.0, 0.1):
        for dense in (0, 1):
            for ctx in (0, 1):
                for fp8 in (0, 1):
                    for mode in ("one", "stages", "pieces"):
                        vit("V1", 16, drop, dense=dense, fp8=fp8, ctx=ctx, mode=mode)
                vit("V1", 16, drop, dense=dense, ctx=ctx, wgrad=0)
                vit("V1", 16, drop, dense=dense, ctx=ctx, dimg=0)
                vit("V1", 16, drop, dense=dense, ctx=ctx, bf16=0)
    for geo, B in (("V1", 4), ("V2", 8), ("V3", 16), ("V4", 4), ("V5", 16), ("V6", 8)):
        for dense in (0, 1):
            vit(geo, B, 0.1, dense=dense)
    for geo, B in (("V1", 16), ("V1", 4), ("V3", 16), ("V4", 8), ("V5", 16)):
        for r1 in (0, 1):
            for drop in (0.0, 0.1):
                cases[f"pen/{geo}/B{B}/{'r1' if r1 else 'gp'}/p{drop}"] = ("pen", dict(geo=geo, B=B, r1=r1, drop=drop))
    for geo, B in (("G1", 4), ("G1", 1), ("G2", 4), ("G3", 4)):
        for drop in (0.0, 0.1):
            for pos in (0, 1):
                for mode in ("one", "pieces"):
                    cases[f"gen/{geo}/B{B}/p{drop}/pos{pos}/{mode}"] = ("gen", dict(geo=geo, B=B, drop=drop, pos=pos, mode=mode))
    return cases


def _gen(seed):
    import torch
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=2)
def _vit_params(geo):
    """(dims struct, layout, fp32 master on the device, bf16 shadow): init of the oracle, matrices scaled by 2.5 as in test_fullsize_gpu.py"""
    import torch
    from oracle import vit_oracle as vo
    from vit_gan_amd import flat
    L = _L()
    c, ih, p, e, h, l, r, kc = VIT[geo]
    d = vo.VitDims(channels=c, image=ih, patch=p, embed=e, heads=h, layers=l, mlp_ratio=r, classes=kc)
    st = {k: (v * 2.5 if v.dim() > 1 else v) for k, v in vo.init_vit_state(d, seed=7).items()}
    gd = L.VgVitDims(*VIT[geo])
    lay = flat.vit_layout(gd)
    P = flat.pack(flat.vit_slots(gd), lay.total, {k: v.numpy() for k, v in st.items()}, device="cuda")
    return gd, lay, P, P.to(torch.bfloat16)


@functools.lru_cache(maxsize=1)
def _gen_params(geo):
    import torch
    from oracle import gen_oracle as go
    from vit_gan_amd import flat
    L = _L()
    z, t, e, h, l, o, cw, w0, patch, c, ih = GEN[geo]
    d = go.GenDims(latent=z, tokens=t, embed=e, heads=h, layers=l, siren_hidden=o, channels=c, image=ih, omega0=w0, patch=patch)
    assert d.out_features == cw, geo
    st = {k: (v * 2.5 if v.dim() > 1 and v.numel() > 1 else v) for k, v in go.init_gen_state(d, seed=7).items()}
    gd = L.VgGenDims(*GEN[geo])
    lay = flat.gen_layout(gd)
    P = flat.pack(flat.gen_slots(gd), lay.total, {k: v.numpy() for k, v in st.items()}, device="cuda")
    return gd, lay, P, P.to(torch.bfloat16)


def _sha(t):
    import torch
    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _filled(nbytes):
    import torch
    return torch.full((int(nbytes),), 0xA5, dtype=torch.uint8, device="cuda")


def _grad_buffer(total):
    import torch
    return (torch.randn(total, generator=_gen(5)) * 1e-3).cuda()


def _pieces(mode, L_, lay):
    from vit_gan_amd.dist import backward_pieces
    if mode == "one":
        return None
    if mode == "stages":
        return [(0, 1), (1, L_ + 1), (L_ + 1, L_ + 2)]
    return [(a, b) for a, b, _, _ in backward_pieces(L_, 3, lay.layer0, lay.layer_stride, lay.total)]


def _step_counter():
    import torch
    return torch.tensor([STEP], dtype=torch.int32, device="cuda")


def run_vit(geo, B, drop, dense, fp8, wgrad, dimg, bf16, ctx, mode):
    import torch
    import gpu_util as u
    L = _L()
    gd, lay, P, Pb = _vit_params(geo)
    c, ih, kc = gd.C, gd.IH, gd.Kc
    x = torch.rand(B, c, ih, ih, generator=_gen(3)) * 2 - 1
    xd = (x.to(torch.bfloat16) if bf16 else x).cuda().contiguous()
    dl = (torch.randn(B, kc, generator=_gen(4)) / B).cuda()
    G = _grad_buffer(lay.total)
    step = _step_counter()
    net = L.VgVitNet(gd, P.data_ptr(), Pb.data_ptr(), G.data_ptr(), drop, SEED, step.data_ptr(), L.context() if ctx else None, fp8, dense)
    ws = _filled(L.lib().vg_vit_ws_bytes(C.byref(gd), B))
    logits = torch.zeros(B, kc, device="cuda")
    d_img = torch.zeros(B, c, ih, ih, dtype=torch.bfloat16, device="cuda") if dimg else None
    u.call("vg_vit_forward", C.byref(net), B, u.ptr(xd), int(bf16), u.ptr(ws), u.ptr(logits), u.stream())
    pieces = _pieces(mode, gd.L, lay)
    if pieces is None:
        u.call("vg_vit_backward", C.byref(net), B, u.ptr(ws), u.ptr(dl), u.ptr(d_img), wgrad, u.stream())
    else:
        for a, b in pieces:
            u.call("vg_vit_backward_stages", C.byref(net), B, u.ptr(ws), u.ptr(dl), u.ptr(d_img), wgrad, a, b, u.stream())
    u.sync()
    out = {"logits": _sha(logits), "G": _sha(G), "ws": _sha(ws)}
    if dimg:
        out["d_img"] = _sha(d_img)
    return out


def run_pen(geo, B, r1, drop):
    import torch
    import gpu_util as u
    L = _L()
    gd, lay, P, Pb = _vit_params(geo)
    c, ih = gd.C, gd.IH
    real = (torch.rand(B, c, ih, ih, generator=_gen(3)) * 2 - 1).to(torch.bfloat16).cuda()
    fake = (torch.rand(B, c, ih, ih, generator=_gen(8)) * 2 - 1).to(torch.bfloat16).cuda()
    eps = torch.rand(B, generator=_gen(6)).cuda()
    G = _grad_buffer(lay.total)
    step = _step_counter()
    net = L.VgVitNet(gd, P.data_ptr(), Pb.data_ptr(), G.data_ptr(), drop, SEED, step.data_ptr(), None, 0, 0)
    ws = _filled(L.lib().vg_vit_ws_bytes(C.byref(gd), B))
    wp = _filled(L.lib().vg_vit_penalty_ws_bytes(C.byref(gd), B))
    out = torch.zeros(1, device="cuda")
    if r1:
        u.call("vg_vit_r1", C.byref(net), B, u.ptr(real), 10.0, u.ptr(ws), u.ptr(wp), u.ptr(out), u.stream())
    else:
        u.call("vg_vit_penalty", C.byref(net), B, u.ptr(real), u.ptr(fake), u.ptr(eps), 10.0, u.ptr(ws), u.ptr(wp), u.ptr(out), u.stream())
    u.sync()
    return {"penalty_out": _sha(out), "G": _sha(G), "ws": _sha(ws), "ws_pen": _sha(wp)}


def run_gen(geo, B, drop, pos, mode):
    import torch
    import gpu_util as u
    L = _L()
    gd, lay, P, Pb = _gen_params(geo)
    z = torch.randn(B, gd.Z, generator=_gen(3)).cuda()
    d_img = (torch.randn(B, gd.C, gd.IH, gd.IH, generator=_gen(4)) / B).to(torch.bfloat16).cuda()
    tab = (torch.randn(gd.T, gd.E, generator=_gen(9)) * 0.1).cuda() if pos else None
    G = _grad_buffer(lay.total)
    step = _step_counter()
    net = L.VgGenNet(gd, P.data_ptr(), Pb.data_ptr(), G.data_ptr(), drop, SEED, step.data_ptr(), None if tab is None else tab.data_ptr())
    ws = _filled(L.lib().vg_gen_ws_bytes(C.byref(gd), B))
    img = torch.zeros(B, gd.C, gd.IH, gd.IH, dtype=torch.bfloat16, device="cuda")
    u.call("vg_gen_forward", C.byref(net), B, u.ptr(z), u.ptr(ws), u.ptr(img), u.stream())
    pieces = _pieces(mode, gd.L, lay)
    if pieces is None:
        u.call("vg_gen_backward", C.byref(net), B, u.ptr(ws), u.ptr(d_img), u.stream())
    else:
        for a, b in pieces:
            u.call("vg_gen_backward_stages", C.byref(net), B, u.ptr(ws), u.ptr(d_img), a, b, u.stream())
    u.sync()
    return {"img": _sha(img), "G": _sha(G), "ws": _sha(ws)}


RUN = {"vit": run_vit, "pen": run_pen, "gen": run_gen}


def digest(case_id):
    kind, kw = digest_cases()[case_id]
    return RUN[kind](**kw)


# ------------------------------------------------------------------ recording
def _dump(doc, path, table):
    """one entry per line: the fixtures stay readable and their diffs small"""
    head = [f' {json.dumps(k)}: {json.dumps(v)},' for k, v in doc.items() if k != table]
    rows = [f'  {json.dumps(k)}: {json.dumps(v, separators=(",", ":"))}' for k, v in doc[table].items()]
    with open(path, "w") as f:
        f.write("\n".join(["{"] + head + [f' "{table}": {{', ",\n".join(rows), " }", "}", ""]))


def main(argv):
    if argv[:1] == ["--write"]:
        commit = argv[1] if len(argv) > 1 else head_commit()
        _dump({"commit": commit, "table": carve_table()}, CARVE_FIXTURE, "table")
        return
    if argv[:1] == ["--write-gpu"]:
        commit = argv[1] if len(argv) > 1 else head_commit()
        hipcc = subprocess.run(["hipcc", "--version"], capture_output=True, text=True).stdout
        version = next((ln.strip() for ln in hipcc.splitlines() if "HIP version" in ln), "")
        doc = {"commit": commit, "hipcc": version, "digests": {}}
        for case_id in digest_cases():
            runs = [digest(case_id) for _ in range(3)]
            if runs[1] != runs[0] or runs[2] != runs[0]:
                raise SystemExit(f"{case_id}: digests differ between runs at the recording commit: {runs}")
            doc["digests"][case_id] = runs[0]
            print(case_id, "ok", flush=True)
        _dump(doc, DIGEST_FIXTURE, "digests")
        return
    raise SystemExit("usage: python tests/host_pins.py --write | --write-gpu [commit id]")


if __name__ == "__main__":
    main(sys.argv[1:])
