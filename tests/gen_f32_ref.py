"""The network cases of the generator's fp32 mode and their oracle runs (a plain helper module, imported like cond_ref / norm_ref):
shared by test_gen_fp32_cpu.py, which shows that the bounds are admissible (float32 oracle against float64 oracle), and
test_gen_fp32_net_gpu.py, which applies them to vg_gen_forward_f32 / vg_gen_backward_f32.  Every oracle run is computed once per process.

Bounds (the discriminator mode's, tests/test_fp32_net_gpu.py):  image |d| <= 1e-5 + 1e-4 |ref| elementwise;  every gradient
|d| <= 1e-3 |ref| + 1e-5 max|ref| elementwise.  No generator parameter has a zero true gradient (q, k, v carry no bias): nothing is skipped.
"""
import functools

import numpy as np
import torch

CLASS_KEY = "class_embedding.weight"

# name -> geometry.  golden: the reference's default network with the recorded weights of tests/golden (GEN_CASES).  Others: the
# oracle's init at `seed`.  patch 0 = the v1 row tokens.  Head widths 96 (g1, cond), 32 (p32, fourier), 64 (p64, drop) all occur.
CASES = {
    "g1": dict(golden="g1"),
    "g1b3": dict(golden="g1b3"),
    "p32": dict(image=32, patch=4, embed=128, heads=4, layers=2, latent=256, siren=256, batch=3, seed=11),
    "p64": dict(image=64, patch=8, embed=512, heads=8, layers=2, latent=256, siren=256, batch=2, seed=12),
    "fourier": dict(image=32, patch=4, embed=128, heads=4, layers=1, latent=128, siren=128, batch=3, seed=13, fourier=True),
    "cond": dict(image=32, patch=0, embed=384, heads=4, layers=1, latent=64, siren=128, batch=4, seed=14, K=3, labels=(2, 0, 2, 0)),  # class 1 absent
    "drop": dict(image=32, patch=0, embed=256, heads=4, layers=2, latent=128, siren=256, batch=3, seed=15, dropout=0.2, drop_seed=24681357),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(d, B, st_np, z, R, pos_table, K, labels, table, dropout, drop_seed): numpy / torch float32 inputs of the case"""
    from cases import GEN_CASES
    from weights import make_input, make_state
    from oracle import gen_oracle as go
    c = CASES[name]
    if "golden" in c:
        g = GEN_CASES[c["golden"]]
        d, B, seed = go.GenDims(), g["batch"], g["seed"]
        st_np = make_state(go.gen_param_shapes(d), seed, "gen")
        z = torch.from_numpy(make_input((B, d.latent), seed))
        R = torch.from_numpy(make_input((B, d.channels, d.image, d.image), seed + 1))
    else:
        P, IH = c["patch"], c["image"]
        d = go.GenDims(latent=c["latent"], tokens=(IH // P) ** 2 if P else IH, embed=c["embed"], heads=c["heads"], layers=c["layers"],
                       siren_hidden=c["siren"], channels=3, image=IH, patch=P)
        B, seed = c["batch"], c["seed"]
        st_np = {k: v.numpy() for k, v in go.init_gen_state(d, seed=seed).items()}
        z = torch.from_numpy(make_input((B, d.latent), seed))
        R = torch.from_numpy(make_input((B, 3, IH, IH), seed + 1))
    out = dict(d=d, B=B, st_np=st_np, z=z, R=R, pos_table=None, K=0, labels=None, table=None, dropout=c.get("dropout", 0.0),
               drop_seed=c.get("drop_seed", 0))
    if c.get("fourier"):
        out["pos_table"] = go.fourier_position_table(d)
    if c.get("K"):
        g = torch.Generator().manual_seed(seed + 100)
        bound = 1.0 / np.sqrt(d.latent)  # the K extra input columns of the mapping Linear the table stands for
        out["K"], out["labels"] = c["K"], torch.tensor(c["labels"], dtype=torch.int32)
        out["table"] = ((torch.rand(c["K"], d.tokens * d.embed, generator=g) * 2 - 1) * bound).float()
    return out


def drop_sites(d):
    """(oracle mask key, engine site) of every dropout the generator applies: 100 + 2l behind output_linear, 101 + 2l inside the MLP"""
    return [(("attn", l), 100 + 2 * l) for l in range(d.layers)] + [(("mlp", l), 101 + 2 * l) for l in range(d.layers)]


def host_masks(name):
    """the case's dropout multipliers from the mask's definition (drop_ref): fp32 [B, T, E] per site, 0 or fl(256 / (256 - thr))"""
    import drop_ref
    c = case(name)
    if not c["dropout"]:
        return None
    d, B = c["d"], c["B"]
    m = {}
    for key, site in drop_sites(d):
        keep, scale = drop_ref.mask(c["dropout"], c["drop_seed"], site, None, B * d.tokens * d.embed)
        m[key] = torch.from_numpy(keep.astype(np.float32) * np.float32(scale)).reshape(B, d.tokens, d.embed)
    return m


def oracle_run(name, dtype, masks=None):
    """gen_oracle.gen_forward of the case in ``dtype`` with loss sum(out * R): (image, {parameter: gradient}), the class table's
    gradient under CLASS_KEY.  The conditional case runs the extended-latent oracle of cond_ref: [z ; onehot(y)] through [W | table^T]."""
    import cond_ref
    from oracle import gen_oracle as go
    c = case(name)
    d = c["d"]
    st = {k: torch.from_numpy(v).to(dtype) for k, v in c["st_np"].items()}
    z = c["z"].to(dtype)
    Z = z.shape[1]
    if c["K"]:
        st = cond_ref.extended_state(st, c["table"].to(dtype))
        z = cond_ref.extended_latent(z, c["labels"], c["K"])
    st = {k: v.clone().requires_grad_(True) for k, v in st.items()}
    mk = None if masks is None else {k: v.to(dtype) for k, v in masks.items()}
    tab = None if c["pos_table"] is None else c["pos_table"].to(dtype)
    out = go.gen_forward(st, z, d, masks=mk, pos_table=tab)
    (out * c["R"].to(dtype)).sum().backward()
    grads = {k: p.grad for k, p in st.items()}
    if c["K"]:
        gw = grads["mapping_mlp.model.0.0.weight"]
        grads["mapping_mlp.model.0.0.weight"], grads[CLASS_KEY] = gw[:, :Z].contiguous(), gw[:, Z:].t().contiguous()
    return out.detach(), grads


@functools.lru_cache(maxsize=None)
def oracle_f32(name):
    """the float32 oracle on the host masks (the reference of the GPU tests)"""
    return oracle_run(name, torch.float32, host_masks(name))


def image_ratio(got, ref):
    """max of |got - ref| / (1e-5 + 1e-4 |ref|)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    return float(((got - ref).abs() / (1e-5 + 1e-4 * ref.abs())).max())


def grad_ratio(got, ref):
    """max of |got - ref| / (1e-3 |ref| + 1e-5 max|ref|)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    top = float(ref.abs().max())
    assert top > 0.0, "a zero reference gradient: the bound would be empty"
    return float(((got - ref).abs() / (1e-3 * ref.abs() + 1e-5 * top)).max())
