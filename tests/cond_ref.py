"""Class conditioning restated off the device, from the text of include/vitgan_hip.h alone (a plain helper module, imported like
bcr_ref / diffaug_ref): the label hash in integer arithmetic, vg_class_add with bf16 round-to-nearest-even on the bit pattern,
vg_class_grad as fp32 sequential sums in ascending n, the label-selected loss in float64 and in the kernel's fp32 order, and the
conditional generator as ``oracle.gen_oracle.gen_forward`` on the extended latent [z ; onehot(y)] with the mapping weight
[W | table^T] - the classic cGAN input the gather stands for."""
import numpy as np
import torch

from drop_ref import M32, h, site_key  # noqa: F401  (the host key and the counter hash of the dropout masks)
KINDS = ("ns", "hinge", "wasserstein")  # kind 0, 1, 2
LABEL_SITE = 3                          # the fused step's draws: its augmentation seed, site 3


# ---------------------------------------------------------------------------------------------------------------- the label hash
def launch_key(seed: int, site: int, step) -> int:
    """ks = h(step_dev ? key ^ (step 0x9E3779B1 + 0x7F4A7C15) : key, 0); ``step`` None = no device counter"""
    key = site_key(seed, site)
    if step is not None:
        key ^= (int(step) * 0x9E3779B1 + 0x7F4A7C15) & M32
    return int(h(key, 0))


def draw_labels(n: int, K: int, seed: int, site: int, step) -> np.ndarray:
    """labels[i] = (k_i K) >> 24, k_i = h(ks, i) >> 8 (24 bits, so the product stays inside 32)"""
    k = h(launch_key(seed, site, step), np.arange(n, dtype=np.uint32)) >> np.uint32(8)
    return ((k.astype(np.uint64) * np.uint64(K)) >> np.uint64(24)).astype(np.int32)


# ------------------------------------------------------------------------------------------------------- the generator's table
def clamp(labels, K: int) -> np.ndarray:
    return np.clip(np.asarray(labels, dtype=np.int64), 0, K - 1)


def bf16_rne_bits(x32: np.ndarray) -> np.ndarray:
    """fp32 -> the 16 bits of its bf16, round to nearest even on the bit pattern (finite inputs)"""
    b = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def bf16_bits_to_f32(b16: np.ndarray) -> np.ndarray:
    return (b16.astype(np.uint32) << np.uint32(16)).view(np.float32)


def bits_of(t: torch.Tensor) -> np.ndarray:
    """the 16-bit patterns of a bf16 tensor"""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def class_add(wmod_bits: np.ndarray, table_bits: np.ndarray, labels) -> np.ndarray:
    """bf16 bit patterns [B, N], [K, N] -> the bit patterns of bf16(float(wmod) + float(table[y])): one fp32 addition, one rounding"""
    y = clamp(labels, table_bits.shape[0])
    return bf16_rne_bits(bf16_bits_to_f32(wmod_bits) + bf16_bits_to_f32(table_bits)[y])


def class_grad(dw: np.ndarray, labels, K: int, into: np.ndarray = None) -> np.ndarray:
    """fp32: one accumulator per output element from +0 over the rows of its class in ascending n; ``into``: accumulate (one more
    addition, a class without a sample untouched), else overwrite (such a class +0)."""
    dw = np.asarray(dw, dtype=np.float32)
    y = clamp(labels, K)
    out = np.zeros((K, dw.shape[1]), dtype=np.float32) if into is None else np.array(into, dtype=np.float32, copy=True)
    for k in range(K):
        acc, seen = np.zeros(dw.shape[1], dtype=np.float32), False
        for n in range(dw.shape[0]):
            if y[n] == k:
                acc, seen = (acc + dw[n]).astype(np.float32), True
        if into is None:
            out[k] = acc
        elif seen:
            out[k] = (out[k] + acc).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------------ the label-selected loss
def _terms(x, kind: int, role: int, xp):
    """(loss term, d loss term / d x) of vg_gan_loss_body for the values x, in xp's precision (numpy float64 or float32)"""
    t = 0.0 if role == 1 else 1.0
    sgn = 1.0 if role == 1 else -1.0
    one = x.dtype.type(1)
    if kind == 0:
        l = np.maximum(x, 0) - x * x.dtype.type(t) + np.log1p(np.exp(-np.abs(x)))
        d = one / (one + np.exp(-x)) - x.dtype.type(t)
    elif kind == 1:
        hm = one + x.dtype.type(sgn) * x
        l = -x if role == 2 else np.maximum(hm, 0)
        d = np.full_like(x, -1) if role == 2 else np.where(hm > 0, x.dtype.type(sgn), x.dtype.type(0))
    else:
        l = x if role == 1 else -x
        d = np.full_like(x, 1 if role == 1 else -1)
    return l.astype(x.dtype), d.astype(x.dtype)


def cond_loss64(logits, labels, kind: int, role: int, grad_scale: float = 1.0):
    """float64: (loss, dlogits [n, Kc], selected [n]) - the mean over the n selected logits, zeros off the label"""
    lg = np.asarray(logits, dtype=np.float64)
    n, Kc = lg.shape
    y = clamp(labels, Kc)
    s = lg[np.arange(n), y]
    l, d = _terms(s, kind, role, np)
    dl = np.zeros_like(lg)
    dl[np.arange(n), y] = d / n * grad_scale
    return float(l.sum() / n), dl, s


def cond_loss32(logits, labels, kind: int, role: int, grad_scale: float = 1.0):
    """the same in the kernel's fp32 order: inv = fl(1 / n); thread t of 256 chains the samples t, t + 256, ...; each wave of 64 sums
    by the xor butterfly (offsets 32 .. 1); the four waves in order; one product with inv.  d_i inv grad_scale left to right."""
    f = np.float32
    lg = np.asarray(logits, dtype=f)
    n, Kc = lg.shape
    y = clamp(labels, Kc)
    s = lg[np.arange(n), y]
    l, d = _terms(s, kind, role, np)
    inv = f(1.0) / f(n)
    acc = np.zeros(256, dtype=f)
    for i in range(n):
        acc[i % 256] = f(acc[i % 256] + l[i])
    w = acc.reshape(4, 64).copy()
    for o in (32, 16, 8, 4, 2, 1):
        w = (w + w[:, np.arange(64) ^ o]).astype(f)
    loss = f(f(f(f(w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]) * inv)
    dl = np.zeros_like(lg)
    dl[np.arange(n), y] = (d * inv).astype(f) * f(grad_scale)
    return loss, dl, s


def torch_cond_loss(logits: torch.Tensor, labels: torch.Tensor, kind: str, role: int) -> torch.Tensor:
    """the autograd form: the step oracle's loss functions on logits.gather(1, y)"""
    from oracle import step_oracle as so
    s = logits.gather(1, labels.long().reshape(-1, 1)).reshape(-1)
    return (so.d_loss_real, so.d_loss_fake, so.g_loss)[role](s, kind)


# ----------------------------------------------------------------------------------------------------- the conditional generator
def extended_state(state, table: torch.Tensor):
    """the generator's state with the mapping weight [W | table^T]: latent Z + K"""
    st = dict(state)
    st["mapping_mlp.model.0.0.weight"] = torch.cat([state["mapping_mlp.model.0.0.weight"], table.t()], dim=1)
    return st


def extended_latent(z: torch.Tensor, labels, K: int) -> torch.Tensor:
    """z_ext = [z ; onehot(y)]"""
    return torch.cat([z, torch.nn.functional.one_hot(torch.as_tensor(labels).long(), K).to(z.dtype)], dim=1)


def gen_forward_gather(state, table: torch.Tensor, z: torch.Tensor, labels, d, **kw) -> torch.Tensor:
    """w = mapping(z) + table[y] as the module computes it: the oracle's forward with the gathered rows folded into the mapping bias
    per sample is not expressible there, so the gather is applied through a batch of one-sample calls' biases - here simply by the
    identity  Linear(z) + table[y] = Linear_b'(z)  with b' = b + table[y], one sample at a time."""
    from oracle import gen_oracle as go
    outs = []
    for n in range(z.shape[0]):
        st = dict(state)
        st["mapping_mlp.model.0.0.bias"] = state["mapping_mlp.model.0.0.bias"] + table[int(labels[n])]
        outs.append(go.gen_forward(st, z[n:n + 1], d, **kw))
    return torch.cat(outs)
