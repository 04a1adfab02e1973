"""The reference's v1 generator (self-modulated LayerNorm blocks + SIREN output) on the HIP engine.

``SirenGenerator`` has the parameter tree - hence the ``state_dict`` keys and shapes - of
``src.v1.generator.Generator`` (src/v1/generator.py:12-55): mapping Linear(Z -> T*E), learned
embedding [T,E], L x TransformerSLN (two SLN, H bias-free per-head q/k/v, output Linear, single-Linear
MLP), final SLN, two SIREN layers; output ``[B, C, IH, IW]`` is the flat view of ``[B, T, C*IW]``.
Forward/backward are ONE C call each into the fused engine.

Dropout: the reference block applies Dropout(0.2) to the attention output and inside the MLP
(src/v1/config.py:36,39) in train mode; here both are fused into the GEMM epilogues (counter-based
mask, p quantised to 1/256) and are active in ``train()`` mode, identity in ``eval()`` - parity with the
reference is defined in eval mode, RNG streams cannot match.
"""
from __future__ import annotations

import ctypes as C
import math

import torch
import torch.nn as nn

from . import _lib, flat
from .flatparams import FlatParams


class _Holder(nn.Module):
    """Parameter container: exists only to give parameters their reference names."""


def _linear_holder(out_f, in_f, bias=True):
    h = _Holder()
    h.weight = nn.Parameter(torch.empty(out_f, in_f))
    if bias:
        h.bias = nn.Parameter(torch.empty(out_f))
    return h


def _mlp_holder(out_f, in_f):  # MLP(...).model = ModuleList([Sequential(Linear, Dropout)])
    m = _Holder()
    m.model = nn.ModuleList([nn.Sequential(_linear_holder(out_f, in_f), nn.Identity())])
    return m


def _sln_holder(E):
    s = _Holder()
    s.layer_norm = nn.LayerNorm(E)
    s.beta = nn.Parameter(torch.randn(1, 1, 1))
    s.gamma = nn.Parameter(torch.randn(1, 1, 1))
    return s


class _GenFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod: "SirenGenerator", z, anchor, drop_p, labels=None):
        fp = mod._flat
        fp.refresh_shadow()
        ctx.drop = (float(drop_p), int(torch.randint(0, 2 ** 62, (1,)).item()) if drop_p > 0 else 0)
        B = z.shape[0]
        zin = z.detach().float().contiguous()
        ws = torch.empty(mod._ws_bytes(B), dtype=torch.uint8, device=z.device)
        img = torch.empty(B, mod.channels, mod.image_size, mod.image_size, dtype=torch.bfloat16, device=z.device)
        net = mod._net(ctx.drop)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if labels is None:
            _lib.call("vg_gen_forward", C.byref(net), B, zin.data_ptr(), ws.data_ptr(), img.data_ptr(), st)
        else:
            _lib.call("vg_gen_forward_cond", C.byref(net), B, zin.data_ptr(), ws.data_ptr(), img.data_ptr(), C.byref(mod._cond(labels)), st)
        ctx.mod, ctx.ws, ctx.B, ctx.labels = mod, ws, B, labels
        return img.to(mod.out_dtype)

    @staticmethod
    def backward(ctx, dimg):
        mod = ctx.mod
        mod._flat.attach_grads()
        d = dimg.detach().to(torch.bfloat16).contiguous()
        net = mod._net(ctx.drop)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if ctx.labels is None:
            _lib.call("vg_gen_backward", C.byref(net), ctx.B, ctx.ws.data_ptr(), d.data_ptr(), st)
        else:
            _lib.call("vg_gen_backward_cond", C.byref(net), ctx.B, ctx.ws.data_ptr(), d.data_ptr(), C.byref(mod._cond(ctx.labels)), st)
        ctx.ws = None
        return None, None, None, None, None


class _GenF32Fn(torch.autograd.Function):
    """The fp32 mode (``SirenGenerator.precision = "fp32"``): vg_gen_forward_f32 / vg_gen_backward_f32 on the fp32 master parameters;
    the gradients land in the same flat gradient buffer, the image comes back in fp32."""

    @staticmethod
    def forward(ctx, mod: "SirenGenerator", z, anchor, drop_p, labels=None):
        ctx.drop = (float(drop_p), int(torch.randint(0, 2 ** 62, (1,)).item()) if drop_p > 0 else 0)
        B = z.shape[0]
        zin = z.detach().float().contiguous()
        ws = torch.empty(mod._ws_bytes_f32(B), dtype=torch.uint8, device=z.device)
        img = torch.empty(B, mod.channels, mod.image_size, mod.image_size, dtype=torch.float32, device=z.device)
        net = mod._net(ctx.drop)
        cond = None if labels is None else C.byref(mod._cond_f32(labels))
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.call("vg_gen_forward_f32", C.byref(net), B, zin.data_ptr(), ws.data_ptr(), img.data_ptr(), cond, st)
        ctx.mod, ctx.ws, ctx.B, ctx.labels = mod, ws, B, labels
        return img

    @staticmethod
    def backward(ctx, dimg):
        mod = ctx.mod
        mod._flat.attach_grads()
        d = dimg.detach().float().contiguous()
        net = mod._net(ctx.drop)
        cond = None if ctx.labels is None else C.byref(mod._cond_f32(ctx.labels))
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.call("vg_gen_backward_f32", C.byref(net), ctx.B, ctx.ws.data_ptr(), d.data_ptr(), cond, st)
        ctx.ws = None
        return None, None, None, None, None


PRECISIONS = ("bf16", "fp32")


def fourier_position_table(T: int, E: int, image_size: int, patch_size: int) -> torch.Tensor:
    """[T, E] fp32: token t at (x, y) in [0,1)^2 (patch-grid cell centre, or (0.5, row centre) for the v1 row tokens);
    column 4*j + c = (sin, cos)(2 pi f_j x), (sin, cos)(2 pi f_j y), E/4 log-spaced frequencies from 1 to side/2."""
    side = image_size // patch_size if patch_size else T
    t = torch.arange(T, dtype=torch.float64)
    if patch_size:
        x, y = ((t % side) + 0.5) / side, (torch.div(t, side, rounding_mode="floor") + 0.5) / side
    else:
        x, y = torch.full((T,), 0.5, dtype=torch.float64), (t + 0.5) / side
    nb = E // 4
    f = torch.pow(torch.tensor(max(side / 2.0, 1.0), dtype=torch.float64), torch.arange(nb, dtype=torch.float64) / max(nb - 1, 1))
    ax, ay = 2 * math.pi * x[:, None] * f[None, :], 2 * math.pi * y[:, None] * f[None, :]
    return torch.stack([torch.sin(ax), torch.cos(ax), torch.sin(ay), torch.cos(ay)], dim=-1).reshape(T, E).float().contiguous()


class SirenGenerator(nn.Module):
    def __init__(self, latent=1024, image_size=32, channels=3, embed=384, heads=4, layers=4, siren_hidden=768,
                 omega_0=30.0, out_dtype=torch.float32, dropout=0.2, patch_size=0, fourier_features=False, n_classes=0):
        """``patch_size == 0`` (default): the reference's v1 generator - one token per image row, each emitting
        ``channels * image_size`` values, assembled by a flat ``view`` (src/v1/generator.py:19,25,51,66-68).
        ``patch_size > 0`` (not in the reference): the same blocks on the discriminator's patch
        grid - ``(image_size / patch_size)**2`` tokens, each emitting one ``channels x P x P`` patch in conv1's
        (c, py, px) order, assembled by the un-patchify scatter.  Scales to 64x64 / 128x128 images (64 tokens).
        ``n_classes = K > 0`` (the reference has none): class-modulated self-modulation, w = mapping(z) + class_embedding[y] with a
        learned table ``class_embedding.weight`` [K, T*E] - the classic cGAN input Linear([z ; onehot(y)]), its K one-hot columns
        evaluated as a gather (vg_class_add / vg_class_grad).  ``forward(z, labels)`` then needs the labels, an integer tensor [B]
        on the device with values in [0, K).  The table lives behind the C layout in the same flat buffer, so whatever runs over
        the buffer (AdamW, the average, clipping, the checkpoint) covers it.  0: the state_dict is the reference's."""
        super().__init__()
        if isinstance(n_classes, bool) or not isinstance(n_classes, int) or not 0 <= n_classes <= 16:
            raise ValueError(f"n_classes must be an integer in [0, 16] (0 = unconditional), got {n_classes!r}")
        self.n_classes = n_classes
        E, hd = embed, embed // heads
        if patch_size:
            if image_size % patch_size:
                raise ValueError("image_size must be a multiple of patch_size")
            T, out_features = (image_size // patch_size) ** 2, channels * patch_size * patch_size
        else:
            T, out_features = image_size, channels * image_size
        self.patch_size = int(patch_size)
        # optional Fourier positional input of the SIREN (north_star; not in the reference): a fixed [T, E] table added to
        # the final SLN output.  A non-persistent buffer: the state_dict stays the reference's.
        self.register_buffer("fourier_table", fourier_position_table(T, E, image_size, self.patch_size) if fourier_features else None,
                             persistent=False)
        self.latent, self.image_size, self.channels, self.out_dtype = latent, image_size, channels, out_dtype
        self.dropout_p = float(dropout)  # attention_dropout_rate = mlp_dropout = 0.2 in src/v1/config.py:36,39
        self.mapping_mlp = _mlp_holder(T * E, latent)
        self.embedding = nn.Parameter(torch.randn(T, E))
        blocks = []
        for _ in range(layers):
            b = _Holder()
            b.layer_norm_1 = _sln_holder(E)
            b.layer_norm_2 = _sln_holder(E)
            b.msha = _Holder()
            heads_l = []
            for _h in range(heads):
                a = _Holder()
                a.q, a.k, a.v = (_linear_holder(hd, E, bias=False) for _ in range(3))
                heads_l.append(a)
            b.msha.attention_heads = nn.ModuleList(heads_l)
            b.msha.output_linear = _linear_holder(E, E)
            b.mlp = _mlp_holder(E, E)
            blocks.append(b)
        self.transformer_layers = nn.ModuleList(blocks)
        self.sln = _sln_holder(E)
        s0, s1 = _Holder(), _Holder()
        s0.linear = _linear_holder(siren_hidden, E)
        s1.linear = _linear_holder(out_features, siren_hidden)
        self.output_network = nn.Sequential(s0, s1)
        self._dims = _lib.VgGenDims(latent, T, E, heads, layers, siren_hidden, out_features, float(omega_0),
                                    self.patch_size, channels, image_size)
        slots, total = flat.gen_slots(self._dims), flat.gen_layout(self._dims).total
        self._class_off = None
        if n_classes:  # registered last: the other parameters keep their names, order and init draws
            self.class_embedding = _Holder()
            self.class_embedding.weight = nn.Parameter(torch.empty(n_classes, T * E))
            self._class_off, total = flat.gen_class_table(self._dims, n_classes)
            slots[flat.CLASS_TABLE_KEY] = (self._class_off, (n_classes, T * E))
        self.reset_parameters()
        self._flat = FlatParams(dict(self.named_parameters()), slots, total)
        # "bf16" (default): the fused engine above.  "fp32": fp32 activations, gradients and GEMM operands on the exact f32-input MFMA
        # with the accurate sine - the reference's own arithmetic, for checking the generator against the fp32 model or sampling a
        # reference checkpoint.  Not a constructor argument: set ``generator.precision = "fp32"``.  GanEngine stays bf16 and refuses it.
        self._precision = "bf16"

    @property
    def precision(self) -> str:
        return self._precision

    @precision.setter
    def precision(self, value: str) -> None:
        if not isinstance(value, str) or value not in PRECISIONS:
            raise ValueError(f"precision must be one of {PRECISIONS}, got {value!r}")
        if value == "fp32" and _lib.lib().vg_gen_ws_bytes_f32(C.byref(self._dims), 1) <= 0:
            d = self._dims
            raise ValueError(f"precision='fp32' takes at most 80 tokens, head widths 32 / 64 / 96 and an embedding of at most 1024; this "
                             f"generator has {d.T} tokens, head width {d.E // d.H}, embedding {d.E}")
        self._precision = value

    def reset_parameters(self):
        """Init distributions of the reference: nn.Linear default U(+-1/sqrt(in)); SIREN U(+-1/in) for
        the first layer and U(+-sqrt(6/in)/omega0) after (src/v1/siren.py:29-42); embedding, gamma,
        beta ~ N(0,1) (generator.py:24-26, spectral_layer_norm.py:16-17)."""
        w0 = float(self._dims.omega0)
        with torch.no_grad():
            for name, p in self.named_parameters():
                if name == "embedding" or name.endswith((".beta", ".gamma")):
                    p.normal_()
                elif name == flat.CLASS_TABLE_KEY:  # the K extra input columns of the mapping Linear it stands for: fan-in = latent
                    b = 1.0 / math.sqrt(self.latent)
                    p.uniform_(-b, b)
                elif "layer_norm.weight" in name:
                    p.fill_(1.0)
                elif "layer_norm.bias" in name:
                    p.zero_()
                elif name == "output_network.0.linear.weight":
                    p.uniform_(-1.0 / p.shape[1], 1.0 / p.shape[1])
                elif name == "output_network.1.linear.weight":
                    b = math.sqrt(6.0 / p.shape[1]) / w0
                    p.uniform_(-b, b)
                elif name.endswith("weight"):
                    b = 1.0 / math.sqrt(p.shape[1])
                    p.uniform_(-b, b)
                else:  # Linear bias: bound from the fan-in of its weight
                    fan_in = dict(self.named_parameters())[name[:-4] + "weight"].shape[1]
                    b = 1.0 / math.sqrt(fan_in)
                    p.uniform_(-b, b)

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        if hasattr(self, "_flat"):
            self._flat.named = dict(self.named_parameters())
            self._flat.rebuild()
        return out

    def zero_grad(self, set_to_none: bool = True):
        self._flat.zero_grad()

    def _ws_bytes(self, B):
        n = _lib.lib().vg_gen_ws_bytes(C.byref(self._dims), B)
        if n <= 0:
            raise RuntimeError("vg_gen_ws_bytes failed")
        return n

    def _ws_bytes_f32(self, B):
        n = _lib.lib().vg_gen_ws_bytes_f32(C.byref(self._dims), B)
        if n <= 0:
            raise RuntimeError("vg_gen_ws_bytes_f32 failed")
        return n

    def _cond_f32(self, labels) -> "_lib.VgGenCondF32":
        """the class-conditioning argument of the fp32 calls: the labels, and the table's fp32 master and fp32 gradient"""
        fp, off = self._flat, self._class_off
        return _lib.VgGenCondF32(labels.data_ptr(), fp.flat.data_ptr() + 4 * off, fp.grad.data_ptr() + 4 * off, self.n_classes)

    def _net(self, drop=(0.0, 0)):
        fp = self._flat
        tab = self.fourier_table
        return _lib.VgGenNet(self._dims, fp.flat.data_ptr(), fp.shadow.data_ptr(), fp.grad.data_ptr(), float(drop[0]), int(drop[1]), None,
                             None if tab is None else tab.data_ptr())

    def _cond(self, labels) -> "_lib.VgGenCond":
        """the class-conditioning argument of the _cond C calls: the labels, and the table's bf16 shadow and fp32 gradient"""
        fp, off = self._flat, self._class_off
        return _lib.VgGenCond(labels.data_ptr(), fp.shadow.data_ptr() + 2 * off, fp.grad.data_ptr() + 4 * off, self.n_classes)

    def _labels(self, labels, B: int, device):
        """``labels`` checked against this generator (required iff it is class-conditional) as the int32 tensor the kernels read"""
        if (labels is not None) != bool(self.n_classes):
            raise ValueError(f"labels are required exactly for a class-conditional generator (n_classes={self.n_classes})")
        if labels is None:
            return None
        from . import ops
        return ops.check_labels(labels, B, self.n_classes, "SirenGenerator", device)

    def forward(self, z, labels=None):
        if not z.is_cuda:
            raise RuntimeError("SirenGenerator.forward: the HIP engine needs cuda tensors; there is no CPU fallback")
        if not self._flat.aliased():
            self._flat.named = dict(self.named_parameters())
            self._flat.rebuild()
        fn = _GenF32Fn if self._precision == "fp32" else _GenFn
        return fn.apply(self, z, self.embedding, self.dropout_p if self.training else 0.0, self._labels(labels, z.shape[0], z.device))
