"""Spectral normalisation of weight matrices inside a flat parameter buffer (csrc/spectral.hip, vg_spectral_*).

``W_eff = sigma0 * W / sigma`` with ``sigma0 = sigma_max`` of the weights the state was measured on and ``sigma`` one power
iteration per step behind ``sigma_max(W)``: the GEMMs read only the bf16 shadow, so the normalised network is a scaled cast of the
fp32 master (``update``) and the optimizer sees the raw-weight gradient after one rank-one correction (``project``).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence, Tuple

import torch

from . import _lib

SETS = ("qkv", "all")
EPS = 1e-12


def parse_spectral_set(name) -> str:
    """"" (nothing), "qkv" or "all"; anything else is a ValueError that names the two sets."""
    if name is None or name == "":
        return ""
    if name not in SETS:
        raise ValueError(f"spectral_norm must be '' or one of the sets {' / '.join(repr(s) for s in SETS)}, got {name!r}")
    return name


def vit_matrix_keys(n_layers: int, which: str) -> List[str]:
    """state_dict keys (without prefix) of the normalised set.  "qkv": queries / keys / values of every block, each [E, E] matrix on
    its own (the reference's v1 set).  "all" adds out_projection, fc1, fc2, classifier.fc1 and embedding.conv1 as [E, C P P].
    classifier.fc2 is NOT in the set: the head kernels read that [Kc, E] matrix from the fp32 master, not from the shadow, so a
    scaled cast cannot reach it."""
    which = parse_spectral_set(which)
    if not which:
        return []
    keys = []
    if which == "all":
        keys.append("embedding.conv1.weight")
    for i in range(n_layers):
        b = f"encoder.{i}."
        keys += [b + f"attention.{nm}.weight" for nm in ("queries", "keys", "values")]
        if which == "all":
            keys += [b + "attention.out_projection.weight", b + "fc1.weight", b + "fc2.weight"]
    if which == "all":
        keys.append("classifier.fc1.weight")
    return keys


class SpectralState:
    """The table, ``u / v / sigma / sigma0`` and the two calls for ``entries`` = [(element offset, N, K)] of a flat buffer of
    ``total`` elements.  The entries are kept in ascending offset order."""

    def __init__(self, entries: Sequence[Tuple[int, int, int]], total: int, device, names: Sequence[str] = ()):
        order = sorted(range(len(entries)), key=lambda i: entries[i][0])
        self.entries = [tuple(int(x) for x in entries[i]) for i in order]
        self.names = [names[i] for i in order] if names else [f"m{i}" for i in range(len(entries))]
        self.total, self.n = int(total), len(self.entries)
        self.table = (_lib.VgSpectralDesc * max(self.n, 1))()
        for d, (off, N, K) in zip(self.table, self.entries):
            d.w_off, d.N, d.K = off, N, K
        ns, nc = C.c_longlong(0), C.c_longlong(0)
        _lib.call("vg_spectral_plan", C.cast(self.table, C.c_void_p), self.n, C.byref(ns), C.byref(nc))
        self.state_floats, self.scratch_floats = int(ns.value), int(nc.value)
        self.device = torch.device(device)
        raw = torch.frombuffer(bytearray(bytes(self.table)), dtype=torch.uint8)
        self.table_dev = raw.to(self.device)
        self.state = torch.zeros(self.state_floats, dtype=torch.float32, device=self.device)
        self.scratch = torch.zeros(self.scratch_floats, dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------------ views of the state
    def u(self, i): d = self.table[i]; return self.state[d.u_off:d.u_off + d.N]            # noqa: E702
    def v(self, i): d = self.table[i]; return self.state[d.v_off:d.v_off + d.K]            # noqa: E702
    def sigma(self, i): d = self.table[i]; return self.state[d.s_off:d.s_off + 1]          # noqa: E702
    def sigma0(self, i): d = self.table[i]; return self.state[d.s_off + 1:d.s_off + 2]     # noqa: E702

    def scale(self, i) -> torch.Tensor:
        """fp32(sigma0 / max(sigma, 1e-12)): the kernel's own expression (IEEE division)."""
        return self.sigma0(i) / torch.clamp(self.sigma(i), min=EPS)

    def matrix(self, flat: torch.Tensor, i) -> torch.Tensor:
        off, N, K = self.entries[i]
        return flat[off:off + N * K].view(N, K)

    # ------------------------------------------------------------------ host: measure the state from the current weights
    @torch.no_grad()
    def measure(self, flat: torch.Tensor) -> None:
        """sigma0 = sigma = sigma_max(W), (u, v) the top singular pair, per matrix (float64 SVD on the host: a one-off).  The scale is
        then exactly 1, so the next shadow is the plain cast."""
        host = torch.zeros(self.state_floats, dtype=torch.float32)
        w = flat.detach().to("cpu", torch.float64)
        for i, (off, N, K) in enumerate(self.entries):
            U, S, Vh = torch.linalg.svd(w[off:off + N * K].view(N, K), full_matrices=False)
            d = self.table[i]
            host[d.u_off:d.u_off + N] = U[:, 0].float()
            host[d.v_off:d.v_off + K] = Vh[0].float()
            host[d.s_off] = host[d.s_off + 1] = S[0].float()
        self.state.copy_(host)

    # ------------------------------------------------------------------ the two calls (enqueue only)
    def update(self, flat: torch.Tensor, shadow: torch.Tensor, iterate: bool = True, stream=None) -> None:
        p = _lib.ptr
        _lib.call("vg_spectral_update", p(flat), p(shadow), self.total, p(self.state), self.state_floats, p(self.scratch), self.scratch_floats,
                  C.cast(self.table, C.c_void_p), p(self.table_dev), self.n, int(bool(iterate)), _lib.stream() if stream is None else stream)

    def project(self, grad: torch.Tensor, flat: torch.Tensor, stream=None) -> None:
        p = _lib.ptr
        _lib.call("vg_spectral_project", p(grad), p(flat), self.total, p(self.state), self.state_floats, p(self.scratch), self.scratch_floats,
                  C.cast(self.table, C.c_void_p), p(self.table_dev), self.n, _lib.stream() if stream is None else stream)

    @torch.no_grad()
    def effective(self, flat: torch.Tensor) -> torch.Tensor:
        """A copy of ``flat`` with fp32(s * W) in every normalised range: the kernel's expression, so its bf16 cast is the shadow."""
        out = flat.detach().clone()
        for i, (off, N, K) in enumerate(self.entries):
            out[off:off + N * K] = self.scale(i) * flat[off:off + N * K]
        return out
