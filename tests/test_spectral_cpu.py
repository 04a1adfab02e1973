"""Spectral normalisation without a GPU: the float64 restatement of tests/spectral_ref.py against torch's SVD and autograd, the bounds
of check_update / check_project against a float32 emulation of the kernels' arithmetic (and against four planted mistakes), the new
entry points' exports and argument codes, and the Python surface's argument errors."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import vit_gan_amd  # noqa: F401
import spectral_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vg_spectral_plan", "vg_spectral_update", "vg_spectral_project")


@pytest.mark.parametrize("scale", ["init", "trained"])
def test_the_iteration_reaches_the_largest_singular_value(scale):
    """sigma of the restatement's iteration never exceeds sigma_max (it is |W v| of a unit v), never decreases, and from a random u
    reaches svdvals(W)[0]: to 1e-9 where the spectrum has a gap (trained-like), to 2e-3 in 300 iterations on a random matrix at
    vit_init_weights' scale, whose top singular values lie within a fraction of a percent of each other.  [1, E]: sigma = |W|_2 at once."""
    worst = 0.0
    for N, K in sr.SHAPES:
        W = sr.make_matrix(N, K, scale)
        smax = float(torch.linalg.svdvals(W.double())[0])
        u = torch.randn(N, generator=torch.Generator().manual_seed(N + K), dtype=torch.float64)
        u /= u.norm()
        last = 0.0
        for it in range(300):
            v, sigma, u = sr.power_step(W, u)
            assert sigma <= smax * (1 + 1e-12) and sigma >= last * (1 - 1e-12), (N, K, it, sigma, last, smax)
            if N == 1:
                assert abs(sigma - float(W.double().norm())) <= 1e-14 * smax
            done = sigma - last <= 1e-15 * sigma
            last = sigma
            if done:
                break
        gap = 1 - last / smax
        worst = max(worst, gap)
        assert gap <= (1e-9 if scale == "trained" or N == 1 else 2e-3), (N, K, gap)
    print(f"\n{scale}: worst 1 - sigma / sigma_max after <= 300 iterations {worst:.3e}")


@pytest.mark.parametrize("N,K", [(1, 384), (10, 384), (384, 48), (128, 256), (384, 384)])
def test_the_gradient_formula_is_autograd_of_the_normalised_weight(N, K):
    g = torch.Generator().manual_seed(N * 3 + K)
    W = sr.make_matrix(N, K, "trained").double().requires_grad_(True)
    u = torch.randn(N, generator=g, dtype=torch.float64)
    v, sigma, u1 = sr.power_step(W.detach(), u / u.norm())
    sigma0 = 1.7 * sigma
    A = torch.randn(N, K, generator=g, dtype=torch.float64)  # L = <A, W_eff>: dL/dW_eff = A
    ((sigma0 * W / (u1 @ W @ v)) * A).sum().backward()
    # sigma = u1^T W v holds exactly for the pair of one iteration (u1 = W v / |W v|)
    want = sr.project(A, W.detach(), u1, v, sigma, sigma0)
    err = float((W.grad - want).abs().max())
    assert err <= 1e-12 * float(want.abs().max()), err


def _cases():
    for N, K in sr.SHAPES:
        for scale in ("init", "trained"):
            yield N, K, scale


def test_float32_form_stays_inside_the_bounds_at_every_shape():
    worst = {}
    for N, K, scale in _cases():
        W = sr.make_matrix(N, K, scale)
        g = torch.Generator().manual_seed(N + 2 * K)
        uc, s0, _ = sr.top_pair(W)
        for start, u in (("converged", uc.float()), ("random", torch.nn.functional.normalize(torch.randn(N, generator=g), dim=0))):
            sigma0 = 1.25 * s0
            v, sigma, un, shadow = sr.emulate_update(W, u, sigma0)
            fr = sr.check_update(W, u, sigma0, v, sigma, un, shadow.float(), f"{N}x{K} {scale} {start}")
            G = torch.randn(N, K, generator=g) * 1e-3 + 0.05 * W
            out = sr.emulate_project(G, W, un, v, sigma, sigma0)
            fr["proj"] = sr.check_project(G, W, un, v, sigma, sigma0, out, f"{N}x{K} {scale} {start}")
            for k, f in fr.items():
                worst[k] = max(worst.get(k, 0.0), f)
    print("\nfloat32 form, worst fraction of each bound:", {k: round(v, 3) for k, v in worst.items()})
    assert all(f <= 1.0 for f in worst.values())


def _setup(N=384, K=384):
    W = sr.make_matrix(N, K, "trained")
    g = torch.Generator().manual_seed(5)
    u = torch.nn.functional.normalize(torch.randn(N, generator=g), dim=0)
    G = torch.randn(N, K, generator=g) * 1e-3 + 0.05 * W
    return W, u, G, 1.3 * sr.top_pair(W)[1]


def test_planted_w_for_w_transpose_leaves_the_bound():
    W, u, G, s0 = _setup()
    v, sigma, un, sh = sr.emulate_update(W, u, s0, transpose_bug=True)
    with pytest.raises(AssertionError, match="v off"):
        sr.check_update(W, u, s0, v, sigma, un, sh.float())


def test_planted_inverse_scale_leaves_the_bound():
    W, u, G, s0 = _setup()
    v, sigma, un, sh = sr.emulate_update(W, u, s0, inverse_scale_bug=True)
    with pytest.raises(AssertionError, match="shadow off"):
        sr.check_update(W, u, s0, v, sigma, un, sh.float())


def test_planted_projection_without_its_sigma_leaves_the_bound():
    W, u, G, s0 = _setup()
    v, sigma, un, _ = sr.emulate_update(W, u, s0)
    assert abs(sigma - 1.0) > 0.5
    with pytest.raises(AssertionError, match="projected gradient off"):
        sr.check_project(G, W, un, v, sigma, s0, sr.emulate_project(G, W, un, v, sigma, s0, no_sigma_bug=True))
    sr.check_project(G, W, un, v, sigma, s0, sr.emulate_project(G, W, un, v, sigma, s0))


def test_planted_projection_with_the_post_update_state_leaves_the_bound():
    """The passes of a step read the shadow made from (u, v, sigma) BEFORE that step's update; projecting with the state after it is
    a different map as long as the iteration still moves."""
    W, u, G, s0 = _setup()
    v1, sigma1, u1, _ = sr.emulate_update(W, u, s0)             # produced the shadow the step's passes read
    W2 = (W + 0.02 * torch.randn(W.shape, generator=torch.Generator().manual_seed(9))).float()
    v2, sigma2, u2, _ = sr.emulate_update(W2, u1, s0)           # the update after AdamW
    wrong = sr.emulate_project(G, W, u2, v2, sigma2, s0)
    with pytest.raises(AssertionError, match="projected gradient off"):
        sr.check_project(G, W, u1, v1, sigma1, s0, wrong)


# ------------------------------------------------------------------------------------------ ABI hygiene
def test_header_declares_and_library_exports_the_new_symbols():
    from vit_gan_amd import _lib
    header = open(os.path.join(ROOT, "include", "vitgan_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib._SIGNATURES
    assert "VgSpectralDesc" in header
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    if out.returncode == 0:
        exported = set(re.findall(r"\bT (\w+)", out.stdout))
        assert set(NEW_SYMBOLS) <= exported
    assert lib.vg_abi_version() == _lib.ABI_VERSION == 9  # additive exports: the ABI number stays


def _table(entries):
    from vit_gan_amd import _lib
    tab = (_lib.VgSpectralDesc * len(entries))()
    for d, (off, N, K) in zip(tab, entries):
        d.w_off, d.N, d.K = off, N, K
    return tab


def test_entry_points_validate_their_arguments_without_a_device():
    from vit_gan_amd import _lib
    lib = _lib.lib()
    p16 = C.c_void_p(4096)  # never dereferenced: validation fails first
    ns, nc = C.c_longlong(), C.c_longlong()
    good = _table([(0, 384, 384), (384 * 384, 1, 384), (384 * 385, 384, 48)])
    total = 384 * 385 + 384 * 48
    pt = lambda t: C.cast(t, C.c_void_p)  # noqa: E731
    assert lib.vg_spectral_plan(None, 3, C.byref(ns), C.byref(nc)) == -1
    assert lib.vg_spectral_plan(pt(good), 0, C.byref(ns), C.byref(nc)) == -1
    for bad in ((0, 0, 384), (0, 384, 0), (0, -1, 4)):
        assert lib.vg_spectral_plan(pt(_table([bad])), 1, C.byref(ns), C.byref(nc)) == -2, bad
    assert lib.vg_spectral_plan(pt(good), 3, C.byref(ns), C.byref(nc)) == 0
    S, Q = ns.value, nc.value
    assert S == 384 + 384 + 4 + 4 + 384 + 4 + 384 + 48 + 4 and all(getattr(d, f) % 4 == 0 for d in good for f in ("u_off", "v_off", "s_off", "t_off"))

    def upd(W=p16, sh=p16, tot=total, st=p16, S_=S, sc=p16, Q_=Q, th=good, td=p16, n=3, it=1):
        return lib.vg_spectral_update(W, sh, tot, st, S_, sc, Q_, None if th is None else pt(th), td, n, it, None)

    def prj(G=p16, W=p16, tot=total, st=p16, S_=S, sc=p16, Q_=Q, th=good, td=p16, n=3):
        return lib.vg_spectral_project(G, W, tot, st, S_, sc, Q_, None if th is None else pt(th), td, n, None)

    for name in ("W", "sh", "st", "sc", "th", "td"):
        assert upd(**{name: None}) == -1, name
    for name in ("G", "W", "st", "sc", "th", "td"):
        assert prj(**{name: None}) == -1, name
    assert upd(n=0) == -1 and prj(n=0) == -1                      # an empty table
    assert upd(it=2) == -4 and upd(it=-1) == -4
    assert upd(tot=total - 1) == -2 and prj(tot=total - 1) == -2  # a range outside the buffer
    assert upd(S_=S - 1) == -2 and prj(Q_=Q - 1) == -2            # state / scratch smaller than the plan's
    raw = _table([(0, 384, 384), (384 * 384, 1, 384), (384 * 385, 384, 48)])
    assert upd(th=raw) == -2                                      # a table that was never planned
    for entries in ([(0, 384, 384), (100, 1, 384)], [(0, 64, 64), (4095, 4, 4)], [(512, 8, 8), (0, 64, 9)]):
        t = _table(entries)
        assert lib.vg_spectral_plan(pt(t), 2, C.byref(ns), C.byref(nc)) == 0
        assert upd(th=t, n=2, tot=1 << 20, S_=ns.value, Q_=nc.value) == -3, entries   # overlapping ranges
        assert prj(th=t, n=2, tot=1 << 20, S_=ns.value, Q_=nc.value) == -3, entries
    zero = _table([(0, 0, 4)])
    assert upd(th=zero, n=1) == -2 and prj(th=zero, n=1) == -2
    assert upd(W=C.c_void_p(4100)) == -3 and prj(G=C.c_void_p(4100)) == -3            # not 16-byte aligned


def test_engine_and_trainer_refuse_a_bad_set_name_without_a_device():
    from vit_gan_amd.config import Config
    from vit_gan_amd.engine import GanEngine
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.modules import ViTDiscriminator
    from vit_gan_amd.spectral import vit_matrix_keys
    from vit_gan_amd.training import train_model
    D = ViTDiscriminator(Config(embeddings_dimension=384, classes_count=1, transformer_blocks_count=1))
    G = SirenGenerator(layers=1)
    for bad in ("bogus", "QKV", "qkv,all", 3):
        with pytest.raises(ValueError, match=r"'qkv' / 'all'"):
            GanEngine(D, G, batch=4, spectral_norm=bad)
        with pytest.raises(ValueError, match=r"'qkv' / 'all'"):
            train_model(spectral_norm=bad, save_artifacts=False)
    with pytest.raises(ValueError, match="two_stream"):
        GanEngine(D, G, batch=4, spectral_norm="all", two_stream=True)
    for good in ("", "qkv", "all"):  # good names get as far as the device check (CPU modules: no CPU fallback)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            GanEngine(D, G, batch=4, spectral_norm=good)
    sd = D.vit.state_dict()
    assert vit_matrix_keys(2, "") == [] and len(vit_matrix_keys(2, "qkv")) == 6 and len(vit_matrix_keys(2, "all")) == 14
    assert all(k in sd for k in vit_matrix_keys(1, "all"))
    # every matrix of the set starts on a multiple of 4 elements of the flat buffer (the 16-byte path), conv and classifier included
    for E, kc in ((384, 1), (384, 10), (128, 1)):
        Dv = ViTDiscriminator(Config(embeddings_dimension=E, classes_count=kc, transformer_blocks_count=2)).vit
        for k in vit_matrix_keys(2, "all"):
            assert Dv._flat.slots[k][0] % 4 == 0, (E, k)
