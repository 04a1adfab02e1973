"""tests/engine_util.py on the CPU: the run comparison, the data stream, the process launcher (children that never touch the GPU side
of torch), and the step oracle with every hook off against the plain step written out from its pieces."""
import time

import pytest
import torch

import engine_util as eu


# ------------------------------------------------------------------------------------------------------------ assert_same_run
def _run(n=3, n_state=4, extras=("a", "b")):
    g = torch.Generator().manual_seed(1)
    return eu.Run(torch.randn(n, 3, generator=g), [torch.randn(5 + i, generator=g) for i in range(n_state)],
                  {k: [torch.randn(2, generator=g) for _ in range(n)] for k in extras})


def _clone(r):
    return eu.Run(r.losses.clone(), [t.clone() for t in r.state], {k: [t.clone() for t in v] for k, v in r.extras.items()})


def _flip(t, i=0):
    t.view(torch.int32).reshape(-1)[i] ^= 1  # one bit of one element


def test_assert_same_run_passes_on_clones():
    a = _run()
    eu.assert_same_run(a, _clone(a), "clones")


def test_assert_same_run_sees_one_bit_of_one_loss():
    a, b = _run(), _clone(_run())
    _flip(b.losses, 4)
    with pytest.raises(AssertionError):
        eu.assert_same_run(a, b, "loss bit")


@pytest.mark.parametrize("which", range(4))
def test_assert_same_run_sees_one_element_of_any_state_tensor(which):
    a, b = _run(), _clone(_run())
    _flip(b.state[which], which)
    with pytest.raises(AssertionError, match=f"state tensor {which}"):
        eu.assert_same_run(a, b, "state")


@pytest.mark.parametrize("name", ["a", "b"])
def test_assert_same_run_sees_any_extra(name):
    a, b = _run(), _clone(_run())
    _flip(b.extras[name][2])
    with pytest.raises(AssertionError, match=f"{name} of step 3"):
        eu.assert_same_run(a, b, "extra")


def test_assert_same_run_sees_what_is_missing_from_either_side():
    a = _run()
    short_state = eu.Run(a.losses, a.state[:-1], a.extras)
    short_steps = eu.Run(a.losses[:-1], a.state, {k: v[:-1] for k, v in a.extras.items()})
    short_extra = eu.Run(a.losses, a.state, {k: (v[:-1] if k == "b" else v) for k, v in a.extras.items()})
    no_extra = eu.Run(a.losses, a.state, {"a": a.extras["a"]})
    for other in (short_state, short_steps, short_extra, no_extra):
        for x, y in ((a, other), (other, a)):
            with pytest.raises(AssertionError):
                eu.assert_same_run(x, y, "missing")


def test_join_runs_is_the_continued_run():
    a = _run(4)
    head = eu.Run(a.losses[:1], [t + 1 for t in a.state], {k: v[:1] for k, v in a.extras.items()})
    tail = eu.Run(a.losses[1:], a.state, {k: v[1:] for k, v in a.extras.items()})
    eu.assert_same_run(eu.join_runs(head, tail), a, "joined")


# ---------------------------------------------------------------------------------------------------------------- the stream
def test_batches_are_the_tensors_drawn_inline():
    B = 4
    g = torch.Generator().manual_seed(4)
    want = []
    for _ in range(2):
        real = torch.rand(B, 3, 32, 32, generator=g) * 2 - 1
        want.append((real, torch.randn(B, 1024, generator=g)))
    got = eu.batches(B, 2, device="cpu")
    assert len(got) == 2 and all(len(b) == 2 for b in got)
    for (r, z), (wr, wz) in zip(got, want):
        assert torch.equal(r, wr) and torch.equal(z, wz)


def test_batches_skip_drops_the_first_k():
    whole = eu.batches(4, 5, device="cpu")
    for k in (1, 3):
        tail = eu.batches(4, 5 - k, skip=k, device="cpu")
        assert len(tail) == 5 - k and all(torch.equal(x, y) for a, b in zip(tail, whole[k:]) for x, y in zip(a, b))


def test_batches_of_the_conditional_geometry():
    g = torch.Generator().manual_seed(4)
    real = torch.rand(8, 3, 16, 16, generator=g) * 2 - 1
    y = torch.randint(0, 3, (8,), generator=g)
    (r, lab), = eu.batches(8, 1, image=16, latent=0, labels=3, device="cpu")
    assert torch.equal(r, real) and torch.equal(lab, y)


# -------------------------------------------------------------------------------------------------------------- the launcher
def _answer(rank, world, base):
    return base + rank, world


def _raise_on_one(rank, world):
    if rank == 1:
        raise ValueError("rank one says no")
    return rank


def _sleep(rank, world, seconds):
    time.sleep(seconds)
    return rank


def _sum_over_ranks(rank, world):
    import torch.distributed as dist
    t = torch.tensor([float(rank + 1)])
    dist.all_reduce(t)
    return float(t)


def test_run_ranks_returns_every_rank_result_in_order():
    assert eu.run_ranks(_answer, 2, 60, 10, backend=None) == [(10, 2), (11, 2)]


def test_run_ranks_joins_a_gloo_group():
    assert eu.run_ranks(_sum_over_ranks, 2, 60) == [3.0, 3.0]


def test_run_ranks_fails_with_the_childs_exception_text():
    with pytest.raises(AssertionError, match="rank 1: ValueError: rank one says no"):
        eu.run_ranks(_raise_on_one, 2, 60, backend=None)


def test_run_ranks_kills_a_child_that_outlives_the_limit():
    t0 = time.monotonic()
    with pytest.raises(AssertionError, match="no result from rank"):  # a CPU child: the session goes on
        eu.run_ranks(_sleep, 1, 1.0, 600.0, backend=None, grace=1.0)
    assert time.monotonic() - t0 < 30
    (child,) = eu.run_ranks.children
    assert not child.is_alive() and child.exitcode not in (0, None)


# --------------------------------------------------------------------------------------------------------------- the oracle
def _plain_step(o, real, z, gp_epsilon):
    """the alternating step of oracle/step_oracle.py's header, from the oracle's pieces, with no hook anywhere"""
    from oracle import step_oracle as so
    from oracle.vit_oracle import vit_forward
    for p in o.d.values():
        p.grad = None
    loss_real = so.d_loss_real(o.D(real), o.loss)
    loss_real.backward()
    fake = o.G(z)
    loss_fake = so.d_loss_fake(o.D(fake.detach()), o.loss)
    loss_fake.backward()
    if o.gp_weight:
        (o.gp_weight * so.gradient_penalty(lambda t: vit_forward(o.d, t, o.ddims), real, fake.detach(), gp_epsilon)).backward()
    if o.clip_d is not None:
        torch.nn.utils.clip_grad_norm_(list(o.d.values()), max_norm=o.clip_d)
    o.opt_d.step()
    for p in o.g.values():
        p.grad = None
    loss_g = so.g_loss(o.D(fake), o.loss)
    (loss_g + o.diversity_weight * so.diversity_loss(fake) if o.diversity_weight else loss_g).backward()
    if o.clip_g is not None:
        torch.nn.utils.clip_grad_norm_(list(o.g.values()), max_norm=o.clip_g)
    o.opt_g.step()
    return {"d_real": float(loss_real.detach()), "d_fake": float(loss_fake.detach()), "g": float(loss_g.detach())}


@pytest.mark.parametrize("extras", [False, True], ids=["plain", "gp_clip_diversity"])
@pytest.mark.parametrize("loss", ["ns", "hinge", "wasserstein"])
def test_step_with_every_hook_off_is_the_plain_step(loss, extras):
    from oracle import gen_oracle as go, step_oracle as so, vit_oracle as vo
    dd, gd = vo.VitDims(layers=1, classes=1), go.GenDims(layers=1)
    ds, gs = vo.init_vit_state(dd, 0), go.init_gen_state(gd, 1)
    oracles = [so.GanStepOracle(ds, gs, dd, gd, loss=loss) for _ in range(3)]
    if extras:
        for o in oracles:
            o.gp_weight, o.clip_d, o.clip_g, o.diversity_weight = 10.0, 0.05, 0.02, 0.1
    plain, default, identity = oracles
    hooks = so.StepHooks(d_inputs=lambda r, f: (r, f), g_input=lambda f: f)
    g = torch.Generator().manual_seed(0)
    for it in range(2):
        real, z, eps = torch.rand(2, 3, 32, 32, generator=g) * 2 - 1, torch.randn(2, 1024, generator=g), torch.rand(2, 1, 1, 1, generator=g)
        want = _plain_step(plain, real, z, eps)
        assert default.step(real, z, gp_epsilon=eps) == want and identity.step(real, z, gp_epsilon=eps, hooks=hooks) == want, it
        for o in (default, identity):
            assert all(torch.equal(o.d[k], plain.d[k]) for k in plain.d) and all(torch.equal(o.g[k], plain.g[k]) for k in plain.g), it
    assert not torch.equal(plain.d["vit.encoder.0.fc2.weight"], ds["vit.encoder.0.fc2.weight"])
