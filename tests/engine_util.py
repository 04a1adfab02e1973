"""The one way the engine tests build, feed, run and compare a GanEngine, and the one way any test runs workers in processes of their own.

A plain helper module beside gpu_util.py.  Nothing here imports the GPU side of torch at module level: test_engine_util_cpu.py imports it
on a machine without one."""
import collections
import os
import sys

import pytest
import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
COND_G = dict(latent=256, image_size=16, channels=3, embed=384, heads=4, layers=2, siren_hidden=256)


# ------------------------------------------------------------------------------------------------------------------ networks
def state_of(module):
    return {k: v.detach().clone() for k, v in module.state_dict().items()}


def build_nets(B, seed, d_layers=2, g_layers=2, dropout=False, full=False, cond=None):
    """(D, G) on the CPU, D constructed before G straight after torch.manual_seed(seed) - the initial weights are a function of
    (seed, shapes) alone.  dropout: D 0.1 / G 0.2 (what bench.py trains with) or 0.0 / 0.0.
    full: the C2 shape bench.py measures (every Config / SirenGenerator default but E = 384 and one logit).
    cond = (n_classes, Kc): the conditional geometry - D with E = 128, H = 4, 16 x 16 images, patch 4, Kc logits; G two SLN blocks
    on 16 row tokens with an n_classes table."""
    import vit_gan_amd  # noqa: F401
    from vit_gan_amd.config import Config
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.modules import ViTDiscriminator
    p_d, p_g = (0.1, 0.2) if dropout else (0.0, 0.0)
    torch.manual_seed(seed)
    if full:
        return ViTDiscriminator(Config(embeddings_dimension=384, classes_count=1, batch_size=B)), SirenGenerator()
    if cond is not None:
        D = ViTDiscriminator(Config(embeddings_dimension=128, attention_heads_count=4, transformer_blocks_count=d_layers, image_size=16,
                                    patch_size=4, classes_count=cond[1], dropout_rate=p_d, batch_size=B))
        return D, SirenGenerator(dropout=p_g, n_classes=cond[0], **COND_G)
    D = ViTDiscriminator(Config(embeddings_dimension=384, classes_count=1, dropout_rate=p_d, batch_size=B, transformer_blocks_count=d_layers))
    return D, SirenGenerator(layers=g_layers, dropout=p_g)


def build(B, loss="ns", seed=3, layers=2, faithful=False):
    """(D, G, oracle): the dropout-free networks on the GPU and a GanStepOracle (fp32, or rounding-faithful) on their initial state"""
    from oracle import gen_oracle as go, step_oracle as so, vit_oracle as vo
    D, G = build_nets(B, seed, d_layers=layers)
    oracle = so.GanStepOracle(state_of(D), state_of(G), vo.VitDims(layers=layers, classes=1), go.GenDims(layers=2), loss=loss, faithful=faithful)
    return D.cuda(), G.cuda(), oracle


def train_engine(B, seed=5, d_layers=2, g_layers=2, full=False, **kw):
    """(engine, D, G, initial state): train-mode networks with dropout (D 0.1 / G 0.2) at a size the CPU model finishes in seconds,
    under a GanEngine with seed 77 and the options given"""
    from vit_gan_amd.engine import GanEngine
    D, G = build_nets(B, seed, d_layers, g_layers, dropout=True, full=full)
    D, G = D.train(), G.train()
    state = (state_of(D), state_of(G))
    opts = dict(batch=B, seed=77)
    opts.update(kw)
    return GanEngine(D.cuda(), G.cuda(), **opts), D, G, state


def bench_like(B, seed=5, d_layers=2, g_layers=2, **kw):
    """train_engine in the configuration bench.py measures - fused real+fake pass, single-stream weight gradients - with the noise
    coming from the caller (external_noise); d_dropout / g_dropout = 0.0 switch the fused dropout off"""
    opts = dict(external_noise=True, fuse_real_fake=True, concurrent_wgrad=False)  # bench.py's defaults
    opts.update(kw)
    return train_engine(B, seed, d_layers, g_layers, **opts)


# ---------------------------------------------------------------------------------------------------------------------- data
def batches(B, n, skip=0, seed=4, image=32, latent=1024, labels=0, device="cuda"):
    """Batches skip .. skip + n - 1 of the stream every engine test is fed: one generator seeded ``seed``; per step the real images
    rand * 2 - 1, then the latents randn (latent = 0: none, the engine draws its own), then ``labels``-way class labels (0: none)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(skip + n):
        batch = (torch.rand(B, 3, image, image, generator=g) * 2 - 1,)
        if latent:
            batch += (torch.randn(B, latent, generator=g),)
        if labels:
            batch += (torch.randint(0, labels, (B,), generator=g),)
        if i >= skip:
            out.append(tuple(t.to(device) for t in batch))
    return out


# ------------------------------------------------------------------------------------------------------------------- running
Run = collections.namedtuple("Run", "losses state extras")  # [n, 3] on the host; cloned _state_tensors(); {name: [per-step clone]}


def run_steps(eng, data, each=None, extras=(), step=None):
    """One engine step per batch of ``data``.  extras: attribute names, or (name, function of the engine) pairs, cloned after every
    step.  each(i): called after step i (0-based) with the device idle.  step(eng, batch): how a batch is handed over, eng.step(*batch)
    unless given."""
    extras = [(e, (lambda en, a=e: getattr(en, a))) if isinstance(e, str) else e for e in extras]
    losses, seen = [], {name: [] for name, _ in extras}
    for i, batch in enumerate(data):
        losses.append((eng.step(*batch) if step is None else step(eng, batch)).clone())
        for name, get in extras:
            seen[name].append(get(eng).detach().clone())
        if each is not None:
            torch.cuda.synchronize()
            each(i)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return Run(torch.stack(losses).cpu(), [t.detach().clone().cpu() for t in eng._state_tensors()],
               {name: [t.cpu() for t in ts] for name, ts in seen.items()})


def join_runs(first, second):
    """the run that is ``first`` continued by ``second``: all the losses and extras, the state after the last step"""
    assert set(first.extras) == set(second.extras)
    return Run(torch.cat([first.losses, second.losses]), second.state, {k: first.extras[k] + second.extras[k] for k in first.extras})


def assert_same_run(a, b, what):
    """bit equality of two runs: the losses, every state tensor, every extra of every step - and the same number of each"""
    assert a.losses.shape == b.losses.shape and torch.equal(a.losses, b.losses), (what, a.losses, b.losses)
    assert len(a.state) == len(b.state), f"{what}: {len(a.state)} state tensors against {len(b.state)}"
    for i, (x, y) in enumerate(zip(a.state, b.state)):
        assert torch.equal(x, y), f"{what}: state tensor {i} differs"
    assert set(a.extras) == set(b.extras), (what, sorted(a.extras), sorted(b.extras))
    for name, xs in a.extras.items():
        ys = b.extras[name]
        assert len(xs) == len(ys), f"{what}: {name} recorded for {len(xs)} steps against {len(ys)}"
        for i, (x, y) in enumerate(zip(xs, ys)):
            assert torch.equal(x, y), f"{what}: {name} of step {i + 1} differs"


def _engine_of(made):
    return made[0] if isinstance(made, tuple) else made


def graph_against_eager(make, data, what="graph replay", **run_kw):
    """make(use_graph=...) -> an engine, or a tuple that starts with one.  Runs ``data`` eagerly and as hipGraph replays; each engine must
    have run as asked (graph_active, no fallback reason, the device step counter), and the two runs must be bit-equal.
    Returns ({"eager": Run, "graph": Run}, {"eager": what make returned, "graph": ...}) for the caller's own assertions."""
    runs, made = {}, {}
    for name, use_graph in (("eager", False), ("graph", True)):
        made[name] = make(use_graph=use_graph)
        eng = _engine_of(made[name])
        runs[name] = run_steps(eng, data, **run_kw)
        assert eng.graph_active == use_graph and eng.graph_fallback_reason is None and int(eng.step_t) == len(data), \
            (name, eng.graph_active, eng.graph_fallback_reason, int(eng.step_t))
    assert_same_run(runs["graph"], runs["eager"], what)
    return runs, made


def resume_against_whole(make, data, n_first, **run_kw):
    """make(**kw) -> (engine, D, G, ...).  Runs all of ``data`` on one engine; runs the first n_first batches on a second, saves it,
    loads the networks and the engine state into a third built from other initial weights (make(seed=99)) and continues.  The
    interrupted run must equal the whole one bit for bit; the first two engines are closed once they have run.  Returns (whole Run, first Run, second Run, saved engine state, [the three
    things make returned]) for the caller's own assertions."""
    made = [make()]
    whole = run_steps(made[0][0], data, **run_kw)
    made[0][0].close()
    made.append(make())
    a, D1, G1 = made[1][:3]
    first = run_steps(a, data[:n_first], **run_kw)
    nets, saved = (D1.state_dict(), G1.state_dict()), a.state_dict()
    a.close()
    made.append(make(seed=99))  # other initial weights: everything comes from the saved state
    b, D2, G2 = made[2][:3]
    D2.load_state_dict(nets[0]), G2.load_state_dict(nets[1])
    b.load_state_dict(saved)
    second = run_steps(b, data[n_first:], **run_kw)
    assert_same_run(join_runs(first, second), whole, "resumed against uninterrupted")
    return whole, first, second, saved, made


# ----------------------------------------------------------------------------------------------------------------- processes
FAULT_CODES = (-6, -11, 134, 139)  # abort / segmentation fault, as a signal or as a shell reports it


def _rank_main(worker, rank, world, port, backend, out, args):
    """the child's frame: paths, the rendezvous, the process group of ``backend`` (None: no group), the worker, its result or its
    exception's text into the queue"""
    try:
        for p in (TESTS, ROOT):
            if p not in sys.path:
                sys.path.insert(0, p)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        if backend is None:
            out.put(("ok", rank, worker(rank, world, *args)))
            return
        import torch.distributed as dist
        if backend == "nccl":
            os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
            torch.cuda.set_device(0)
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        try:
            out.put(("ok", rank, worker(rank, world, *args)))
        finally:
            dist.destroy_process_group()
    except BaseException as e:  # surface the failure in the parent
        import traceback
        out.put(("err", rank, f"rank {rank}: {type(e).__name__}: {e}\n{traceback.format_exc()[-1500:]}"))


def run_ranks(worker, world, timeout, *args, backend="gloo", gpu=False, grace=30.0):
    """worker(rank, world, *args) in ``world`` spawned processes joined in a ``backend`` process group (None: no group); returns
    their results in rank order.  A worker that raises fails the test with its text; so does one that has not answered within
    ``timeout`` seconds.  The children are always reaped: joined for ``grace`` seconds, then terminated, then killed.
    gpu: the children open the GPU.  One of them killed at the limit, or dead of an abort or a segmentation fault, means a hung or
    faulted device: the whole pytest session ends there, so that nothing more is started on it."""
    import queue
    import socket
    import time
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(worker, r, world, port, backend, out, args)) for r in range(world)]
    run_ranks.children = procs  # for the launcher's own test
    results, problem, killed = {}, None, []
    try:
        for p in procs:
            p.start()
        deadline = time.monotonic() + timeout
        while len(results) < world and problem is None:
            try:
                status, rank, val = out.get(timeout=min(1.0, max(0.0, deadline - time.monotonic())))
            except queue.Empty:
                dead = [r for r, p in enumerate(procs) if r not in results and not p.is_alive()]
                if dead and out.empty():
                    problem = f"rank {dead[0]} exited with code {procs[dead[0]].exitcode} and no result"
                elif time.monotonic() >= deadline:
                    problem = f"no result from rank(s) {sorted(set(range(world)) - set(results))} within {timeout} s"
                continue
            if status == "ok":
                results[rank] = val
            else:
                problem = val
    finally:
        end = time.monotonic() + grace
        for p in procs:
            if p.pid is not None:
                p.join(timeout=max(0.0, end - time.monotonic()))
        for stop in ("terminate", "kill"):
            for r, p in enumerate(procs):
                if p.pid is not None and p.is_alive():
                    getattr(p, stop)()
                    p.join(timeout=5.0)
                    if r not in killed:
                        killed.append(r)
    faulted = [r for r, p in enumerate(procs) if r not in killed and p.exitcode in FAULT_CODES]
    if gpu and (killed or faulted):
        test = os.environ.get("PYTEST_CURRENT_TEST", worker.__name__)
        pytest.exit(f"{test}: a child process with the GPU open " + (f"had to be killed (rank(s) {killed})" if killed else
                    f"died with exit code {[procs[r].exitcode for r in faulted]} (rank(s) {faulted})") +
                    f"; {problem or 'its result had arrived'}.  Nothing more is started on this GPU by this session.", returncode=3)
    assert problem is None, problem
    return [results[r] for r in range(world)]


# ------------------------------------------------------------------------------------------- an engine step against a reference step
def assert_losses_match(got, ref, tol):
    """the three losses of an engine step against the reference step's, each within ``tol``"""
    for v, k in zip(got, ("d_real", "d_fake", "g")):
        assert abs(v - ref[k]) < tol, (k, got, ref)


def assert_penalty_matches(got, ref, rel, floor):
    assert abs(got - ref) < rel * abs(ref) + floor, (got, ref)


def assert_first_update_matches(D, w0, oracle, key, worst, close, share):
    """the first AdamW update of D's weight ``key`` (+-lr per element): no element further than ``worst`` from the reference's update,
    and more than ``share`` of them within ``close`` - sign flips on noise-level gradients only"""
    upd, ref_upd = D.state_dict()[key].detach().cpu() - w0[key], oracle.d[key].detach() - w0[key]
    assert float((upd - ref_upd).abs().max()) < worst and float(((upd - ref_upd).abs() < close).float().mean()) > share, key
