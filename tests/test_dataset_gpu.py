"""The device-resident dataset on the GPU: vg_dataset_fetch against the restated rule (tests/dataset_ref.py) - indices and labels at
every counter, rank and size, pixels bit-equal to torch's gather, flip and table on the host at every geometry and both layouts - the
engine with a dataset against the same engine host-fed the restated batches, bit for bit (eager and replayed, unconditional and
class-conditional), ``run``, resume, and the trainer.  Every test here fails on the parent commit: no export, no ``dataset`` argument."""
import os
import re

import numpy as np
import pytest
import torch

import dataset_ref as dr
import gpu_util as u

pytestmark = pytest.mark.gpu

SEED = 0x1234ABCD5678EF01
GUARD = 0x5A5A5A5A


def _fetch(images, labels, lut, layout, B, rank, world, flags, step, want_labels=True):
    """one launch on guarded outputs -> (imgs bf16 [B, C, IH, IH], labels_out or None, index_out); the guards must come back whole"""
    N = images.shape[0]
    C_, IH = (images.shape[1], images.shape[2]) if layout == 0 else (images.shape[3], images.shape[1])
    per = C_ * IH * IH
    out = torch.full(((B + 2) * per,), 7.0, dtype=torch.bfloat16, device="cuda")
    idx = torch.full((B + 8,), GUARD, dtype=torch.int32, device="cuda")
    lab = torch.full((B + 8,), GUARD, dtype=torch.int32, device="cuda") if want_labels and labels is not None else None
    counter = torch.tensor([step], dtype=torch.int32, device="cuda")
    u.call("vg_dataset_fetch", u.ptr(images), u.ptr(labels), N, C_, IH, layout, u.ptr(lut), u.ptr(out[per:]), None if lab is None else u.ptr(lab[4:]),
           u.ptr(idx[4:]), B, rank, world, flags, SEED, u.ptr(counter), u.stream())
    u.sync()
    assert bool((out[:per] == 7.0).all()) and bool((out[(B + 1) * per:] == 7.0).all()), "the image guards were written"
    for t in (idx, lab):
        assert t is None or (bool((t[:4] == GUARD).all()) and bool((t[B + 4:] == GUARD).all())), "an index / label guard was written"
    return out[per:(B + 1) * per].reshape(B, C_, IH, IH), None if lab is None else lab[4:B + 4].cpu().numpy(), idx[4:B + 4].cpu().numpy()


# ------------------------------------------------------------------------------------------------------------- which image, which label
@pytest.mark.parametrize("size", ["B", 50, 1000, 65537])
def test_indices_and_labels_follow_the_restated_rule(size):
    lut = dr.table((0.5,), (0.5,)).to(torch.bfloat16).cuda()
    seen = 0
    for B in (1, 7, 16):
        for rank, world in ((0, 1), (0, 2), (1, 2), (2, 3)):
            N = B * world if size == "B" else size
            if N < B * world:
                continue
            g = torch.Generator().manual_seed(N + B)
            images = torch.randint(0, 256, (N, 1, 4, 4), generator=g, dtype=torch.uint8).cuda()
            labels = torch.randint(0, 10, (N,), generator=g, dtype=torch.int32)
            labels_d = labels.cuda()
            nb = N // (B * world)
            for step in sorted({0, 1, nb - 1, nb, 3 * nb + 2}):
                for shuffle in (1, 0):
                    _, lab, idx = _fetch(images, labels_d, lut, 0, B, rank, world, shuffle, step)
                    want = dr.indices(step, N, B, rank, world, SEED, shuffle=bool(shuffle))
                    assert np.array_equal(idx, want), (N, B, rank, world, step, shuffle, idx, want)
                    assert np.array_equal(lab, labels.numpy()[want])
                    seen += 1
    assert seen >= 60
    # the pointers are optional: no labels at all, and labels without an output for them
    _, lab, idx = _fetch(images, None, lut, 0, B, rank, world, 1, 2)
    assert lab is None and np.array_equal(idx, dr.indices(2, N, B, rank, world, SEED))
    _, lab, idx = _fetch(images, labels_d, lut, 0, B, rank, world, 1, 2, want_labels=False)
    assert lab is None and np.array_equal(idx, dr.indices(2, N, B, rank, world, SEED))


# ---------------------------------------------------------------------------------------------------------------------------- pixels
MEANS = {1: ((0.1307,), (0.3081,)), 3: ((0.4914, 0.4822, 0.4465), (0.247, 0.243, 0.261))}


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("C_,IH", [(3, 32), (1, 32), (3, 36), (1, 28), (3, 64), (3, 128), (3, 224)])
def test_pixels_are_bit_equal_to_gather_flip_and_table(C_, IH, layout):
    N, B = 13, 5
    g = torch.Generator().manual_seed(100 * IH + 10 * C_ + layout)
    images = torch.randint(0, 256, (N, C_, IH, IH) if layout == 0 else (N, IH, IH, C_), generator=g, dtype=torch.uint8)
    mean, std = MEANS[C_]
    lut = dr.table(mean, std).to(torch.bfloat16)
    assert torch.equal(lut.float(), dr.table(mean, std))
    images_d, lut_d = images.cuda(), lut.cuda()
    flipped = []
    for flags in (1, 3, 2, 0):
        for step in (0, 1, 5):
            got, _, idx = _fetch(images_d, None, lut_d, layout, B, 0, 1, flags, step)
            want_idx = dr.indices(step, N, B, 0, 1, SEED, shuffle=bool(flags & 1))
            fl = dr.flips(step, N, B, 0, 1, SEED, flip=bool(flags & 2))
            assert np.array_equal(idx, want_idx)
            want = dr.decode(images, layout, want_idx, fl, mean, std).to(torch.bfloat16)
            assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16)), (C_, IH, layout, flags, step)
            if flags & 2:
                flipped += list(fl)
    assert any(flipped) and not all(flipped), "both orientations were exercised"


# ---------------------------------------------------------------------------------------------------------------------------- engine
B = 8
N_ENG = 3 * B + 5  # three batches an epoch: six steps cross an epoch boundary


def _engine(ds=None, K=0, **kw):
    from vit_gan_amd.config import Config
    from vit_gan_amd.engine import GanEngine
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.modules import ViTDiscriminator
    torch.manual_seed(5)
    D = ViTDiscriminator(Config(embeddings_dimension=384, classes_count=max(K, 1), batch_size=B, transformer_blocks_count=2)).cuda().train()
    G = SirenGenerator(layers=2, n_classes=K).cuda().train()
    return GanEngine(D, G, batch=B, seed=77, n_classes=K, dataset=ds, **kw)


def _dataset(K=0, N=N_ENG, **kw):
    from vit_gan_amd.data import DeviceDataset
    g = torch.Generator().manual_seed(9)
    images = torch.randint(0, 256, (N, 3, 32, 32), generator=g, dtype=torch.uint8)
    labels = torch.randint(0, K, (N,), generator=g) if K else None
    return images, labels, DeviceDataset(images.clone(), labels, flip=True, **kw)


def _snapshot(eng):
    fd, fg = eng.vit._flat, eng.gen._flat
    return [t.detach().clone().cpu() for t in (fd.flat, fd.shadow, fg.flat, fg.shadow, eng.m_d, eng.v_d, eng.m_g, eng.v_g, eng.step_t)]


def _same(a, b, what):
    for name, x, y in zip(("D master", "D shadow", "G master", "G shadow", "m_d", "v_d", "m_g", "v_g", "step_t"), a, b):
        assert torch.equal(x, y), f"{what}: {name} differs"


def _restated_batch(images, labels, seed, step, N=N_ENG):
    idx = dr.indices(step, N, B, 0, 1, seed)
    real = dr.decode(images, 0, idx, dr.flips(step, N, B, 0, 1, seed), (0.5,) * 3, (0.5,) * 3)
    return idx, real.cuda(), None if labels is None else labels[torch.as_tensor(idx)].cuda()


@pytest.mark.parametrize("K", [0, 3])
@pytest.mark.parametrize("use_graph", [False, True])
def test_dataset_engine_is_the_host_fed_engine_bit_for_bit(use_graph, K):
    from vit_gan_amd.data import data_seed
    images, labels, ds = _dataset(K)
    fed, own, ran = _engine(None, K, use_graph=use_graph), _engine(ds, K, use_graph=use_graph), _engine(ds, K, use_graph=use_graph)
    try:
        assert own.data_seed == data_seed(77) and own.steps_per_epoch == 3 and fed.batch_indices is None and own.epoch == 0
        with pytest.raises(ValueError, match="without real and labels"):
            own.step(torch.zeros(B, 3, 32, 32, device="cuda"))
        with pytest.raises(ValueError, match="real must be"):
            fed.step()
        with pytest.raises(RuntimeError, match="no dataset"):
            fed.run(1)
        seen = []
        for s in range(6):
            idx, real, lab = _restated_batch(images, labels, own.data_seed, s)
            got = own.step().clone()
            want = (fed.step(real, labels=lab) if K else fed.step(real)).clone()
            assert torch.equal(got, want), f"step {s}: losses {got.tolist()} against host-fed {want.tolist()}"
            assert np.array_equal(own.batch_indices.cpu().numpy(), idx), s
            assert torch.equal(own.imgs[:B].float().cpu(), real.cpu()) and torch.equal(own.z, fed.z)
            if K:
                assert torch.equal(own.real_labels, lab.to(torch.int32)) and torch.equal(own.fake_labels, fed.fake_labels)
            seen.append(tuple(idx))
        assert len(set(seen)) == 6 and own.epoch == 2
        assert sorted(np.concatenate(seen[:3])) == sorted(set(np.concatenate(seen[:3]))), "an epoch visits no image twice"
        _same(_snapshot(own), _snapshot(fed), "dataset engine against host-fed")
        # run(6) is six step() calls
        last = ran.run(6)
        _same(_snapshot(ran), _snapshot(own), "run(6) against six steps")
        assert torch.equal(last, own.losses) and ran.steps == 6 and ran.graph_active == use_graph
        if use_graph:  # bare replays: every one fetches its own batch
            three = []
            for _ in range(3):
                ran.run(1)
                three.append(tuple(ran.batch_indices.cpu().tolist()))
            assert len(set(three)) == 3 and three == [tuple(dr.indices(s, N_ENG, B, 0, 1, ran.data_seed)) for s in (6, 7, 8)]
    finally:
        for e in (fed, own, ran):
            e.close()


@pytest.mark.parametrize("use_graph", [False, True])
def test_resume_continues_the_epoch_bit_for_bit(use_graph):
    images, labels, ds = _dataset()
    ref = _engine(ds, use_graph=use_graph)
    ref_losses = [ref.step().clone() for _ in range(6)]
    ref_s = _snapshot(ref)
    ref.close()
    first = _engine(ds, use_graph=use_graph)
    first.run(4)
    nets = ({k: v.clone() for k, v in first._disc.state_dict().items()}, {k: v.clone() for k, v in first.gen.state_dict().items()})
    state = first.state_dict()
    first.close()
    assert tuple(state["dataset"]) == (N_ENG, B, 1, True, True, first.data_seed) and int(state["step_t"]) == 4
    second = _engine(ds, use_graph=use_graph)
    with torch.no_grad():
        for p in list(second._disc.parameters()) + list(second.gen.parameters()):
            p.add_(0.01)
    second._disc.load_state_dict(nets[0], strict=True)
    second.gen.load_state_dict(nets[1], strict=True)
    second.load_state_dict(state)
    assert second.epoch == 1
    got = [second.step().clone() for _ in range(2)]
    assert np.array_equal(second.batch_indices.cpu().numpy(), dr.indices(5, N_ENG, B, 0, 1, second.data_seed))
    assert torch.equal(torch.stack(got), torch.stack(ref_losses[4:]))
    _same(_snapshot(second), ref_s, "resumed against uninterrupted")
    second.close()
    # a state of another dataset, or of none, does not continue this epoch: refused, strict or not
    _, _, bigger = _dataset(N=N_ENG + 1)
    other = _engine(bigger)
    for strict in (True, False):
        with pytest.raises(ValueError, match="dataset"):
            other.load_state_dict(state, strict=strict)
    other.close()
    plain = _engine()
    with pytest.raises(ValueError, match="dataset"):
        plain.load_state_dict(state)
    plain_state = plain.state_dict()
    assert "dataset" not in plain_state
    plain.close()
    third = _engine(ds)
    with pytest.raises(ValueError, match="dataset"):
        third.load_state_dict(plain_state)
    third.close()


def test_external_noise_keeps_z_the_callers():
    images, labels, ds = _dataset()
    own, fed = _engine(ds, external_noise=True, use_graph=True), _engine(None, external_noise=True, use_graph=True)
    g = torch.Generator().manual_seed(4)
    with pytest.raises(ValueError, match="external_noise"):
        own.run(2)
    for s in range(3):
        z = torch.randn(B, 1024, generator=g).cuda()
        _, real, _ = _restated_batch(images, None, own.data_seed, s)
        assert torch.equal(own.step(z=z), fed.step(real, z))
    _same(_snapshot(own), _snapshot(fed), "external noise")
    own.close()
    fed.close()


# --------------------------------------------------------------------------------------------------------------------------- trainer
CFG = {"epochs": 3, "batch_size": 8, "embeddings_dimension": 128, "attention_heads_count": 4, "transformer_blocks_count": 1}


def test_trainer_runs_epochs_from_the_dataset(tmp_path):
    from vit_gan_amd.training import save_images, train_model
    images, _, ds = _dataset(N=20)
    out = train_model(CFG, dataset=ds, max_epochs=2, output_base=str(tmp_path))
    eng = out["engine"]
    assert eng.steps == 4 and eng.steps_per_epoch == 2 and eng.epoch == 2 and len(out["history"]) == 2
    log = open(os.path.join(out["dirs"].save, "training.log")).read()
    assert len(re.findall(r"Epoch \[[01]/2\] \| Disc Loss: \S+, Gen Loss: \S+ \| FID: nan", log)) == 2, log
    assert "Exception" not in log
    for e in (0, 1):  # the input grid is the batch the epoch's first step trains on, decoded from the restated rule
        path = os.path.join(out["dirs"].input, f"input_epoch_{e}.png")
        _, real, _ = _restated_batch(images, None, eng.data_seed, 2 * e, N=20)
        save_images(str(tmp_path / "want.png"), real, 8)
        assert open(path, "rb").read() == open(tmp_path / "want.png", "rb").read(), e
