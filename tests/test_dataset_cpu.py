"""The device-resident dataset without a GPU: the restated rule (tests/dataset_ref.py) is a bijection, covers an epoch across ranks, moves
between epochs and is uniform; the product's host mirrors and table equal it and equal torch; two planted defects fail the same checks;
every return code of vg_dataset_fetch; the argument errors of the engine and the trainer; the CIFAR-10 binary reader.  Every test here
fails on the parent commit, which has no module ``data``, no export and no ``dataset`` argument."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import dataset_ref as dr
import vit_gan_amd  # noqa: F401
from vit_gan_amd import _lib
from vit_gan_amd.config import Config
from vit_gan_amd.data import DeviceDataset, data_seed

SEED = 0x1234ABCD5678EF01
SPLITS = ((1, 1), (7, 1), (16, 2), (5, 3))


# ------------------------------------------------------------------------------------------------------------ the checks themselves
def check_bijection(perm, N, epoch):
    count = []
    idx = perm(np.arange(N), N, epoch, count)
    assert idx.min() >= 0 and idx.max() < N, (N, epoch)
    assert np.array_equal(np.sort(idx), np.arange(N)), f"N {N}, epoch {epoch}: not a bijection"
    return count[0] if count else 0.0


def check_epoch_cover(index_fn, N, B, world):
    """the nb B world positions of all ranks of one epoch give distinct indices, and every rank's share is disjoint from the others'"""
    nb = N // (B * world)
    for epoch in (0, 3):
        got = np.concatenate([index_fn(epoch * nb + j, N, B, rank, world) for j in range(nb) for rank in range(world)])
        assert got.size == nb * B * world and got.min() >= 0 and got.max() < N
        assert np.unique(got).size == got.size, f"N {N}, B {B}, world {world}, epoch {epoch}: an image is visited twice"


# ------------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("N", dr.SIZES)
def test_restated_permutation_is_a_bijection(N):
    for epoch in dr.EPOCHS:
        mean_passes = check_bijection(lambda p, n, e, count: dr.perm_epoch(p, n, e, SEED, count=count), N, epoch)
        assert mean_passes <= 4.0, (N, epoch, mean_passes)  # the Feistel domain is at most 4 N wide
    assert dr.half_width(N) == max(1, int(np.ceil(int(N - 1).bit_length() / 2)))


@pytest.mark.parametrize("B,world", SPLITS)
def test_ranks_of_an_epoch_visit_distinct_images(B, world):
    for N in (B * world, 53, 1000):
        if N >= B * world:
            check_epoch_cover(lambda s, n, b, r, w: dr.indices(s, n, b, r, w, SEED), N, B, world)
            check_epoch_cover(lambda s, n, b, r, w: dr.indices(s, n, b, r, w, SEED, shuffle=False), N, B, world)


def test_epochs_differ_and_seeds_differ():
    N = 1000
    p = np.arange(N)
    a = dr.perm_epoch(p, N, 0, SEED)
    for other in (dr.perm_epoch(p, N, 1, SEED), dr.perm_epoch(p, N, 2, SEED), dr.perm_epoch(p, N, 0, SEED + 1)):
        agree = float((a == other).mean())
        assert agree < 0.02, agree  # 1 / N expected; 20 / N is a 19 sigma excess of a Poisson(1) count
    assert np.array_equal(a, dr.perm_epoch(p, N, 0, SEED))
    # neighbouring positions land far apart: the mean distance of two uniform draws is N / 3
    assert 0.25 * N < float(np.abs(np.diff(a)).mean()) < 0.42 * N


def test_index_at_a_position_is_uniform_over_epochs():
    N, E = 1000, 20000
    assert np.array_equal(dr.perm_epochs(7, N, np.arange(50), SEED), [int(dr.perm_epoch([7], N, e, SEED)[0]) for e in range(50)])
    for p in (0, 1, 999):
        idx = dr.perm_epochs(p, N, np.arange(E), SEED)
        counts = np.bincount(idx, minlength=N).astype(np.float64)
        chi2 = float(((counts - E / N) ** 2 / (E / N)).sum())
        z = (chi2 - (N - 1)) / np.sqrt(2.0 * (N - 1))
        print(f"position {p}: chi-square z-score {z:.2f}")
        assert abs(z) < 5.0, (p, z)
    a = dr.perm_epochs(0, N, np.arange(E), SEED)
    assert float((a[1:] == a[:-1]).mean()) < 0.003  # consecutive epochs agree at a position 1 / N of the time: 20 +- 4.5 of 20 000


def test_flips_are_fair_and_keyed_on_the_visit():
    N, B = 4096, 64
    f = np.concatenate([dr.flips(s, N, B, 0, 1, SEED) for s in range(N // B)])
    assert abs(float(f.mean()) - 0.5) < 5 * 0.5 / np.sqrt(N)
    assert not np.array_equal(f[:B], dr.flips(N // B, N, B, 0, 1, SEED)), "the next epoch draws again"
    assert not np.array_equal(dr.flips(0, N, B, 0, 2, SEED), dr.flips(0, N, B, 1, 2, SEED)), "ranks draw their own"
    assert not dr.flips(0, N, B, 0, 1, SEED, flip=False).any()


# -------------------------------------------------------------------------------------------------- the product equals the restatement
def _images(N, C, IH, layout, seed=0):
    g = torch.Generator().manual_seed(seed)
    shape = (N, C, IH, IH) if layout == 0 else (N, IH, IH, C)
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)


def test_product_indices_flips_and_table_equal_the_restatement():
    mean, std = (0.4914, 0.4822, 0.4465), (0.247, 0.243, 0.261)
    for N in (1, 2, 17, 53, 1000, 65537):
        ds = DeviceDataset(torch.zeros(N, 3, 8, 8, dtype=torch.uint8), layout="nchw", flip=True, mean=mean, std=std)
        plain = DeviceDataset(torch.zeros(N, 3, 8, 8, dtype=torch.uint8), layout="nchw", shuffle=False)
        assert len(ds) == N
        for B, world in SPLITS:
            if N < B * world:
                with pytest.raises(ValueError, match="fewer than one global batch"):
                    ds.steps_per_epoch(B, world)
                continue
            nb = N // (B * world)
            assert ds.steps_per_epoch(B, world) == nb
            for step in (0, 1, nb - 1, nb, 3 * nb + 2):
                for rank in range(world):
                    at = (step, B, rank, world, SEED)
                    assert np.array_equal(ds.indices(*at).numpy(), dr.indices(step, N, B, rank, world, SEED)), (N, at)
                    assert np.array_equal(ds.flips(*at).numpy(), dr.flips(step, N, B, rank, world, SEED)), (N, at)
                    assert np.array_equal(plain.indices(*at).numpy(), dr.indices(step, N, B, rank, world, SEED, shuffle=False))
                    assert not plain.flips(*at).any()
    # the product's permutation under the same checks as the restatement
    ds = DeviceDataset(torch.zeros(53, 1, 4, 4, dtype=torch.uint8), layout="nchw")
    for B, world in SPLITS:
        check_epoch_cover(lambda s, n, b, r, w: ds.indices(s, b, r, w, SEED).numpy(), 53, B, world)
    # the table: the restatement's, and torch's ((x / 255) - mean) / std -> bf16 on the 256 byte values
    ds = DeviceDataset(torch.zeros(4, 3, 8, 8, dtype=torch.uint8), layout="nchw", mean=mean, std=std)
    assert ds.lut.shape == (3, 256) and ds.lut.dtype == torch.float32 and torch.equal(ds.lut, dr.table(mean, std))
    x = torch.arange(256, dtype=torch.uint8).reshape(1, 1, 16, 16).expand(1, 3, 16, 16)
    want = ((x.float() / 255) - torch.tensor(mean).reshape(1, 3, 1, 1)) / torch.tensor(std).reshape(1, 3, 1, 1)
    assert torch.equal(ds.lut.reshape(1, 3, 16, 16), want.to(torch.bfloat16).float())
    assert torch.equal(ds.lut_bf16.float(), ds.lut) and ds.lut_bf16.dtype == torch.bfloat16
    one = DeviceDataset(torch.zeros(4, 3, 8, 8, dtype=torch.uint8), layout="nchw")
    assert torch.equal(one.lut, dr.table((0.5,) * 3, (0.5,) * 3)) and float(one.lut[0, 0]) == -1.0 and float(one.lut[2, 255]) == 1.0


def test_product_decode_equals_torch_gather_flip_and_table():
    mean, std = (0.1, 0.5, 0.9), (0.5, 0.25, 1.0)
    for layout in (0, 1):
        imgs = _images(11, 3, 8, layout, seed=layout)
        ds = DeviceDataset(imgs, layout="nchw" if layout == 0 else "nhwc", mean=mean, std=std, flip=True)
        idx, flip = [3, 10, 0, 3], [True, False, True, False]
        got = ds.decode(idx, flip)
        assert got.dtype == torch.float32 and got.shape == (4, 3, 8, 8)
        assert torch.equal(got, dr.decode(imgs, layout, idx, flip, mean, std))
        assert torch.equal(got, got.to(torch.bfloat16).float()), "every value is a bf16"
        assert torch.equal(ds.decode(idx), dr.decode(imgs, layout, idx, [False] * 4, mean, std))
        assert torch.equal(got[0], got[3].flip(2))


def test_layout_and_argument_errors_of_the_dataset():
    assert DeviceDataset(torch.zeros(2, 3, 8, 8, dtype=torch.uint8)).layout == 0
    assert DeviceDataset(torch.zeros(2, 8, 8, 3, dtype=torch.uint8)).layout == 1
    assert DeviceDataset(np.zeros((2, 8, 8, 1), dtype=np.uint8)).C == 1
    for shape, kw, match in (((2, 3, 4, 4), {}, "auto"), ((2, 8, 8, 8), {}, "auto"), ((2, 3, 8, 12), {}, "square"), ((2, 3, 8, 8), dict(layout="chw"), "layout"),
                             ((2, 5, 8, 8), dict(layout="nchw"), "C <= 4"), ((2, 1, 6, 6), dict(layout="nchw"), "IH"), ((2, 1, 4, 4), dict(layout="nchw", std=0.0), "std"),
                             ((2, 3, 8, 8), dict(mean=(0.5, 0.5)), "mean"), ((2, 3, 8, 8), dict(labels=torch.zeros(3, dtype=torch.int64)), "labels"),
                             ((2, 3, 8, 8), dict(labels=torch.zeros(2)), "labels")):
        with pytest.raises(ValueError, match=match):
            DeviceDataset(torch.zeros(shape, dtype=torch.uint8), **kw)
    with pytest.raises(ValueError, match="uint8"):
        DeviceDataset(torch.zeros(2, 3, 8, 8))
    ds = DeviceDataset(torch.zeros(8, 3, 8, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="rank"):
        ds.indices(0, 4, rank=2, world=2)
    assert data_seed(7) == data_seed(7) and data_seed(7) != data_seed(8)


# ------------------------------------------------------------------------------------------------------------------ planted defects
def test_modulo_in_place_of_cycle_walking_is_rejected():
    """p % N after one Feistel pass folds the 2^2k domain onto [0, N): two positions collide whenever N is not a power of four"""
    broken = lambda p, n, e, count: dr.perm_epoch(p, n, e, SEED, walk=False)  # noqa: E731
    for N in (3, 5, 17, 50, 1000, 65537):
        with pytest.raises(AssertionError, match="bijection"):
            check_bijection(broken, N, 0)
    with pytest.raises(AssertionError, match="visited twice"):
        check_epoch_cover(lambda s, n, b, r, w: dr.indices(s, n, b, r, w, SEED, walk=False), 1000, 16, 2)


def test_a_per_rank_seed_is_rejected():
    """with the rank in the seed every rank walks its own permutation and the shares of one epoch overlap"""
    with pytest.raises(AssertionError, match="visited twice"):
        check_epoch_cover(lambda s, n, b, r, w: dr.indices(s, n, b, r, w, SEED + 1000003 * r), 1000, 16, 2)
    with pytest.raises(AssertionError, match="visited twice"):
        check_epoch_cover(lambda s, n, b, r, w: dr.indices(s, n, b, r, w, SEED ^ (r << 17)), 53, 5, 3)


# ---------------------------------------------------------------------------------------------------------------------------- C ABI
def test_export_exists_with_abi_9():
    lib = _lib.lib()
    assert lib.vg_abi_version() == _lib.ABI_VERSION == 9
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vitgan_hip.h")).read()
    assert hasattr(lib, "vg_dataset_fetch") and "vg_dataset_fetch" in _lib._SIGNATURES and "int vg_dataset_fetch(" in header
    assert len(_lib._SIGNATURES["vg_dataset_fetch"][1]) == 17


def test_every_return_code_comes_back_before_any_launch():
    lib, p, odd = _lib.lib(), C.c_void_p(64), C.c_void_p(72)  # (non-null dummies: never dereferenced on these paths; no device here)
    #          images labels N  C  IH layout lut imgs labels_out index_out B rank world flags seed step stream
    good = [p, p, 1000, 3, 32, 0, p, p, p, p, 16, 0, 1, 3, 1, p, None]

    def rc(**kw):
        names = ("images", "labels", "N", "C", "IH", "layout", "lut", "imgs", "labels_out", "index_out", "B", "rank", "world", "flags", "seed", "step")
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.vg_dataset_fetch(*a)

    for name in ("images", "lut", "imgs", "step"):
        assert rc(**{name: None}) == -1, name
    assert rc(labels=None) == -1, "labels_out without labels"
    for name in ("N", "C", "IH", "B"):
        assert rc(**{name: 0}) == -1 and rc(**{name: -3}) == -1, name
    assert rc(world=0) == -2 and rc(world=-1) == -2 and rc(rank=-1) == -2 and rc(rank=1) == -2 and rc(rank=2, world=2) == -2
    assert rc(layout=2) == -2 and rc(layout=-1) == -2 and rc(flags=4) == -2 and rc(flags=-1) == -2
    assert rc(N=15) == -2 and rc(N=31, world=2) == -2 and rc(N=2 ** 31) == -2
    # (IH IH % 8 == 0 implies IH % 4 == 0 and so C IH IH % 16 == 0: the second geometry rule cannot fail on its own)
    assert rc(IH=6, C=1) == -3 and rc(IH=30) == -3 and rc(IH=2, C=4) == -3, "IH IH % 8"
    assert rc(C=5) == -3, "C > 4"
    assert rc(IH=240, C=3) == -3 and rc(IH=408, C=1) == -3, "one image and the table exceed 160 KiB of LDS"
    assert rc(images=odd) == -3 and rc(lut=odd) == -3 and rc(imgs=odd) == -3
    # the order: -1 before -2 before -3
    assert rc(images=None, world=0, C=5) == -1 and rc(world=0, C=5) == -2


# ----------------------------------------------------------------------------------------------------------- engine and trainer
def _nets(Kc=1, n_classes=0):
    from vit_gan_amd.generator import SirenGenerator
    from vit_gan_amd.modules import ViTDiscriminator
    torch.manual_seed(0)
    D = ViTDiscriminator(Config(embeddings_dimension=128, classes_count=Kc, dropout_rate=0.0, batch_size=4, transformer_blocks_count=1))
    return D, SirenGenerator(latent=64, embed=128, heads=4, layers=1, siren_hidden=128, dropout=0.0, n_classes=n_classes)


def test_engine_refuses_bad_datasets_without_a_device(monkeypatch):
    from vit_gan_amd import engine
    D, G = _nets()
    img = lambda n, ih=32, c=3: torch.zeros(n, c, ih, ih, dtype=torch.uint8)  # noqa: E731
    lab = torch.zeros(16, dtype=torch.int64)
    with pytest.raises(TypeError, match="DeviceDataset"):
        engine.GanEngine(D, G, batch=4, dataset=img(16))
    for ds, match in ((DeviceDataset(img(16, 64), layout="nchw"), "3 x 64 x 64"), (DeviceDataset(img(16, 32, 1), layout="nchw"), "1 x 32 x 32"),
                      (DeviceDataset(img(16), lab), "has labels, n_classes=0"), (DeviceDataset(img(3)), "fewer than one global batch of 4 x 1")):
        with pytest.raises(ValueError, match=match):
            engine.GanEngine(D, G, batch=4, dataset=ds)
    D3, G3 = _nets(3, 3)
    with pytest.raises(ValueError, match="has no labels, n_classes=3"):
        engine.GanEngine(D3, G3, batch=4, n_classes=3, dataset=DeviceDataset(img(16)))
    monkeypatch.setattr(engine, "world_size", lambda pg: 2)
    with pytest.raises(ValueError, match="fewer than one global batch of 4 x 2"):
        engine.GanEngine(D, G, batch=4, dataset=DeviceDataset(img(7)))
    monkeypatch.undo()
    # what is allowed gets as far as the device check: label VALUES are not read, and the other options go with a dataset
    wild = torch.tensor([-5, 99] * 8)
    for nets, kw in (((D, G), dict(dataset=DeviceDataset(img(4)))), ((D, G), dict(dataset=DeviceDataset(img(16)), use_graph=True, diffaug="color", ema_decay=0.9)),
                     ((D, G), dict(dataset=DeviceDataset(img(16)), external_noise=True, two_stream=True)),
                     ((D3, G3), dict(dataset=DeviceDataset(img(16), wild), n_classes=3))):
        with pytest.raises(RuntimeError, match="cuda"):
            engine.GanEngine(*nets, batch=4, **kw)
    with pytest.raises(RuntimeError, match="cuda"):  # off is off
        engine.GanEngine(D, G, batch=4, dataset=None)


def test_trainer_refuses_bad_arguments_without_a_device():
    from vit_gan_amd.training import SyntheticLoader, train_model
    cfg = dict(batch_size=4, image_size=32)
    ds = DeviceDataset(torch.zeros(16, 3, 32, 32, dtype=torch.uint8))
    labelled = DeviceDataset(torch.zeros(16, 3, 32, 32, dtype=torch.uint8), torch.zeros(16, dtype=torch.int64))
    with pytest.raises(ValueError, match="either dataset or data_loader"):
        train_model(cfg, dataset=ds, data_loader=SyntheticLoader(Config(**cfg), 1, torch.device("cpu")), save_artifacts=False)
    with pytest.raises(TypeError, match="DeviceDataset"):
        train_model(cfg, dataset=torch.zeros(16, 3, 32, 32, dtype=torch.uint8), save_artifacts=False)
    with pytest.raises(ValueError, match="the configuration says 3 x 64 x 64"):
        train_model(dict(batch_size=4, image_size=64), dataset=ds, save_artifacts=False)
    with pytest.raises(ValueError, match="fewer than one global batch"):
        train_model(dict(batch_size=32, image_size=32), dataset=ds, save_artifacts=False)
    with pytest.raises(ValueError, match="labels"):
        train_model(cfg, dataset=ds, conditional=True, save_artifacts=False)
    with pytest.raises(ValueError, match="labels"):
        train_model(cfg, dataset=labelled, save_artifacts=False)
    if not torch.cuda.is_available():  # a good call gets as far as the device check
        with pytest.raises(RuntimeError, match="MI355X"):
            train_model(cfg, dataset=ds, save_artifacts=False)


# ------------------------------------------------------------------------------------------------------------- the CIFAR-10 reader
def test_cifar10_binary_round_trip(tmp_path):
    g = np.random.default_rng(3)
    rec = g.integers(0, 256, size=(20, 3073), dtype=np.uint8)
    rec[:, 0] = g.integers(0, 10, size=20)
    rec.tofile(tmp_path / "test_batch.bin")
    ds = DeviceDataset.from_cifar10_bin(str(tmp_path), train=False, flip=True)
    assert len(ds) == 20 and (ds.C, ds.IH, ds.layout) == (3, 32, 0) and ds.flip and ds.shuffle
    assert ds.images.dtype == torch.uint8 and np.array_equal(ds.images.numpy(), rec[:, 1:].reshape(20, 3, 32, 32))
    assert ds.labels.dtype == torch.int32 and np.array_equal(ds.labels.numpy(), rec[:, 0])
    for i in range(1, 6):
        rec[4 * (i - 1):4 * i].tofile(tmp_path / f"data_batch_{i}.bin")
    tr = DeviceDataset.from_cifar10_bin(str(tmp_path))
    assert len(tr) == 20 and torch.equal(tr.images, ds.images) and torch.equal(tr.labels, ds.labels)
    os.remove(tmp_path / "data_batch_3.bin")
    with pytest.raises(FileNotFoundError, match="never downloaded"):
        DeviceDataset.from_cifar10_bin(str(tmp_path))
    (tmp_path / "data_batch_3.bin").write_bytes(b"\x00" * 100)
    with pytest.raises(ValueError, match="3073"):
        DeviceDataset.from_cifar10_bin(str(tmp_path))
