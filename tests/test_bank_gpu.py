"""csrc/databank.hip on the MI355X, bit for bit on every element against tests/bank_hostmodel.py (no tolerance anywhere):

  * rg_bank_reid_batch at five geometries (16-byte rows, two element-wise tails, the test-time form, one real shape), N in
    {1, 5, 64}, with draws planted at their corners, and against the existing composition on an fp32 batch
    (table gather -> ops.flip_pad_crop -> ops.erase_rects_ -> flip_images);
  * rg_bank_gan_batch and rg_bank_pose_batch (the latter against ops.pose_maps(mode=1) + flip_images on the gathered centres);
  * byte-equal repeats and side-stream runs, launch accounting at the rg_hip.lib boundary, the allocation bound of a `next()`,
    the host check in front of the launch;
  * end to end: a ClusterContrastTrainer.step, extract_features_device and a train_all iteration fed by the loaders.
"""
import numpy as np
import pytest
import torch

from tests import bank_hostmodel as HM

pytestmark = pytest.mark.gpu

M = 7
GEOMETRIES = {                       # (Hs, Ws, pad, H, W)
    "vec": (16, 8, 2, 16, 8),
    "tail6": (12, 6, 2, 12, 6),
    "tail10": (10, 10, 3, 10, 10),
    "testtime": (16, 8, 0, 16, 8),
    "real": (256, 128, 10, 256, 128),
}


def _planes(Hs, Ws, seed=0):
    """[M, Hs, Ws, 3] uint8: plane 0 all 0, plane 1 all 255, the rest tell images, channels, rows and columns apart"""
    m, r, q, c = np.meshgrid(np.arange(M), np.arange(Hs), np.arange(Ws), np.arange(3), indexing="ij")
    a = (53 * m + 37 * r + 11 * q + 101 * c + (r * q) % 7) % 256
    a = (a + np.random.RandomState(seed).randint(0, 3, size=a.shape)) % 256
    a[0], a[1] = 0, 255
    return a.astype(np.uint8)


def _indices(N):
    """repeated and non-monotone bank rows; the all-0 and the all-255 plane among the first five"""
    return [(6, 0, 6, 1, 3, 2, 5, 4)[n % 8] if n % 11 else 4 for n in range(N)]


def _corner_draws(N, Hs, Ws, pad, H, W):
    """(flip, top, left, er0, ec0, eh, ew) per sample: offsets at 0 and at their maximum, both flips in every batch of more than
    one sample, no rectangle, a rectangle in each corner, a 1 x 1 one, and the largest the draw rule allows, (H-1) x (W-1)"""
    tmax, lmax = 2 * pad + Hs - H, 2 * pad + Ws - W
    h2, w2 = max(H // 3, 1), max(W // 3, 1)
    rects = [(H // 2, W // 2, 1, 1), (0, 0, 0, 0), (0, 0, H - 1, W - 1), (0, 0, h2, w2), (0, W - w2, h2, w2), (H - h2, 0, h2, w2),
             (H - h2, W - w2, h2, w2), (1, 1, H - 1, W - 1), (H - 1, W - 1, 1, 1), (1, 0, H - 1, W - 1)]
    offs = [(0, 0), (tmax, lmax), (0, lmax), (tmax, 0), (tmax // 2, lmax // 2 + lmax % 2)]
    out = []
    for n in range(N):
        k = n + 1 if N > 1 else 3                       # a single sample: flipped, both offsets at their maximum, a rectangle
        out.append(((k % 2),) + offs[(k // 2) % len(offs)] + rects[k % len(rects)])
    return out


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def luts(dev):
    from rg_hip import ops
    return (ops.bank_lut(HM.REID_MEAN, HM.REID_STD).to(dev), ops.bank_lut(HM.GAN_MEAN, HM.GAN_STD).to(dev),
            torch.tensor(HM.REID_MEAN, dtype=torch.float32).to(dev))


_MODEL_CACHE = {}


def _reid_case(name, N):
    """(planes, idx, draws, host-model batch), computed once per case and left unchanged"""
    key = (name, N)
    if key not in _MODEL_CACHE:
        Hs, Ws, pad, H, W = GEOMETRIES[name]
        planes, idx = _planes(Hs, Ws), _indices(N)
        draws = [(0,) * 7] * N if name == "testtime" else _corner_draws(N, Hs, Ws, pad, H, W)
        ref = HM.reid_batch_model(planes, idx, draws, HM.bank_lut(HM.REID_MEAN, HM.REID_STD), np.asarray(HM.REID_MEAN, np.float32),
                                  H, W, pad)
        ref.setflags(write=False)
        _MODEL_CACHE[key] = (planes, idx, draws, ref)
    return _MODEL_CACHE[key]


CASES = [(g, n) for g in ("vec", "tail6", "tail10", "testtime") for n in (1, 5, 64)] + [("real", 3)]


@pytest.mark.parametrize("name,N", CASES, ids=["%s-n%d" % c for c in CASES])
def test_reid_batch_equals_the_host_model(dev, luts, name, N):
    from rg_hip import ops
    Hs, Ws, pad, H, W = GEOMETRIES[name]
    planes, idx, draws, ref = _reid_case(name, N)
    if N > 1 and name != "testtime":
        assert {d[0] for d in draws} == {0, 1} and any(d[5] == 0 for d in draws) and any(d[5] == H - 1 and d[6] == W - 1 for d in draws)
    bank = torch.from_numpy(planes).to(dev)
    got = ops.bank_reid_batch(bank, ops.bank_draws(idx, draws), luts[0], luts[2], (H, W), pad)
    assert got.dtype == torch.float32 and tuple(got.shape) == (N, 3, H, W)
    wrong = int((got.cpu().numpy().view(np.uint32) != ref.view(np.uint32)).sum())
    print("%s N=%d: %d of %d elements differ from the host model" % (name, N, wrong, ref.size))
    assert wrong == 0


@pytest.mark.parametrize("name,N", [("vec", 5), ("tail6", 64), ("tail10", 5), ("real", 3)])
def test_reid_batch_equals_the_existing_composition(dev, luts, name, N):
    """table gather (torch indexing on the device) -> ops.flip_pad_crop -> ops.erase_rects_ -> flip_images on an fp32 batch"""
    from rg_hip import ops
    from reid.utils.data.device_pipeline import flip_images
    Hs, Ws, pad, H, W = GEOMETRIES[name]
    planes, idx, draws, _ = _reid_case(name, N)
    bank = torch.from_numpy(planes).to(dev)
    got = ops.bank_reid_batch(bank, ops.bank_draws(idx, draws), luts[0], luts[2], (H, W), pad)
    sel = bank[torch.tensor(idx, device=dev)].long()                                        # [N, Hs, Ws, 3]
    x = torch.stack([luts[0][c][sel[..., c]] for c in range(3)], dim=1).contiguous()         # [N, 3, Hs, Ws] fp32
    par = torch.tensor([(0, d[1], d[2]) for d in draws], dtype=torch.int32).to(dev)
    x = ops.flip_pad_crop(x, par, (H, W), pad=pad, pad_value=luts[0][:, 0].contiguous())
    x = ops.erase_rects_(x, torch.tensor([d[3:7] for d in draws], dtype=torch.int32).to(dev), luts[2])
    x = flip_images(x, [d[0] for d in draws])
    assert _bytes(got) == _bytes(x)


@pytest.mark.parametrize("Hg,Wg,N", [(8, 4, 5), (8, 4, 64), (7, 5, 5), (128, 64, 3)])
def test_gan_batch_equals_the_host_model(dev, luts, Hg, Wg, N):
    from rg_hip import ops
    planes, idx = _planes(Hg, Wg, seed=1), _indices(N)
    flips = [(n + 1) % 2 if n % 5 else 1 for n in range(N)]
    ref = HM.gan_batch_model(planes, idx, flips, HM.bank_lut(HM.GAN_MEAN, HM.GAN_STD))
    got = ops.bank_gan_batch(torch.from_numpy(planes).to(dev), ops.bank_draws(idx, [(f, 0, 0, 0, 0, 0, 0) for f in flips]), luts[1])
    assert tuple(got.shape) == (N, 3, Hg, Wg) and _bytes(got) == ref.tobytes()


def _centres(Hg, Wg, J=18):
    g = np.random.RandomState(4)
    c = np.stack([g.randint(0, Hg, size=(M, J)), g.randint(0, Wg, size=(M, J))], axis=2).astype(np.int64)
    c[0, 3] = HM.MISSING                                  # missing joints: both coordinates, or one
    c[2, 0, 1] = HM.MISSING
    c[5] = HM.MISSING                                     # an image without any joint
    c[3, 1] = (-9, Wg + 4)                                # centres outside the map are evaluated like any other
    c[4, 17] = (Hg + 30, -2)
    c[6, 2] = (0, Wg - 1)
    return c.astype(np.int32)


@pytest.mark.parametrize("Hg,Wg,N", [(8, 4, 5), (128, 64, 5)])
def test_pose_batch_equals_pose_maps_then_flip(dev, Hg, Wg, N):
    from rg_hip import ops
    from reid.utils.data.device_pipeline import flip_images
    centres, idx = _centres(Hg, Wg), [5, 0, 3, 3, 4, 2, 6][:N]
    flips = [1, 0, 1, 0, 1, 1, 0][:N]
    table = torch.from_numpy(centres).to(dev)
    got = ops.bank_pose_batch(table, ops.bank_draws(idx, [(f, 0, 0, 0, 0, 0, 0) for f in flips]), Hg, Wg, 6.0)
    assert tuple(got.shape) == (N, 18, Hg, Wg)
    gathered = table[torch.tensor(idx, device=dev)].contiguous()
    want = flip_images(ops.pose_maps(gathered, torch.full((N,), 6.0, dtype=torch.float32).to(dev), Hg, Wg, mode=1), flips)
    assert _bytes(got) == _bytes(want)
    assert float(got[0].abs().max()) == 0.0 and float(got[1, 3].abs().max()) == 0.0 and float(got[1, 4].max()) == 1.0


def test_outputs_are_reproducible_and_stream_independent(dev, luts):
    from rg_hip import ops
    Hs, Ws, pad, H, W = GEOMETRIES["real"]
    planes, idx, draws, ref = _reid_case("real", 3)
    bank = torch.from_numpy(planes).to(dev)
    d = ops.bank_draws(idx, draws, device=dev)
    table = torch.from_numpy(_centres(H, W)).to(dev)

    def run():
        return (ops.bank_reid_batch(bank, d, luts[0], luts[2], (H, W), pad), ops.bank_gan_batch(bank, d, luts[1]),
                ops.bank_pose_batch(table, d, H, W, 6.0))
    first = [_bytes(t) for t in run()]
    assert first[0] == ref.tobytes()
    assert [_bytes(t) for t in run()] == first
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = run()
    side.synchronize()
    assert [_bytes(t) for t in out] == first


def _small_bank(dev, Hs=64, Ws=32, poses=True, n=12):
    from clustercontrast.utils.data.device_bank import DeviceImageBank
    g = np.random.RandomState(7)
    fnames = ["%04d_c%ds1_%06d.jpg" % (m // 2 + 1, m % 3 + 1, m) for m in range(n)]
    cords = g.randint(0, 64, size=(n, 18, 2))
    cords[1, 4] = -1
    return DeviceImageBank.from_arrays(g.randint(0, 256, size=(n, Hs, Ws, 3)).astype(np.uint8), fnames, [m // 2 + 1 for m in range(n)],
                                       [m % 3 for m in range(n)], gan_u8=g.randint(0, 256, size=(n, Hs, Ws, 3)).astype(np.uint8),
                                       cords=cords if poses else None, old_sizes=np.tile(np.array([[64, 64]]), (n, 1)), device=dev)


def _count_all(monkeypatch):
    """{entry point: [argument tuple of every call]} over EVERY prototype of the library"""
    from rg_hip.lib import lib
    from tests.test_mp_models_gpu import _wrap
    lib.load()
    return _wrap(monkeypatch, lib, [n for n in lib.protos if n not in ("rg_last_error",)])


def test_launch_accounting(dev, monkeypatch):
    """at the rg_hip.lib boundary: a plain next() is ONE library call, a with_gan next() on a bank with poses THREE"""
    from clustercontrast.utils.data.device_bank import DeviceGanLoader, DeviceTestLoader, DeviceTrainLoader
    bank = _small_bank(dev)
    trainset = [(f, 3 + m % 4, c) for m, (f, c) in enumerate(zip(bank.fnames, bank.camids))]
    plain = DeviceTrainLoader(bank, trainset, 8, padding=4)
    both = DeviceTrainLoader(bank, trainset, 8, padding=4, with_gan=True)
    calls = _count_all(monkeypatch)
    plain.next()
    n = {k: len(v) for k, v in calls.items() if v}
    assert n == {"rg_bank_reid_batch": 1}, n
    for v in calls.values():
        del v[:]
    both.next()
    n = {k: len(v) for k, v in calls.items() if v}
    assert n == {"rg_bank_reid_batch": 1, "rg_bank_gan_batch": 1, "rg_bank_pose_batch": 1}, n
    for v in calls.values():
        del v[:]
    assert len(list(DeviceTestLoader(bank, trainset, 5))) == 3 and len(list(DeviceGanLoader(bank, trainset, 6))) == 2
    n = {k: len(v) for k, v in calls.items() if v}
    assert n == {"rg_bank_reid_batch": 3, "rg_bank_gan_batch": 2, "rg_bank_pose_batch": 2}, n


def test_allocation_bound(dev):
    """the device memory a next() takes is the returned tensors plus the packed draws and labels: no fp32 intermediate batch"""
    from clustercontrast.utils.data.device_bank import DeviceTrainLoader
    bank = _small_bank(dev)
    trainset = [(f, 3 + m % 4, c) for m, (f, c) in enumerate(zip(bank.fnames, bank.camids))]
    N = 4                                                        # every tensor below 1 MiB: the allocator splits its blocks exactly
    loader = DeviceTrainLoader(bank, trainset, N, padding=4, with_gan=True)
    out = loader.next()                                          # tables uploaded, library loaded
    del out
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    reid, gan = loader.next()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base

    def block(nbytes):                                           # the caching allocator hands out multiples of 512 bytes
        return -(-nbytes // 512) * 512
    returned = sum(block(t.numel() * 4) for t in (reid[0], gan["Xs"], gan["Ps"]))
    small = block(9 * N * 4) + block(4 * N * 8)                  # int32 [9 N] draws + indices, int64 [4, N] labels
    print("next(): peak %d bytes over the baseline; returned %d, parameters %d" % (peak, returned, small))
    assert peak <= returned + small
    assert reid[0].numel() * 4 > small                           # an fp32 intermediate batch would not fit under the bound


def test_bad_draws_never_reach_the_device(dev, luts, monkeypatch):
    from rg_hip import ops
    Hs, Ws, pad, H, W = GEOMETRIES["vec"]
    bank = torch.from_numpy(_planes(Hs, Ws)).to(dev)
    table = torch.from_numpy(_centres(8, 4)).to(dev)
    calls = _count_all(monkeypatch)
    good = (1, 4, 0, 2, 1, 3, 2)
    for idx, row in [(7, good), (-1, good), (0, (1, 5, 0, 0, 0, 0, 0)), (0, (1, 0, 5, 0, 0, 0, 0)), (0, (1, 0, 0, 14, 0, 3, 2)),
                     (0, (1, 0, 0, 0, 7, 3, 2)), (0, (2, 0, 0, 0, 0, 0, 0)), (0, (0, -1, 0, 0, 0, 0, 0))]:
        with pytest.raises(ValueError):
            ops.bank_reid_batch(bank, ops.bank_draws([0, idx], [good, row]), luts[0], luts[2], (H, W), pad)
    for idx in (7, -1):
        with pytest.raises(ValueError):
            ops.bank_gan_batch(bank, ops.bank_draws([idx], None), luts[1])
        with pytest.raises(ValueError):
            ops.bank_pose_batch(table, ops.bank_draws([idx], None), 8, 4)
    with pytest.raises(ValueError):
        ops.bank_reid_batch(bank, ops.bank_draws([0], None), luts[0], luts[2], (H + 2 * pad + 1, W), pad)
    with pytest.raises(TypeError):
        ops.bank_reid_batch(bank, (torch.zeros(1, dtype=torch.int32, device=dev), None), luts[0], luts[2], (H, W), pad)
    assert not any(calls.values()), {k: len(v) for k, v in calls.items() if v}


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_trainer_step_fed_by_the_train_loader(dev):
    """one ClusterContrastTrainer.step on a DeviceTrainLoader batch == the same step on the host model's batch: byte-equal losses"""
    from clustercontrast.trainers import ClusterContrastTrainer
    from clustercontrast.utils.data.device_bank import DeviceTrainLoader
    from tests.test_paths_gpu import _cc_parts
    B, pad = 8, 4
    bank = _small_bank(dev, poses=False)
    trainset = [(f, (5 * m) % 9, c) for m, (f, c) in enumerate(zip(bank.fnames, bank.camids))]
    drawn = []

    def draws(indices):
        drawn.append((list(indices), _corner_draws(len(indices), 64, 32, pad, 64, 32)))
        return drawn[-1][1]
    loader = DeviceTrainLoader(bank, trainset, B, padding=pad, draws=draws, generator=torch.Generator().manual_seed(1))
    losses = []
    for source in ("bank", "host"):
        enc, mem, opt, _, _, _ = _cc_parts(dev, B)
        trainer = ClusterContrastTrainer(enc, mem)
        enc.train()
        if source == "bank":
            batch = loader.next()
            imgs, labels, indexes = trainer._parse_data(batch)
            assert imgs.data_ptr() == batch[0].data_ptr() and labels.data_ptr() == batch[2].data_ptr()      # .to(dev): no copy
        else:
            indices, params = drawn[0]
            rows = [bank.row[trainset[i][0]] for i in indices]
            ref = HM.reid_batch_model(bank.reid.cpu().numpy(), rows, params, HM.bank_lut(HM.REID_MEAN, HM.REID_STD),
                                      np.asarray(HM.REID_MEAN, np.float32), 64, 32, pad)
            assert _bytes(batch[0]) == ref.tobytes()
            host = [torch.from_numpy(ref), [trainset[i][0] for i in indices], torch.tensor([trainset[i][1] for i in indices]),
                    torch.tensor([trainset[i][2] for i in indices]), torch.tensor(indices)]
            assert host[1] == batch[1] and all(torch.equal(h, b.cpu()) for h, b in zip(host[2:], batch[2:]))
            imgs, labels, indexes = trainer._parse_data(host)
        losses.append(trainer.step(imgs, labels, opt))
    print("losses", [float(v) for v in losses])
    assert _bytes(losses[0]) == _bytes(losses[1]) and np.isfinite(float(losses[0]))


def test_extract_features_over_the_test_loader(dev):
    from clustercontrast.evaluators import extract_features_device
    from clustercontrast.utils.data.device_bank import DeviceTestLoader
    from tests.test_paths_gpu import _cc_parts
    bank = _small_bank(dev, poses=False)
    testset = [(bank.fnames[m], bank.pids[m], bank.camids[m]) for m in (9, 0, 4, 11, 2, 7, 7 - 6, 3, 10, 5)]
    enc = _cc_parts(dev, 4)[0]
    feats, labels = extract_features_device(enc, DeviceTestLoader(bank, testset, 4))
    rows = [bank.row[f] for f, _, _ in testset]
    ref = HM.reid_batch_model(bank.reid.cpu().numpy(), rows, np.zeros((10, 8), np.int64), HM.bank_lut(HM.REID_MEAN, HM.REID_STD),
                              np.zeros(3, np.float32), 64, 32, 0)
    host = [(torch.from_numpy(ref[s:s + 4]), [t[0] for t in testset[s:s + 4]], torch.tensor([t[1] for t in testset[s:s + 4]]),
             torch.tensor([t[2] for t in testset[s:s + 4]]), torch.arange(s, min(s + 4, 10))) for s in (0, 4, 8)]
    want, want_labels = extract_features_device(enc, host)
    assert feats.matrix.shape[0] == 10 and list(feats.index) == [t[0] for t in testset] == list(want.index)
    assert _bytes(feats.matrix) == _bytes(want.matrix)
    assert [int(labels[f]) for f in feats.index] == [int(want_labels[f]) for f in want.index] == [t[1] for t in testset]


def test_train_all_consumes_a_with_gan_batch(dev, capsys):
    """one `train_all` iteration on a with_gan batch; the GAN's set_input keeps the loader's device tensors as they are"""
    from clustercontrast.trainers import ClusterContrastWithGANTrainer
    from clustercontrast.utils.data.device_bank import DeviceTrainLoader
    from dual_gan.models.models import create_model
    from tests.test_dualgan_gpu import _gan_opt
    from tests.test_paths_gpu import _cc_parts
    B = 4
    bank = _small_bank(dev)
    trainset = [(f, (5 * m) % 9, c) for m, (f, c) in enumerate(zip(bank.fnames, bank.camids))]
    loader = DeviceTrainLoader(bank, trainset, B, padding=4, with_gan=True, generator=torch.Generator().manual_seed(2), length=1)
    seen = []
    inner = loader.next
    loader.next = lambda: seen.append(inner()) or seen[-1]
    enc, mem, opt, _, _, _ = _cc_parts(dev, B)
    torch.manual_seed(1)
    gan = create_model(_gan_opt(model="AE", num_feats=256))
    trainer = ClusterContrastWithGANTrainer(enc, GAN=gan, memory=mem)
    trainer.sync_every_step = True
    trainer.train_all(0, loader, opt, print_freq=1, train_iters=1, joint=False)
    out = capsys.readouterr().out
    assert out.count("Epoch: [0][1/1]") == 1 and len(seen) == 1
    reid, gd = seen[0]
    assert sorted(gd) == ["Ps", "Xs", "Xs_path", "gt_label"]
    assert tuple(gd["Xs"].shape) == (B, 3, 64, 32) and tuple(gd["Ps"].shape) == (B, 18, 64, 32) and gd["Xs"].is_cuda
    assert gan.input is gd and gan.source_image.data_ptr() == gd["Xs"].data_ptr() and gan.source_pose.data_ptr() == gd["Ps"].data_ptr()
    assert gd["gt_label"].dtype == torch.int64 and gd["gt_label"].is_cuda
