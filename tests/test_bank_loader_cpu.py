"""The host side of the device image bank without a GPU: the pose CSV parser, the structure of what the three loaders yield (with
the three launches replaced by the host model on CPU tensors), the host check that refuses every out-of-range draw, and the
identity samplers against index lists recorded from the reference's sampler.py (tests/golden/reference_bank.npz)."""
import os
import random
import types

import numpy as np
import pytest
import torch

from rg_hip import ops
from tests import bank_hostmodel as HM
from tests.golden import cases_bank as C

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_bank.npz"))
HS, WS, HG, WG, PAD = 12, 6, 6, 4, 2


# ---- the CSV parser -----------------------------------------------------------------------------------------------------------
def test_read_pose_csv(tmp_path):
    from clustercontrast.utils.data.device_bank import read_pose_csv
    path = str(tmp_path / "pose.csv")
    rows = {"0002_c1s1_000451_03.jpg": ([10, -1, 30, 127], [5, -1, 63, 0]),
            "0007_c3s2_000001_00.jpg": ([-1, -1, -1, -1], [-1, -1, -1, -1])}
    with open(path, "w") as f:
        f.write("name:keypoints_y:keypoints_x\n")
        for name, (ys, xs) in rows.items():
            f.write("%s: %s: %s\n" % (name, ys, xs))                  # the reference's writer leaves a space after each ':'
    got = read_pose_csv(path)
    assert sorted(got) == sorted(rows)
    for name, (ys, xs) in rows.items():
        assert got[name].shape == (4, 2) and got[name][:, 0].tolist() == ys and got[name][:, 1].tolist() == xs
    with open(path, "w") as f:
        f.write("file:keypoints_y:keypoints_x\n")
    with pytest.raises(ValueError):
        read_pose_csv(path)


# ---- loader structure ---------------------------------------------------------------------------------------------------------
def _fake_ops(calls):
    """rg_hip.ops with the three launches replaced by the host model on CPU tensors (the draws are checked as the wrappers do)"""
    def reid(bank_u8, draws, lut, fill, out_hw, pad=0):
        calls.append("reid")
        draws.check("bank_reid_batch", bank_u8.shape[0], (bank_u8.shape[1], bank_u8.shape[2], out_hw[0], out_hw[1], pad))
        return torch.from_numpy(HM.reid_batch_model(bank_u8.numpy(), draws.idx.tolist(), draws.params.tolist(), lut.numpy(),
                                                    fill.numpy(), out_hw[0], out_hw[1], pad))

    def gan(bank_u8, draws, lut):
        calls.append("gan")
        draws.check("bank_gan_batch", bank_u8.shape[0])
        return torch.from_numpy(HM.gan_batch_model(bank_u8.numpy(), draws.idx.tolist(), draws.params[:, 0].tolist(), lut.numpy()))

    def pose(centres, draws, height, width, sigma=6.0):
        calls.append("pose")
        draws.check("bank_pose_batch", centres.shape[0])
        return torch.from_numpy(HM.pose_batch_model(centres.numpy(), draws.idx.tolist(), draws.params[:, 0].tolist(), sigma, height,
                                                    width))
    return types.SimpleNamespace(bank_lut=ops.bank_lut, bank_draws=ops.bank_draws, bank_reid_batch=reid, bank_gan_batch=gan,
                                 bank_pose_batch=pose)


@pytest.fixture(scope="module")
def bank():
    from clustercontrast.utils.data.device_bank import DeviceImageBank
    g = np.random.RandomState(2)
    M = 9
    fnames = ["%04d_c%ds1_%06d.jpg" % (m // 2 + 1, m % 3 + 1, m) for m in range(M)]
    cords = g.randint(0, 40, size=(M, 5, 2))
    cords[2, 1] = -1
    old = np.tile(np.array([[40, 40]]), (M, 1))
    return DeviceImageBank.from_arrays(g.randint(0, 256, size=(M, HS, WS, 3)).astype(np.uint8), fnames, [m // 2 + 1 for m in range(M)],
                                       [m % 3 for m in range(M)], gan_u8=g.randint(0, 256, size=(M, HG, WG, 3)).astype(np.uint8),
                                       cords=cords, old_sizes=old, device="cpu")


def _trainset(bank):
    """a pseudo-labelled SUBSET in another order than the bank's, with labels that are not the data set's identities"""
    keep = [7, 2, 5, 0, 8, 3, 1]
    return [(bank.fnames[m], 100 + k % 3, bank.camids[m]) for k, m in enumerate(keep)], keep


def test_bank_bookkeeping(bank):
    assert len(bank) == 9 and bank.row[bank.fnames[4]] == 4
    assert bank.reid_size == (HS, WS) and bank.gan_size == (HG, WG)
    assert bank.nbytes == 9 * (HS * WS * 3 + HG * WG * 3 + 5 * 2 * 4)
    assert bank.centres.dtype == torch.int32 and (bank.centres[2, 1] == HM.MISSING).all()
    from clustercontrast.utils.data.device_bank import DeviceImageBank, default_workers
    assert 1 <= default_workers() <= min(16, len(os.sched_getaffinity(0)))
    with pytest.raises(ValueError):
        DeviceImageBank.from_arrays(np.zeros((2, 4, 4, 3), np.uint8), ["a", "a"], [0, 0], [0, 0], device="cpu")
    with pytest.raises(ValueError):
        DeviceImageBank.from_arrays(np.zeros((2, 4, 4, 3), np.float32), ["a", "b"], [0, 0], [0, 0], device="cpu")


def test_train_loader_batches(bank):
    from clustercontrast.utils.data.device_bank import DeviceTrainLoader
    from clustercontrast.utils.data.device_transforms import RandomErasing
    trainset, keep = _trainset(bank)
    calls = []
    g = torch.Generator().manual_seed(3)
    random.seed(4)
    loader = DeviceTrainLoader(bank, trainset, 3, padding=PAD, generator=g, erasing=RandomErasing(1.0, mean=[0.485, 0.456, 0.406]),
                               ops=_fake_ops(calls))
    assert len(loader) == 2                                            # 7 entries, batches of 3, drop_last
    batches = list(loader)
    assert len(batches) == 2 and calls == ["reid", "reid"]
    seen = []
    for b in batches:
        assert isinstance(b, list) and len(b) == 5
        imgs, fnames, pids, camids, indexes = b
        assert imgs.dtype == torch.float32 and tuple(imgs.shape) == (3, 3, HS, WS)
        assert isinstance(fnames, list) and all(isinstance(f, str) for f in fnames)
        for t in (pids, camids, indexes):
            assert t.dtype == torch.int64 and tuple(t.shape) == (3,)
        for f, p, c, i in zip(fnames, pids.tolist(), camids.tolist(), indexes.tolist()):
            assert trainset[i] == (f, p, c)                            # the loader's labels, not the bank's identities
            assert p >= 100
        seen += indexes.tolist()
    assert len(set(seen)) == 6 and set(seen) <= set(range(7))          # a permutation's first six
    # not dropping the short batch; a fixed length
    loader = DeviceTrainLoader(bank, trainset, 3, padding=PAD, drop_last=False, length=11, ops=_fake_ops(calls))
    assert len(loader) == 11 and [b[0].shape[0] for b in loader] == [3, 3, 1]
    assert len(DeviceTrainLoader(bank, trainset, 3, padding=PAD, drop_last=False, ops=_fake_ops(calls))) == 3


def test_train_loader_next_and_new_epoch(bank):
    from clustercontrast.utils.data.device_bank import DeviceTrainLoader
    from clustercontrast.utils.data.device_sampler import RandomMultipleGallerySampler
    trainset, _ = _trainset(bank)
    order = [[4, 1, 0, 6, 2, 3, 5], [0, 1, 2, 3, 4, 5, 6]]

    class Fixed(object):
        def __init__(self):
            self.epochs = 0

        def __len__(self):
            return 7

        def __iter__(self):
            self.epochs += 1
            return iter(order[(self.epochs - 1) % 2])
    s = Fixed()
    loader = DeviceTrainLoader(bank, trainset, 2, sampler=s, padding=PAD, ops=_fake_ops([]))
    assert len(loader) == 3
    got = [loader.next()[4].tolist() for _ in range(4)]                # three batches, then the next epoch starts by itself
    assert got == [[4, 1], [0, 6], [2, 3], [0, 1]] and s.epochs == 2
    loader.new_epoch()
    assert loader.next()[4].tolist() == [4, 1] and s.epochs == 3
    # the reference's sampler, by this build's module: every drawn index is a clustered entry
    trainset[3] = (trainset[3][0], -1, trainset[3][2])
    loader = DeviceTrainLoader(bank, trainset, 4, sampler=RandomMultipleGallerySampler(trainset, 2), padding=PAD, ops=_fake_ops([]))
    pids = loader.next()[2]
    assert (pids >= 100).all()


def test_train_loader_draw_order_and_override(bank):
    """per sample in batch order: flip (torch generator), top, left (torch generator), rectangle (random)"""
    from clustercontrast.utils.data.device_bank import DeviceTrainLoader
    from clustercontrast.utils.data.device_transforms import PadRandomCropFlip, RandomErasing
    trainset, keep = _trainset(bank)
    er = RandomErasing(0.5, mean=[0.485, 0.456, 0.406])
    lut, fill = HM.bank_lut(HM.REID_MEAN, HM.REID_STD), np.asarray([0.485, 0.456, 0.406], dtype=np.float32)

    class InOrder(object):
        def __len__(self):
            return 7

        def __iter__(self):
            return iter(range(7))
    random.seed(9)
    loader = DeviceTrainLoader(bank, trainset, 7, sampler=InOrder(), padding=PAD, generator=torch.Generator().manual_seed(8),
                               erasing=er, ops=_fake_ops([]))
    imgs = loader.next()[0]
    random.seed(9)
    g = torch.Generator().manual_seed(8)
    crop = PadRandomCropFlip((HS, WS), PAD, 0.0, generator=g)
    want = []
    for _ in range(7):
        flip = 1 if float(torch.rand(1, generator=g)) < 0.5 else 0
        _, top, left = crop.draw(HS, WS)
        want.append((flip, top, left) + er.draw(3, HS, WS))
    assert len(set(w[0] for w in want)) == 2 and any(w[5] for w in want)
    ref = HM.reid_batch_model(bank.reid.numpy(), keep, want, lut, fill, HS, WS, PAD)
    assert imgs.numpy().tobytes() == ref.tobytes()
    # draws= replaces them
    fixed = [(1, 4, 0, 1, 1, 3, 2)] * 7
    loader = DeviceTrainLoader(bank, trainset, 7, sampler=InOrder(), padding=PAD, draws=lambda indices: fixed, ops=_fake_ops([]))
    assert loader.next()[0].numpy().tobytes() == HM.reid_batch_model(bank.reid.numpy(), keep, fixed, lut, fill, HS, WS, PAD).tobytes()
    # flip_all=False, erasing=None: only the crop offsets are drawn
    loader = DeviceTrainLoader(bank, trainset, 7, sampler=InOrder(), padding=PAD, flip_all=False, erasing=None,
                               generator=torch.Generator().manual_seed(8), ops=_fake_ops([]))
    g = torch.Generator().manual_seed(8)
    crop = PadRandomCropFlip((HS, WS), PAD, 0.0, generator=g)
    want = [(0,) + crop.draw(HS, WS)[1:] + (0, 0, 0, 0) for _ in range(7)]
    assert loader.next()[0].numpy().tobytes() == HM.reid_batch_model(bank.reid.numpy(), keep, want, lut, fill, HS, WS, PAD).tobytes()


def test_train_loader_with_gan(bank):
    from clustercontrast.utils.data.device_bank import DeviceTrainLoader, DeviceImageBank
    trainset, keep = _trainset(bank)
    calls = []
    fixed = [(k % 2, 0, 0, 0, 0, 0, 0) for k in range(4)]
    loader = DeviceTrainLoader(bank, trainset, 4, padding=PAD, with_gan=True, draws=lambda indices: fixed, ops=_fake_ops(calls))
    out = loader.next()
    assert isinstance(out, tuple) and len(out) == 2 and calls == ["reid", "gan", "pose"]
    reid, gan = out
    assert isinstance(reid, list) and len(reid) == 5 and sorted(gan) == ["Ps", "Xs", "Xs_path", "gt_label"]
    idx = reid[4].tolist()
    rows = [keep[i] for i in idx]
    assert gan["Xs"].dtype == torch.float32 and tuple(gan["Xs"].shape) == (4, 3, HG, WG)
    assert gan["Ps"].dtype == torch.float32 and tuple(gan["Ps"].shape) == (4, 5, HG, WG)
    assert gan["Xs_path"] == [bank.fnames[m] for m in rows]
    assert gan["gt_label"].dtype == torch.int64 and gan["gt_label"].tolist() == [m // 2 + 1 for m in rows]   # from the file name
    assert reid[2].tolist() == [trainset[i][1] for i in idx]
    flips = [f[0] for f in fixed]
    assert gan["Xs"].numpy().tobytes() == HM.gan_batch_model(bank.gan.numpy(), rows, flips, HM.bank_lut(HM.GAN_MEAN, HM.GAN_STD)).tobytes()
    assert gan["Ps"].numpy().tobytes() == HM.pose_batch_model(bank.centres.numpy(), rows, flips, 6.0, HG, WG).tobytes()
    # a bank without poses: no 'Ps', two launches; a bank without GAN planes refuses with_gan
    calls[:] = []
    plain = DeviceImageBank(bank.reid, bank.gan, None, bank.fnames, bank.pids, bank.camids, None)
    out = DeviceTrainLoader(plain, trainset, 4, padding=PAD, with_gan=True, ops=_fake_ops(calls)).next()
    assert sorted(out[1]) == ["Xs", "Xs_path", "gt_label"] and calls == ["reid", "gan"]
    with pytest.raises(ValueError):
        DeviceTrainLoader(DeviceImageBank(bank.reid, None, None, bank.fnames, bank.pids, bank.camids, None), trainset, 4,
                          with_gan=True, ops=_fake_ops(calls))
    with pytest.raises(KeyError):
        DeviceTrainLoader(bank, [("no_such_file.jpg", 0, 0)], 1, ops=_fake_ops(calls))


def test_test_and_gan_loaders(bank):
    from clustercontrast.utils.data.device_bank import DeviceGanLoader, DeviceTestLoader
    testset = [(bank.fnames[m], bank.pids[m], bank.camids[m]) for m in (6, 1, 4, 4 + 4, 0)]
    rows = [6, 1, 4, 8, 0]
    calls = []
    loader = DeviceTestLoader(bank, testset, 2, ops=_fake_ops(calls))
    assert len(loader) == 3
    batches = list(loader)
    assert [b[0].shape[0] for b in batches] == [2, 2, 1] and calls == ["reid"] * 3
    lut = HM.bank_lut(HM.REID_MEAN, HM.REID_STD)
    ref = HM.reid_batch_model(bank.reid.numpy(), rows, np.zeros((5, 8), np.int64), lut, np.zeros(3, np.float32), HS, WS, 0)
    assert isinstance(batches[0], tuple) and len(batches[0]) == 5
    assert torch.cat([b[0] for b in batches]).numpy().tobytes() == ref.tobytes()
    assert sum((b[1] for b in batches), []) == [t[0] for t in testset]
    assert torch.cat([b[2] for b in batches]).tolist() == [t[1] for t in testset]
    assert torch.cat([b[3] for b in batches]).tolist() == [t[2] for t in testset]
    assert torch.cat([b[4] for b in batches]).tolist() == list(range(5))
    assert all(b[k].dtype == torch.int64 for b in batches for k in (2, 3, 4))
    calls[:] = []
    gl = list(DeviceGanLoader(bank, testset, 3, ops=_fake_ops(calls)))
    assert len(gl) == 2 and calls == ["gan", "pose", "gan", "pose"]
    d, pid, index = gl[1]
    assert sorted(d) == ["Ps", "Xs", "Xs_path", "gt_label"] and pid.tolist() == [testset[3][1], testset[4][1]] and index.tolist() == [3, 4]
    assert torch.cat([b[0]["Xs"] for b in gl]).numpy().tobytes() == \
        HM.gan_batch_model(bank.gan.numpy(), rows, [0] * 5, HM.bank_lut(HM.GAN_MEAN, HM.GAN_STD)).tobytes()


# ---- the host check -----------------------------------------------------------------------------------------------------------
GEOM = (HS, WS, HS, WS, PAD)         # top, left in [0, 4]; rectangles inside 12 x 6
GOOD = (1, 4, 0, 2, 1, 10, 5)


def test_good_draws_pass():
    d = ops.bank_draws([0, 6, 3], [GOOD, (0, 0, 4, 0, 0, 0, 0), (0, 2, 2, 11, 5, 1, 1)])
    d.check("t", 7, GEOM)
    assert d.idx.dtype == torch.int32 and d.params.dtype == torch.int32 and tuple(d.params.shape) == (3, 8)
    assert d.host.numel() == 27 and d.params[:, 7].tolist() == [0, 0, 0]          # ONE buffer: params, then idx
    assert d.host[24:].tolist() == [0, 6, 3]


@pytest.mark.parametrize("idx,row", [
    (-1, GOOD), (7, GOOD), (2 ** 31 + 1, GOOD),
    (0, (2, 4, 0, 2, 1, 10, 5)), (0, (-1, 4, 0, 2, 1, 10, 5)),                      # flip
    (0, (1, 5, 0, 0, 0, 0, 0)), (0, (1, -1, 0, 0, 0, 0, 0)),                        # top
    (0, (1, 0, 5, 0, 0, 0, 0)), (0, (1, 0, -1, 0, 0, 0, 0)),                        # left
    (0, (1, 0, 0, -1, 0, 2, 2)), (0, (1, 0, 0, 0, -1, 2, 2)),                       # rectangle origin
    (0, (1, 0, 0, 3, 0, 10, 2)), (0, (1, 0, 0, 0, 2, 2, 5)),                        # rectangle past the far edges
    (0, (1, 0, 0, 0, 0, -2, 2)), (0, (1, 0, 0, 0, 0, 2, -2)), (0, (1, 0, 0, 0, 0, 2, 0)),
    (0, (1, 0, 0, 2 ** 31 - 1, 0, 2, 2)),                                           # would wrap in int32 arithmetic
])
def test_bad_draws_raise_value_error(idx, row):
    with pytest.raises(ValueError):
        d = ops.bank_draws([0, idx, 1], [GOOD, row, GOOD])
        d.check("t", 7, GEOM)


def test_bad_draw_is_refused_through_the_loader(bank):
    from clustercontrast.utils.data.device_bank import DeviceTrainLoader
    trainset, _ = _trainset(bank)
    calls = []
    loader = DeviceTrainLoader(bank, trainset, 2, padding=PAD, draws=lambda i: [(0, 5, 0, 0, 0, 0, 0)] * 2, ops=_fake_ops(calls))
    with pytest.raises(ValueError):
        loader.next()
    for bad in (torch.zeros(2, 3), torch.zeros(2, 8, dtype=torch.float32)):
        with pytest.raises(ValueError):
            ops.bank_draws([0, 1], bad)
    with pytest.raises(ValueError):
        ops.bank_draws([], None)


# ---- the samplers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", C.SAMPLERS)
@pytest.mark.parametrize("name", list(C.CASES))
def test_sampler_draws_the_reference_index_list(name, sampler):
    from clustercontrast.utils.data import device_sampler as S
    entries = C.make_entries(name)
    assert any(p < 0 for _, p, _ in entries)
    s = getattr(S, sampler)(entries, C.NUM_INSTANCES)
    assert len(s) == int(GOLD["%s_%s_len" % (name, sampler)])
    C.seed_all(name)
    for epoch in range(2):
        got, ref = list(s), GOLD[C.key(name, sampler, epoch)].tolist()
        assert got == ref, "%s %s epoch %d" % (name, sampler, epoch)
        assert all(entries[i][1] >= 0 for i in got)


def test_sampler_module_does_not_shadow_the_reference_module_name():
    import clustercontrast.utils.data as D
    here = os.path.dirname(os.path.abspath(D.__file__))
    assert os.path.isfile(os.path.join(here, "device_sampler.py")) and not os.path.exists(os.path.join(here, "sampler.py"))
    assert not os.path.exists(os.path.join(here, "preprocessor.py"))
