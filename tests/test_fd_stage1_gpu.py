"""FD-GAN stage I's loader on the MI355X (csrc/databank.hip: rg_bank_fd_crop_batch):

  * the kernel byte for byte against tests/fd_stage1_hostmodel.py (itself held to PIL by tests/test_fd_stage1_cpu.py), written
    between two guard samples, at the smallest shapes that reach every branch: up- and down-sampling from odd sizes at misaligned
    bank offsets, the recipe (128x64 -> 256x128, four strips of columns), 513x257 -> 256x128 (7 taps), 700x40 -> 256x128 (the
    strip width set by the LDS tile, a narrower last strip) and 64x32 -> 16x8 (ratio 4), with the draws planted at their edges;
  * both regimes visited, byte-equal repeats and side-stream runs, the host check in front of the launch, launch accounting and the
    allocation bound of a loader batch;
  * DeviceStage1Loader against the reference's own items (tests/golden/reference_fdstage1.npz) and against the host model under the
    same seeds, and one SiameseTrainer.step fed by it.
"""
import os
import random

import numpy as np
import pytest
import torch

from tests import fd_stage1_hostmodel as HM
from tests.golden import cases_fdstage1 as C

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_fdstage1.npz"))
LUT = HM.bank_lut(HM.REID_MEAN, HM.REID_STD)


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


def _image(h, w, k):
    """uint8 [h, w, 3]: tells images, channels, rows and columns apart; image 1 is two-level noise"""
    r, q, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    a = (53 * k + 37 * r + 11 * q + 101 * c + (r * q) % 7 + np.random.RandomState(k).randint(0, 30, size=r.shape)) % 256
    if k == 1:
        a = np.where(a > 127, 255, 0)
    return a.astype(np.uint8)


def _planted(sizes, H, W, N):
    """[N][11] draws (row, x1, y1, w, h, flip, er0, ec0, eh, ew, rgb): boxes that end on the right / lower edge, 1-pixel boxes,
    whole images, a box of the output's own size where one fits; both flips; patches cut by each edge, an empty one, one pixel;
    colours 0, 0xFFFFFF and three distinct bytes"""
    h2, w2 = max(H // 3, 1), max(W // 3, 1)
    rects = [(0, 0, h2, w2), (1, W - w2, h2, w2), (H - h2, 1, h2, w2), (H // 2, W // 2, 1, 1), (2, 0, h2, W), (0, 0, 0, 0),
             (H - 1, W - 1, 1, 1), (0, 3, H, 1)]
    colours = [0x030201, 0, 0xFFFFFF, 0x10F080]
    out = []
    for n in range(N):
        m = n % len(sizes)
        hs, ws = sizes[m]
        boxes = [(ws - max(ws // 2, 1), 0, max(ws // 2, 1), hs - 1 if hs > 1 else 1), (0, hs - max(hs // 3, 1), ws, max(hs // 3, 1)),
                 (ws - 1, hs - 1, 1, 1), (0, 0, ws, hs), (ws // 3, hs // 4, 1, max(hs // 2, 1)), (0, hs // 2, max(ws - 1, 1), 1),
                 (1 if ws > 2 else 0, 1 if hs > 2 else 0, max(ws - 2, 1), max(hs - 2, 1))]
        if hs >= H and ws >= W:
            boxes.append((ws - W, hs - H, W, H))                      # the identity: both passes copy
        out.append((m,) + boxes[(n // len(sizes)) % len(boxes)] + ((n + n // 3) % 2,) + rects[n % len(rects)] + (colours[n % 4],))
    return out


# name -> (image sizes (h, w), output (H, W), N)
CASES = {"odd16x8": ([(12, 6), (33, 17), (12, 6), (33, 17), (33, 17)], (16, 8), 40),
         "recipe": ([(128, 64)] * 3, (256, 128), 5),
         "strips513": ([(513, 257), (128, 64)], (256, 128), 8),
         "tall700": ([(700, 40)], (256, 128), 2),
         "ratio4": ([(64, 32)] * 2, (16, 8), 14)}
_CACHE = {}


def _case(name):
    """(images, draws, host-model batch), computed once per case and left unchanged"""
    if name not in _CACHE:
        sizes, (H, W), N = CASES[name]
        images = [_image(h, w, k) for k, (h, w) in enumerate(sizes)]
        draws = _planted(sizes, H, W, N)
        ref = HM.fd_crop_model(images, [d[0] for d in draws], [d[1:] for d in draws], LUT, H, W)
        ref.setflags(write=False)
        _CACHE[name] = (images, draws, ref)
    return _CACHE[name]


def _bank(images, size, dev):
    from clustercontrast.utils.data.device_bank import DeviceRawBank
    M = len(images)
    return DeviceRawBank.from_arrays(images, ["%08d_00_%04d.jpg" % (k, k) for k in range(M)], list(range(M)), [0] * M, device=dev, size=size)


@pytest.fixture(scope="module")
def lut(dev):
    from rg_hip import ops
    t = ops.bank_lut(HM.REID_MEAN, HM.REID_STD)
    assert t.numpy().tobytes() == LUT.tobytes()
    return t.to(dev)


def _launch_guarded(bank, draws, lut):
    """the entry point itself, writing samples [1, N + 1) of an [N + 2] buffer of 0xFF bytes -> (batch, guard bytes untouched)"""
    from rg_hip import ops
    from rg_hip.lib import lib
    H, W = bank.size
    draws.check("test", bank.sizes_host, H, W)
    draws.to(bank.device)
    N = draws.host.shape[0]
    buf = torch.full((N + 2, 3, H, W), float("nan"), dtype=torch.float32, device=bank.device)
    buf.view(torch.int32).fill_(-1)
    tx, ty = bank.table_x, bank.table_y
    lib.rg_bank_fd_crop_batch(bank.data.data_ptr(), bank.offsets.data_ptr(), bank.sizes.data_ptr(), len(bank), tx.data_ptr(), tx.shape[2],
                              tx.shape[0] - 1, ty.data_ptr(), ty.shape[2], ty.shape[0] - 1, draws.dev.data_ptr(), lut.data_ptr(),
                              buf[1].data_ptr(), N, H, W, int(draws.host[:, 4].max()), ops._stream())
    torch.cuda.synchronize()
    guards = buf.view(torch.int32)[[0, N + 1]]
    return buf[1:N + 1], bool((guards == -1).all())


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_equals_the_host_model(dev, lut, name):
    from rg_hip import ops
    sizes, (H, W), N = CASES[name]
    images, draws, ref = _case(name)
    if N >= 14:                                                      # the planted edges are all there
        assert {d[5] for d in draws} == {0, 1} and any(d[9] == 0 for d in draws) and {0, 0xFFFFFF, 0x030201} <= {d[10] for d in draws}
        assert any(d[1] + d[3] == sizes[d[0]][1] and d[1] > 0 for d in draws) and any(d[2] + d[4] == sizes[d[0]][0] and d[2] > 0 for d in draws)
        assert any(d[3] == 1 and d[4] == 1 for d in draws) and any((d[4], d[3]) == sizes[d[0]] for d in draws)
        assert any(d[7] + d[9] == W and d[7] > 0 for d in draws) and any(d[6] + d[8] == H and d[6] > 0 for d in draws)
        assert any(d[6] == 0 and d[8] > 0 for d in draws) and any(d[7] == 0 and d[9] > 0 for d in draws)
    if name == "odd16x8":
        assert any((d[4], d[3]) == (H, W) for d in draws)            # a box of the output's size
    bank = _bank(images, (H, W), dev)
    assert name != "odd16x8" or any(int(o) % 4 for o in bank.offsets.tolist())      # images at misaligned offsets
    hmax = max(d[4] for d in draws)
    want = ops.FD_CROP_WHOLE if W == 8 else ops.FD_CROP_STRIPS
    assert ops.fd_crop_regime(hmax, W) == want
    # strips513: four strips of 32 columns; tall700: 699 rows leave 28 columns to the LDS tile, the fifth strip has 16
    assert ops.fd_crop_strip_width(hmax, W) == {"odd16x8": 8, "ratio4": 8, "recipe": 32, "strips513": 32, "tall700": 28}[name]
    got, guards_ok = _launch_guarded(bank, ops.fd_crop_draws([d for d in draws]), lut)
    assert guards_ok, "a guard sample was written"
    assert got.dtype == torch.float32 and tuple(got.shape) == (N, 3, H, W)
    wrong = int((got.cpu().numpy().view(np.uint32) != ref.view(np.uint32)).sum())
    print("%s N=%d: %d of %d elements differ from the host model" % (name, N, wrong, ref.size))
    assert wrong == 0
    assert _bytes(ops.bank_fd_crop_batch(bank, ops.fd_crop_draws([d for d in draws]), lut)) == ref.tobytes()       # the wrapper


def test_each_regime_is_visited():
    from rg_hip import ops
    seen = {ops.fd_crop_regime(max(d[4] for d in _case(name)[1]), CASES[name][1][1]) for name in CASES}
    assert seen == {ops.FD_CROP_WHOLE, ops.FD_CROP_STRIPS}


def test_outputs_are_reproducible_and_stream_independent(dev, lut):
    from rg_hip import ops
    for name in ("odd16x8", "strips513"):
        images, draws, ref = _case(name)
        bank = _bank(images, CASES[name][1], dev)
        d = ops.fd_crop_draws([r for r in draws], device=dev)
        first = _bytes(ops.bank_fd_crop_batch(bank, d, lut))
        assert first == ref.tobytes()
        assert _bytes(ops.bank_fd_crop_batch(bank, d, lut)) == first
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            out = ops.bank_fd_crop_batch(bank, d, lut)
        side.synchronize()
        assert _bytes(out) == first


def _count_all(monkeypatch):
    from rg_hip.lib import lib
    from tests.test_mp_models_gpu import _wrap
    lib.load()
    return _wrap(monkeypatch, lib, [n for n in lib.protos if n not in ("rg_last_error",)])


def test_bad_draws_never_reach_the_device(dev, lut, monkeypatch):
    from rg_hip import ops
    images, draws, _ = _case("odd16x8")
    bank = _bank(images, (16, 8), dev)
    calls = _count_all(monkeypatch)
    good = (1, 2, 3, 10, 20, 1, 2, 1, 3, 2, 0x123456)
    for row in [(5,) + good[1:], (-1,) + good[1:], (1, 8, 3, 10, 20) + good[5:], (1, 2, 14, 10, 20) + good[5:], (0, 0, 0, 7, 12) + good[5:],
                (1, 2, 3, 0, 20) + good[5:], (1, 2, 3, 10, 0) + good[5:], (1, -1, 3, 10, 20) + good[5:], good[:5] + (2,) + good[6:],
                good[:6] + (14, 1, 3, 2, 0), good[:6] + (2, 7, 3, 2, 0), good[:6] + (2, 1, 3, 0, 0), good[:10] + (2 ** 24,)]:
        with pytest.raises(ValueError):
            ops.bank_fd_crop_batch(bank, ops.fd_crop_draws([good, row]), lut)
    with pytest.raises(TypeError):
        ops.bank_fd_crop_batch(bank, ops.fd_draws([0]), lut)
    assert not any(v for k, v in calls.items() if k != "rg_bank_fd_crop_regime"), {k: len(v) for k, v in calls.items() if v}


# ---- the loader -----------------------------------------------------------------------------------------------------------------
def _toy_bank(dev, size=(C.H, C.W)):
    from clustercontrast.utils.data.device_bank import DeviceRawBank
    return DeviceRawBank.from_arrays([C.source_image(k) for k in range(len(C.SIZES))], C.NAMES, C.PIDS, C.CAMS, device=dev, size=size)


def test_stage1_loader_batches_equal_the_reference_items(dev):
    from reid.utils.data.device_stage1 import DeviceStage1Loader
    loader = DeviceStage1Loader(_toy_bank(dev), C.TRAIN, C.ITEM_PAIRS, neg_pos_ratio=C.RATIO)
    C.seed_sampler()
    C.seed_items()
    (imgs1, fnames1, pids1, camids1), (imgs2, fnames2, pids2, camids2) = next(iter(loader))
    assert random.random() == float(GOLD["item_probe"]) and float(torch.rand(1)) == float(GOLD["item_torch_probe"])
    pairs = GOLD["pairs"][:C.ITEM_PAIRS]
    assert imgs1.is_cuda and pids1.is_cuda and camids2.is_cuda and pids1.dtype == camids1.dtype == torch.int64
    assert imgs1.untyped_storage().data_ptr() == imgs2.untyped_storage().data_ptr()                  # one allocation
    for side, (imgs, names, pids, cams) in enumerate(((imgs1, fnames1, pids1, camids1), (imgs2, fnames2, pids2, camids2))):
        assert tuple(imgs.shape) == (C.ITEM_PAIRS, 3, C.H, C.W)
        for n in range(C.ITEM_PAIRS):
            a = imgs[n].cpu().numpy()
            assert C.byte_sum(a) == GOLD["item_sums"][n, side], (n, side)
            if n < C.ITEM_FULL:
                assert a.tobytes() == GOLD["item_%d_%d" % (n, side)].tobytes(), (n, side)
        assert names == [C.NAMES[i] for i in pairs[:, side]] and pids.tolist() == [C.PIDS[i] for i in pairs[:, side]]
        assert cams.tolist() == [C.CAMS[i] for i in pairs[:, side]]


def test_stage1_loader_epoch_equals_the_host_model_at_the_recipe_size(dev):
    """a whole epoch at 256x128 (the toy images up-sampled, the 150x70 ones resampled by odd ratios) under the same seeds"""
    from reid.utils.data.device_stage1 import DeviceStage1Loader
    H, W = 256, 128
    images = [C.source_image(k) for k in range(len(C.SIZES))]
    loader = DeviceStage1Loader(_toy_bank(dev, (H, W)), C.TRAIN, 8, neg_pos_ratio=C.RATIO)
    np.random.seed(5)
    random.seed(6)
    torch.manual_seed(7)
    batches = list(loader)
    assert [b[0][0].shape[0] for b in batches] == [8, 8, 4] and len(loader) == 3
    np.random.seed(5)
    random.seed(6)
    torch.manual_seed(7)
    pairs = HM.pair_list(C.TRAIN, C.RATIO)[1]
    for s, b in zip((0, 8, 16), batches):
        chunk = pairs[s:s + 8]
        draws = [[(i,) + HM.item_draw(images[i], H, W) for i in pair] for pair in chunk]
        for side in (0, 1):
            rows = [d[side] for d in draws]
            want = HM.fd_crop_model(images, [r[0] for r in rows], [r[1:] for r in rows], LUT, H, W)
            assert _bytes(b[side][0]) == want.tobytes(), (s, side)
            assert b[side][2].tolist() == [C.PIDS[p[side]] for p in chunk]


def test_launch_accounting_and_allocation_bound(dev, monkeypatch):
    """at the rg_hip.lib boundary a batch is ONE launch; the device memory it takes is its output plus the packed draws and the ids"""
    from reid.utils.data.device_stage1 import DeviceStage1Loader
    B = 2                                                        # every tensor below 1 MiB: the allocator splits its blocks exactly
    loader = DeviceStage1Loader(_toy_bank(dev), C.TRAIN, B, neg_pos_ratio=C.RATIO)
    it = iter(loader)
    out = next(it)                                               # table uploaded, library loaded
    del out
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    calls = _count_all(monkeypatch)
    b1, b2 = next(it)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    n = {k: len(v) for k, v in calls.items() if v and k != "rg_bank_fd_crop_regime"}
    assert n == {"rg_bank_fd_crop_batch": 1}, n

    def block(nbytes):                                           # the caching allocator hands out multiples of 512 bytes
        return -(-nbytes // 512) * 512
    returned = block(2 * B * 3 * C.H * C.W * 4)
    small = block(2 * B * 12 * 4) + block(2 * 2 * B * 8)         # int32 draws, int64 pids and camids
    print("batch: peak %d bytes over the baseline; returned %d, parameters %d" % (peak, returned, small))
    assert peak <= returned + small
    assert b1[0].numel() * 4 > small and b1[0].numel() > small      # neither an fp32 nor a uint8 intermediate batch would fit under the bound


def test_siamese_step_fed_by_the_stage1_loader(dev):
    import reid.models as RM
    from reid.models.embedding import EltwiseSubEmbed
    from reid.models.multi_branch import SiameseNet
    from reid.trainers import SiameseTrainer
    from reid.utils.data.device_stage1 import DeviceStage1Loader
    from torch import nn
    loader = DeviceStage1Loader(_toy_bank(dev), C.TRAIN, 4, neg_pos_ratio=C.RATIO)
    C.seed_sampler()
    C.seed_items()
    batch = next(iter(loader))
    torch.manual_seed(1)
    net = SiameseNet(RM.create('resnet18', pretrained=False, cut_at_pooling=True),
                     EltwiseSubEmbed(use_batch_norm=True, use_classifier=True, num_features=512, num_classes=2)).to(dev).train()
    opt = torch.optim.SGD(net.parameters(), 0.01, momentum=0.9, weight_decay=5e-4)
    trainer = SiameseTrainer(net, nn.CrossEntropyLoss())
    (imgs1, imgs2), targets = trainer._parse_data(batch)
    assert targets.tolist() == [1, 0, 1, 0] and imgs1.data_ptr() == batch[0][0].data_ptr()      # already on the device: no copy
    loss, prec = trainer.step(imgs1, imgs2, targets, opt)
    print("loss %.5f prec %.3f" % (float(loss), float(prec)))
    assert np.isfinite(float(loss)) and 0.0 <= float(prec) <= 1.0
