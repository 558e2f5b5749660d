"""FD-GAN stage I's loader without a GPU: the integer host model (tests/fd_stage1_hostmodel.py) against PIL itself, the
coefficient-table builder against the model, six planted defects, the crop's draws and whole loader batches against
tests/golden/reference_fdstage1.npz (the reference's own RandomSizedRectCrop, RandomSizedEarser and Preprocessor on the toy set of
tests/golden/cases_fdstage1.py) with the host model standing in for the launch, and the wrapper's host validation in front of a
recording stand-in for the library."""
import os
import random
import types

import numpy as np
import pytest
import torch
from PIL import Image

from rg_hip import ops
from tests import fd_stage1_hostmodel as HM
from tests.golden import cases_fdstage1 as C

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_fdstage1.npz"))
LUT = HM.bank_lut(HM.REID_MEAN, HM.REID_STD)
IMAGES = [C.source_image(k) for k in range(len(C.SIZES))]


def _pil(a, H, W):
    return np.asarray(Image.fromarray(a).resize((W, H), Image.BILINEAR), dtype=np.uint8)


def _pil_cases():
    """(source, box, output) cases: the named edges first, then seeded random ones, 320 in all"""
    g = np.random.RandomState(7)
    cases = []

    def add(hs, ws, box, H, W, two_level=False):
        a = g.randint(0, 256, size=(hs, ws, 3)).astype(np.uint8)
        if two_level:
            a = np.where(a > 127, 255, 0).astype(np.uint8)
        cases.append((a, box, H, W))
    add(40, 30, (0, 0, 30, 40), 40, 30)                    # crop equal to the output: both passes the identity
    add(40, 30, (3, 5, 20, 31), 31, 9)                     # the vertical axis equal
    add(40, 30, (3, 5, 20, 31), 50, 20)                    # the horizontal axis equal
    add(9, 9, (4, 4, 1, 1), 16, 8)                         # a 1x1 crop
    add(9, 9, (8, 0, 1, 9), 7, 5)                          # one pixel wide, at the right edge
    add(64, 32, (0, 0, 32, 64), 128, 64)                   # ksize 3 (up-sampling)
    add(130, 70, (0, 0, 70, 130), 70, 40)                  # ksize 5: ratios in (1, 2]
    add(200, 100, (0, 0, 100, 200), 70, 40)                # ksize 7: ratios in (2, 3]
    add(513, 257, (0, 0, 257, 513), 256, 128)              # ksize 7 at the size of the GPU test
    add(128, 64, (0, 0, 64, 128), 16, 8)                   # ksize 17: ratio 8
    add(120, 63, (0, 0, 63, 120), 16, 8)                   # ksize 17: ratios in (7, 8)
    add(128, 64, (9, 3, 46, 124), 256, 128)                # the recipe
    while len(cases) < 320:
        hs, ws = int(g.randint(1, 201)), int(g.randint(1, 121))
        H, W = int(g.randint(5, 65)), int(g.randint(5, 65))
        w, h = int(g.randint(1, ws + 1)), int(g.randint(1, hs + 1))
        if h > 8 * H or w > 8 * W:
            continue
        add(hs, ws, (int(g.randint(0, ws - w + 1)), int(g.randint(0, hs - h + 1)), w, h), H, W, two_level=len(cases) % 9 == 0)
    return cases


PIL_CASES = _pil_cases()


def test_the_model_equals_pil_byte_for_byte():
    ksizes = set()
    for a, (x1, y1, w, h), H, W in PIL_CASES:
        crop = Image.fromarray(a).crop((x1, y1, x1 + w, y1 + h))
        assert crop.size == (w, h)
        want = np.asarray(crop.resize((W, H), Image.BILINEAR), dtype=np.uint8)
        got = HM.resample(a[y1:y1 + h, x1:x1 + w], H, W)
        assert np.array_equal(got, want), (a.shape, (x1, y1, w, h), H, W, int((got != want).sum()))
        ksizes |= {2 * int(np.ceil(max(w / W, 1.0))) + 1, 2 * int(np.ceil(max(h / H, 1.0))) + 1}
    assert len(PIL_CASES) >= 300 and {3, 5, 7, 17} <= ksizes
    assert any(w == 1 and h == 1 for _, (_, _, w, h), _, _ in PIL_CASES)
    assert any((h, w) == (H, W) for _, (_, _, w, h), H, W in PIL_CASES)
    assert any(h == H and w != W for _, (_, _, w, h), H, W in PIL_CASES) and any(w == W and h != H for _, (_, _, w, h), H, W in PIL_CASES)


@pytest.mark.parametrize("m", [128, 256])
def test_the_table_builder_equals_the_model_for_every_input_length(m):
    from clustercontrast.utils.data.device_bank import pil_bilinear_table
    table = pil_bilinear_table(1024, m)
    assert table.dtype == np.int32 and table.shape[:2] == (1025, m) and not table[0].any()
    K = table.shape[2] - 2
    assert 3 <= K <= 2 * (1024 // m) + 1                     # the longest row: ratio 1024 / m
    for n in range(1, 1025):
        want = np.zeros((m, 2 + K), dtype=np.int64)
        for j, (lo, cnt, k) in enumerate(HM.coeffs(n, m)):
            want[j, 0], want[j, 1], want[j, 2:2 + cnt] = lo, cnt, k
        assert np.array_equal(table[n], want), n
    assert (table[1:, :, 0] + table[1:, :, 1] <= np.arange(1, 1025)[:, None]).all() and (table[1:, :, 1] >= 1).all()
    assert (table[:, :, 2:] >= 0).all()
    assert np.array_equal(table[m, :, :4], np.stack([np.arange(m), np.minimum(2, m - np.arange(m)), np.full(m, 1 << 22), np.zeros(m)], 1))
    with pytest.raises(ValueError):
        pil_bilinear_table(8 * m + 1, m)
    assert pil_bilinear_table(8 * m, m).shape[2] <= 2 + 17


@pytest.mark.parametrize("defect", ["vertical_first", "fp32_coeffs", "no_half", "round_bounds"])
def test_resampling_defects_are_told_apart_by_pil(defect):
    hit = 0
    for a, (x1, y1, w, h), H, W in PIL_CASES[:120]:
        hit += not np.array_equal(HM.resample(a[y1:y1 + h, x1:x1 + w], H, W, defect), _pil(a[y1:y1 + h, x1:x1 + w], H, W))
    print("%s: %d of 120 cases differ from PIL" % (defect, hit))
    assert hit >= 1


# ---- the reference's crops ------------------------------------------------------------------------------------------------------
def test_toy_images_are_the_recorded_ones():
    assert C.images_sum() == int(GOLD["images_sum"])


@pytest.mark.parametrize("name", sorted(C.BOXES))
def test_crop_draws_equal_the_reference_boxes(name):
    from reid.utils.data.device_stage1 import FDRandomSizedRectCrop
    hs, ws, draws, seed = C.BOXES[name]
    crop = FDRandomSizedRectCrop(256, 128)
    random.seed(seed)
    got = [crop.draw(ws, hs) for _ in range(draws)]
    assert random.random() == float(GOLD["boxes_%s_probe" % name])           # same consumption of the generator
    assert got == [tuple(b) for b in GOLD["boxes_" + name].tolist()] and len(got) == draws
    random.seed(seed)                                                          # and the host model's restatement
    assert [HM.crop_draw(ws, hs) for _ in range(draws)] == got
    whole = [b for b in got if b == (0, 0, ws, hs)]
    assert len(whole) == {"64x64": draws}.get(name, len(whole))               # 64x64: every box is at least 72 high
    assert all(0 <= x1 and 0 <= y1 and 1 <= w and 1 <= h and x1 + w <= ws and y1 + h <= hs for x1, y1, w, h in got)
    if name == "128x64":
        assert draws >= 200 and any(x1 + w == ws for x1, y1, w, h in got) and any(y1 + h == hs for x1, y1, w, h in got)


@pytest.mark.parametrize("name", sorted(C.CROPS))
def test_model_crops_equal_the_reference_outputs(name):
    k, H, W, draws, full, seed = C.CROPS[name]
    random.seed(seed)
    boxes = [HM.crop_draw(C.SIZES[k][1], C.SIZES[k][0]) for _ in range(draws)]
    assert random.random() == float(GOLD["crop_%s_probe" % name])
    assert boxes == [tuple(b) for b in GOLD["crop_%s_boxes" % name].tolist()]
    for n, box in enumerate(boxes):
        got = HM.crop_bytes(IMAGES[k], box + (0, 0, 0, 0, 0, 0), H, W)
        if n < full:
            assert np.array_equal(got, GOLD["crop_%s_%d" % (name, n)]), (name, n)
        assert C.byte_sum(got) == GOLD["crop_%s_sums" % name][n], (name, n)


# ---- whole items ----------------------------------------------------------------------------------------------------------------
def _same_items(items):
    """[(item of a, item of b)] per pair against the fixture: the stored ones bit for bit, all by their sums"""
    ok = []
    for n, pair in enumerate(items):
        for side, a in enumerate(pair):
            same = C.byte_sum(a) == GOLD["item_sums"][n, side]
            if n < C.ITEM_FULL:
                same = same and a.tobytes() == GOLD["item_%d_%d" % (n, side)].tobytes()
            ok.append(bool(same))
    return ok


def _model_items(defect=None):
    C.seed_items()
    items = [[HM.item(IMAGES, int(i), C.H, C.W, LUT, defect) for i in pair] for pair in GOLD["pairs"][:C.ITEM_PAIRS]]
    return items, random.random(), float(torch.rand(1))


def test_host_model_items_equal_the_reference():
    items, probe, tprobe = _model_items()
    assert all(_same_items(items)) and len(items) == C.ITEM_PAIRS
    assert probe == float(GOLD["item_probe"]) and tprobe == float(GOLD["item_torch_probe"])


@pytest.mark.parametrize("defect", ["erase_after_flip", "origin_ignored"] + ["vertical_first", "no_half"])
def test_item_defects_are_told_apart(defect):
    items, probe, _ = _model_items(defect)
    assert probe == float(GOLD["item_probe"])                           # the same draws ...
    assert not all(_same_items(items)), defect                          # ... another batch


def _fake_ops(calls):
    """rg_hip.ops with the launch replaced by the host model on CPU tensors; the draws are checked as the wrapper checks them"""
    def crop(raw, draws, lut):
        calls.append("crop")
        draws.check("bank_fd_crop_batch", raw.sizes_host, raw.size[0], raw.size[1])
        data, off = raw.data.numpy(), raw.offsets.tolist()
        images = [data[o:o + h * w * 3].reshape(h, w, 3) for o, (h, w) in zip(off, raw.sizes.tolist())]
        rows = draws.host[:, :11].tolist()
        return torch.from_numpy(HM.fd_crop_model(images, [r[0] for r in rows], [r[1:] for r in rows], lut.numpy(), raw.size[0],
                                                 raw.size[1]))
    return types.SimpleNamespace(bank_lut=ops.bank_lut, fd_crop_draws=ops.fd_crop_draws, bank_fd_crop_batch=crop)


def _cpu_bank(size=(C.H, C.W)):
    from clustercontrast.utils.data.device_bank import DeviceRawBank
    return DeviceRawBank.from_arrays(IMAGES, C.NAMES, C.PIDS, C.CAMS, device="cpu", size=size)


def test_raw_bank_layout():
    bank = _cpu_bank()
    assert len(bank) == 10 and bank.size == (C.H, C.W) and bank.row[C.NAMES[4]] == 4
    assert bank.data.dtype == torch.uint8 and bank.offsets.dtype == torch.int64 and bank.sizes.dtype == torch.int32
    assert bank.sizes.tolist() == [list(s) for s in C.SIZES] == bank.sizes_host.tolist()
    assert bank.data.numel() == sum(h * w * 3 for h, w in C.SIZES) and bank.offsets[0] == 0
    for k in (0, 3, 9):
        o, (h, w) = int(bank.offsets[k]), C.SIZES[k]
        assert np.array_equal(bank.data[o:o + h * w * 3].numpy().reshape(h, w, 3), IMAGES[k])
    assert tuple(bank.table_x.shape[:2]) == (71, C.W) and tuple(bank.table_y.shape[:2]) == (151, C.H)
    assert bank.nbytes == bank.data.numel() + 10 * 16 + 4 * (bank.table_x.numel() + bank.table_y.numel())


def test_stage1_loader_batches_equal_the_reference_items():
    from reid.utils.data.device_stage1 import DeviceStage1Loader
    calls = []
    loader = DeviceStage1Loader(_cpu_bank(), C.TRAIN, C.ITEM_PAIRS, neg_pos_ratio=C.RATIO, ops=_fake_ops(calls))
    assert len(loader) == -(-20 // C.ITEM_PAIRS)
    C.seed_sampler()
    C.seed_items()
    first = next(iter(loader))
    assert calls == ["crop"]
    assert random.random() == float(GOLD["item_probe"]) and float(torch.rand(1)) == float(GOLD["item_torch_probe"])
    (imgs1, fnames1, pids1, camids1), (imgs2, fnames2, pids2, camids2) = first
    pairs = GOLD["pairs"][:C.ITEM_PAIRS]
    assert tuple(imgs1.shape) == tuple(imgs2.shape) == (C.ITEM_PAIRS, 3, C.H, C.W) and imgs1.dtype == torch.float32
    assert imgs1.untyped_storage().data_ptr() == imgs2.untyped_storage().data_ptr()                  # one allocation
    assert all(_same_items([[imgs1[n].numpy(), imgs2[n].numpy()] for n in range(C.ITEM_PAIRS)]))
    for side, (names, pids, cams) in enumerate(((fnames1, pids1, camids1), (fnames2, pids2, camids2))):
        assert pids.dtype == cams.dtype == torch.int64
        assert names == [C.NAMES[i] for i in pairs[:, side]] and pids.tolist() == [C.PIDS[i] for i in pairs[:, side]]
        assert cams.tolist() == [C.CAMS[i] for i in pairs[:, side]]
    assert (pids1 == pids2).long().tolist() == [1, 0] * (C.ITEM_PAIRS // 2)        # ratio 1: a positive, then a negative


def test_stage1_loader_epochs_and_short_last_batch():
    from reid.utils.data.device_stage1 import DeviceStage1Loader
    loader = DeviceStage1Loader(_cpu_bank(), C.TRAIN, 8, neg_pos_ratio=C.RATIO, ops=_fake_ops([]))
    C.seed_sampler()
    random.seed(1)
    sizes, pids = [], [[], []]
    for b in loader:
        sizes.append(b[0][0].shape[0])
        for side in (0, 1):
            pids[side] += b[side][2].tolist()
    assert sizes == [8, 8, 4] and len(loader) == 3                          # the short last batch is kept
    assert pids[0] == [C.PIDS[a] for a in GOLD["pairs"][:, 0]] and pids[1] == [C.PIDS[b] for b in GOLD["pairs"][:, 1]]
    with pytest.raises(KeyError, match="nowhere.jpg"):
        DeviceStage1Loader(_cpu_bank(), C.TRAIN + [("nowhere.jpg", 2, 0)], 4, ops=_fake_ops([]))


def test_get_data_stage1_device(tmp_path):
    from reid.utils.data.device_pairs import DeviceFDTestLoader
    from reid.utils.data.device_stage1 import DeviceStage1Loader, get_data_stage1_device
    for k, name in enumerate(C.NAMES):
        Image.fromarray(IMAGES[k]).save(str(tmp_path / name), format="PNG")
    ds = types.SimpleNamespace(trainval=C.TRAIN[:8], train=C.TRAIN[:5], val=C.TRAIN[5:8], query=[C.TRAIN[8]],
                               gallery=[C.TRAIN[9], C.TRAIN[8]], images_dir=str(tmp_path))
    got, train, val, test = get_data_stage1_device(ds, C.H, C.W, 4, True, 1, workers=2, device="cpu")
    assert got is ds and isinstance(train, DeviceStage1Loader) and isinstance(val, DeviceFDTestLoader) and isinstance(test, DeviceFDTestLoader)
    assert len(train.bank) == 8 and train.bank.size == (C.H, C.W) and train.sampler.neg_pos_ratio == 1 and len(train) == 4
    assert train.bank.sizes_host.tolist() == [list(s) for s in C.SIZES[:8]]
    assert np.array_equal(train.bank.data[:128 * 64 * 3].numpy().reshape(128, 64, 3), IMAGES[0])
    assert val.bank is test.bank and len(val.bank) == 5 and len(val) == 1 and len(test) == 1
    assert np.array_equal(val.bank.reid[val.bank.row[C.NAMES[7]]].numpy(), _pil(IMAGES[7], C.H, C.W))       # RectScale's plane
    assert len(get_data_stage1_device(ds, C.H, C.W, 4, False, 1, workers=1, device="cpu")[1].bank) == 5


def test_an_over_large_image_is_refused_by_name():
    from clustercontrast.utils.data.device_bank import DeviceRawBank
    big = np.zeros((C.H * 8 + 1, 8, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="too_high.jpg"):
        DeviceRawBank.from_arrays([IMAGES[0], big], ["ok.jpg", "too_high.jpg"], [1, 2], [0, 0], device="cpu", size=(C.H, C.W))
    wide = np.zeros((8, C.W * 8 + 1, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="too_wide.jpg"):
        DeviceRawBank.from_arrays([wide], ["too_wide.jpg"], [1], [0], device="cpu", size=(C.H, C.W))
    DeviceRawBank.from_arrays([np.zeros((C.H * 8, C.W * 8, 3), dtype=np.uint8)], ["edge.jpg"], [1], [0], device="cpu", size=(C.H, C.W))
    with pytest.raises(ValueError, match="grey.jpg"):
        DeviceRawBank.from_arrays([np.zeros((8, 8), dtype=np.uint8)], ["grey.jpg"], [1], [0], device="cpu")


# ---- the wrapper's host validation ----------------------------------------------------------------------------------------------
class _Recorder(object):
    """stands in for rg_hip.lib.lib: records every entry point a wrapper reaches"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("rg_"):
            raise AttributeError(name)
        return lambda *a: self.calls.append(name)


@pytest.fixture
def recorder(monkeypatch):
    import rg_hip.ops.databank as DB
    rec = _Recorder()
    monkeypatch.setattr(DB, "lib", rec)
    return rec


GOOD = (1, 3, 5, 20, 50, 1, 2, 1, 10, 5, 0x00FF10)       # image 1 is 150x70; the patch lies inside 64 x 32
BAD_ROWS = [
    (-1,) + GOOD[1:], (10,) + GOOD[1:],                                                       # bank row
    (1, -1, 5, 20, 50) + GOOD[5:], (1, 3, -1, 20, 50) + GOOD[5:],                              # box origin
    (1, 3, 5, 0, 50) + GOOD[5:], (1, 3, 5, 20, 0) + GOOD[5:],                                  # empty box
    (1, 51, 5, 20, 50) + GOOD[5:], (1, 3, 101, 20, 50) + GOOD[5:],                             # past the far edges of 150x70
    (3, 0, 0, 33, 64) + GOOD[5:], (3, 0, 0, 32, 65) + GOOD[5:],                                # fits image 1, not image 3 (64x32)
    (1, 2 ** 31 - 1, 5, 20, 50) + GOOD[5:],                                                    # would wrap in int32 arithmetic
    GOOD[:5] + (2,) + GOOD[6:], GOOD[:5] + (-1,) + GOOD[6:],                                    # flip
    GOOD[:6] + (-1, 1, 10, 5, 0), GOOD[:6] + (2, -1, 10, 5, 0),                                 # patch origin
    GOOD[:6] + (60, 1, 10, 5, 0), GOOD[:6] + (2, 30, 10, 5, 0),                                 # patch past the far edges
    GOOD[:6] + (2, 1, -10, 5, 0), GOOD[:6] + (2, 1, 10, -5, 0), GOOD[:6] + (2, 1, 10, 0, 0),
    GOOD[:10] + (-1,), GOOD[:10] + (2 ** 24,),                                                  # rgb
]


def test_good_crop_draws_pack_into_one_buffer():
    d = ops.fd_crop_draws([GOOD, (3, 0, 0, 32, 64, 0, 0, 0, 0, 0, 0)])
    d.check("t", _cpu_bank().sizes_host, C.H, C.W)
    assert d.host.dtype == torch.int32 and tuple(d.host.shape) == (2, 12) and d.host[0].tolist() == list(GOOD) + [0]
    for bad in (lambda: ops.fd_crop_draws(torch.zeros((0, 11), dtype=torch.int64)), lambda: ops.fd_crop_draws([GOOD[:10]]),
                lambda: ops.fd_crop_draws(torch.zeros((1, 11))), lambda: ops.fd_crop_draws([(2 ** 31,) + GOOD[1:]])):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("row", BAD_ROWS)
def test_bad_crop_draws_raise_before_anything_is_launched(recorder, row):
    with pytest.raises(ValueError):
        ops.bank_fd_crop_batch(_cpu_bank(), ops.fd_crop_draws([GOOD, row, GOOD]), torch.from_numpy(LUT))
    assert recorder.calls == []


def test_bad_geometry_raises_before_anything_is_launched(recorder):
    good = ops.fd_crop_draws([GOOD])
    with pytest.raises(TypeError):
        ops.bank_fd_crop_batch(_cpu_bank(), ops.fd_draws([0]), torch.from_numpy(LUT))
    with pytest.raises(RuntimeError, match="GPU"):                     # good draws, but the bank is not on a device: still no launch
        ops.bank_fd_crop_batch(_cpu_bank(), good, torch.from_numpy(LUT))
    assert recorder.calls == []


def test_regime_query_answers_without_a_gpu():
    assert ops.fd_crop_regime(33, 8) == ops.FD_CROP_WHOLE and ops.fd_crop_strip_width(33, 8) == 8
    assert ops.fd_crop_regime(128, 32) == ops.FD_CROP_WHOLE and ops.fd_crop_regime(128, 36) == ops.FD_CROP_STRIPS
    assert ops.fd_crop_regime(128, 128) == ops.FD_CROP_STRIPS and ops.fd_crop_strip_width(128, 128) == 32      # the recipe: 4 strips
    assert ops.fd_crop_strip_width(640, 128) == 32 and ops.fd_crop_strip_width(641, 128) == 28                 # 3 x 641 x 32 > 60 KiB
    assert ops.fd_crop_strip_width(700, 128) == 28 and ops.fd_crop_strip_width(5120, 8) == 4
    for hmax, width in ((128, 6), (0, 8), (5121, 8)):
        with pytest.raises(ValueError):
            ops.fd_crop_regime(hmax, width)


def test_module_does_not_shadow_the_reference_module_names():
    import reid.utils.data as D
    here = os.path.dirname(os.path.abspath(D.__file__))
    assert os.path.isfile(os.path.join(here, "device_stage1.py"))
    for name in ("sampler.py", "preprocessor.py", "transforms.py"):
        assert not os.path.exists(os.path.join(here, name))
    assert D.DeviceStage1Loader.__module__ == "reid.utils.data.device_stage1" and D.get_data_stage1_device and D.FDRandomSizedRectCrop
