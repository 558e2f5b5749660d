"""FD-GAN stage II's pair loaders without a GPU, against tests/golden/reference_fdpairs.npz (the reference's own sampler, transforms
and Preprocessor on the toy set of tests/golden/cases_fdpairs.py): the sampler (sort and draws apart), the eraser's draws, the
landmark reader and the bilinear staging on files written from the fixture's arrays, whole items through the host model
(tests/fd_pairs_hostmodel.py) and through DevicePairLoader with the two launches replaced by it, six planted defects, and the
wrappers' host validation in front of a recording stand-in for the library."""
import os
import random
import types

import numpy as np
import pytest
import torch

from rg_hip import ops
from tests import fd_pairs_hostmodel as HM
from tests.golden import cases_fdpairs as C

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_fdpairs.npz"))
LUT = HM.bank_lut(HM.REID_MEAN, HM.REID_STD)
S = C.MAP_STRIDE


def _same_item(got, aug, n, side):
    """an item equals the fixture's: images bit for bit, maps exactly (CPU: scipy on both sides) at the stored stride, plus the
    full maps' per-joint sums and argmax"""
    key = "item_%s_%d_%d_" % (aug, n, side)
    maps = np.asarray(got["posemap"])
    return (np.asarray(got["origin"]).tobytes() == GOLD[key + "origin"].tobytes()
            and np.asarray(got["target"]).tobytes() == GOLD[key + "target"].tobytes()
            and np.array_equal(maps[:, ::S, ::S], GOLD[key + "posemap"])
            and np.allclose(maps.astype(np.float64).sum((1, 2)), GOLD[key + "posemap_sum"], rtol=1e-12, atol=0)
            and [int(m.argmax()) for m in maps] == GOLD[key + "posemap_argmax"].tolist()
            and np.asarray(got["pid"]).reshape(-1).tolist() == GOLD[key + "pid"].reshape(-1).tolist())


def _model_items(aug, defect=None):
    """the host model's items for the fixture's stored pairs of `aug`, and the two generator probes behind them"""
    pairs = GOLD["pairs_r3_e0"][:C.ITEM_PAIRS[aug]]
    C.seed_items(aug)
    items = [[HM.item(GOLD["planes"], GOLD["landmarks"], C.TRAINVAL, C.PID_IMGS, int(i), aug, LUT, defect) for i in pair] for pair in pairs]
    return items, random.random(), float(torch.rand(1))


# ---- the sampler ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", C.RATIOS)
def test_sampler_sorts_the_pids_as_strings(ratio):
    from reid.utils.data.device_pairs import RandomPairSampler
    s = RandomPairSampler(C.TRAINVAL, ratio)
    assert s.index_map == GOLD["index_map_r%d" % ratio].tolist() == [3, 4, 5, 6, 7, 0, 1, 2, 8, 9]     # '10' < '100' < '2' < '7'
    assert len(s) == int(GOLD["len_r%d" % ratio]) == len(C.TRAINVAL) * (1 + ratio)


@pytest.mark.parametrize("ratio", C.RATIOS)
def test_sampler_draws_the_reference_pairs_for_two_epochs(ratio):
    from reid.utils.data.device_pairs import RandomPairSampler
    s = RandomPairSampler(C.TRAINVAL, ratio)
    C.seed_sampler(ratio)
    for epoch in range(2):
        got = [tuple(p) for p in s]
        assert got == [tuple(p) for p in GOLD["pairs_r%d_e%d" % (ratio, epoch)].tolist()], epoch
        assert all(type(a) is int and type(b) is int for a, b in got)
    C.seed_sampler(ratio)
    assert HM.pair_list(C.TRAINVAL, ratio)[1] == [tuple(p) for p in GOLD["pairs_r%d_e0" % ratio].tolist()]     # the host model's


def test_sampler_refuses_a_single_image_identity():
    from reid.utils.data.device_pairs import RandomPairSampler
    with pytest.raises(ValueError, match="single image"):
        RandomPairSampler(C.TRAINVAL + [("00000055_00_0099.jpg", 55, 0)], 1)
    with pytest.raises(ValueError):
        RandomPairSampler(C.TRAINVAL[:5], 3)                       # two images outside identity 2, three negatives asked for


# ---- the eraser -----------------------------------------------------------------------------------------------------------------
def _paste(rect):
    img = np.full((C.H, C.W, 3), 255, dtype=np.uint8)
    if rect is not None and rect[2] > 0:
        er0, ec0, eh, ew, rgb = rect
        img[er0:er0 + eh, ec0:ec0 + ew] = [(rgb >> (8 * c)) & 255 for c in range(3)]
    return img


def test_eraser_draws_equal_the_reference_on_a_white_image():
    from reid.utils.data.device_pairs import FDRandomErase
    er = FDRandomErase()
    random.seed(C.ERASE_SEED)
    rects = [er.draw(C.H, C.W) for _ in range(C.ERASE_CALLS)]
    assert random.random() == float(GOLD["erase_probe"])            # same consumption of the generator
    got = np.stack([_paste(r) for r in rects])
    wrong = [k for k in range(C.ERASE_CALLS) if not np.array_equal(got[k], GOLD["erase_white"][k])]
    assert not wrong, wrong
    drawn = [r for r in rects if r is not None and r[2] > 0]
    assert len(drawn) >= 10 and any(r[0] + r[2] == C.H or r[1] + r[3] == C.W for r in drawn)       # some are cut by an edge
    for r in drawn:
        assert 0 <= r[0] and r[0] + r[2] <= C.H and 0 <= r[1] and r[1] + r[3] <= C.W and 0 <= r[4] < 2 ** 24
    random.seed(C.ERASE_SEED)                                          # and the host model's restatement
    assert [HM.erase_draw(C.H, C.W) for _ in range(C.ERASE_CALLS)] == rects


# ---- files ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy_dirs(tmp_path_factory):
    """the toy set on disk: the fixture's DECODED originals written losslessly under their .jpg names (PIL reads by content), and
    the landmark files"""
    from PIL import Image
    root = tmp_path_factory.mktemp("fdpairs")
    images, poses = root / "images", root / "poses"
    images.mkdir()
    poses.mkdir()
    for k, name in enumerate(C.NAMES):
        Image.fromarray(GOLD["orig_%d" % k]).save(str(images / name), format="PNG")
        (poses / (os.path.splitext(name)[0] + ".txt")).write_text("\n".join(C.landmark_lines(k)) + "\n")
    return str(images), str(poses)


def test_read_landmarks_and_bilinear_staging(toy_dirs):
    from clustercontrast.utils.data.device_bank import DeviceImageBank, stage_files
    from reid.utils.data.device_pairs import read_landmarks, stage_landmarks
    images, poses = toy_dirs
    for k, name in enumerate(C.NAMES):
        h, w = C.SIZES[k]
        lm = read_landmarks(os.path.join(poses, os.path.splitext(name)[0] + ".txt"), C.H / h, C.W / w)
        assert lm.dtype == np.int32 and np.array_equal(lm, GOLD["landmarks"][k]), k
    assert (GOLD["landmarks"] == -1).any() and GOLD["landmarks"].min() == -1 and (GOLD["landmarks"][:, :, 0] == C.H - 1).any()
    staged = stage_files(C.TRAINVAL, images, (C.H, C.W), None, workers=2, reid_resample="bilinear", pose_root=poses)
    assert np.array_equal(staged["reid_u8"], GOLD["planes"])           # RectScale: PIL's BILINEAR, same-size images as they are
    assert np.array_equal(staged["landmarks"], GOLD["landmarks"]) and staged["old_sizes"].tolist() == [list(s) for s in C.SIZES]
    assert np.array_equal(stage_landmarks(C.NAMES, poses, staged["old_sizes"], (C.H, C.W), only={C.NAMES[4]})[[0, 4]],
                          np.stack([np.full((C.J, 2), -1), GOLD["landmarks"][4]]))
    bicubic = stage_files(C.TRAINVAL, images, (C.H, C.W), None, workers=1)                       # the default is unchanged
    assert "landmarks" not in bicubic and not np.array_equal(bicubic["reid_u8"], GOLD["planes"])
    assert np.array_equal(bicubic["reid_u8"][0], GOLD["planes"][0])                              # 64x32 originals: taken as they are
    with pytest.raises(ValueError):
        stage_files(C.TRAINVAL, images, (C.H, C.W), None, reid_resample="nearest")
    bank = DeviceImageBank.from_files(C.TRAINVAL, images, (C.H, C.W), None, device="cpu", reid_resample="bilinear", pose_root=poses)
    assert bank.landmarks.dtype == torch.int32 and tuple(bank.landmarks.shape) == (10, C.J, 2) and bank.gan is None
    assert bank.nbytes == 10 * (C.H * C.W * 3 + C.J * 2 * 4)


# ---- whole items ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aug", C.AUGS)
def test_host_model_items_equal_the_reference(aug):
    items, probe, tprobe = _model_items(aug)
    for n, pair in enumerate(items):
        for side, it in enumerate(pair):
            assert _same_item(it, aug, n, side), (aug, n, side)
    assert probe == float(GOLD["item_%s_probe" % aug]) and tprobe == float(GOLD["item_%s_torch_probe" % aug])


def _fake_ops(calls):
    """rg_hip.ops with the launches replaced by the host model on CPU tensors; the draws are checked as the wrappers check them"""
    def image(bank_u8, draws, lut):
        calls.append("image")
        draws.check_images("bank_fd_image_batch", bank_u8.shape[0], bank_u8.shape[1], bank_u8.shape[2])
        return torch.from_numpy(HM.fd_image_model(bank_u8.numpy(), draws.idx.tolist(), draws.params.tolist(), lut.numpy()))

    def pose(landmarks, draws, height, width):
        calls.append("pose")
        draws.check_poses("bank_fd_pose_batch", landmarks.shape[0], landmarks.shape[1], height, width)
        return torch.from_numpy(HM.fd_pose_model(landmarks.numpy(), draws.pose_idx.tolist(), draws.pose_params.tolist(), height, width))

    def reid(bank_u8, draws, lut, fill, out_hw, pad=0):
        calls.append("reid")
        draws.check("bank_reid_batch", bank_u8.shape[0], (bank_u8.shape[1], bank_u8.shape[2], out_hw[0], out_hw[1], pad))
        return torch.from_numpy(HM.ordered_batch(bank_u8.numpy(), draws.idx.tolist(), lut.numpy()))
    return types.SimpleNamespace(bank_lut=ops.bank_lut, bank_draws=ops.bank_draws, fd_draws=ops.fd_draws, bank_fd_image_batch=image,
                                 bank_fd_pose_batch=pose, bank_reid_batch=reid)


def _cpu_bank():
    from clustercontrast.utils.data.device_bank import DeviceImageBank
    return DeviceImageBank.from_arrays(GOLD["planes"], C.NAMES, C.PIDS, C.CAMS, landmarks=GOLD["landmarks"], device="cpu")


@pytest.mark.parametrize("aug", C.AUGS)
def test_pair_loader_batches_equal_the_reference_items(aug):
    from reid.utils.data.device_pairs import DevicePairLoader
    calls = []
    B = C.ITEM_PAIRS[aug]
    loader = DevicePairLoader(_cpu_bank(), C.TRAINVAL, C.PID_IMGS, B, neg_pos_ratio=3, pose_aug=aug, ops=_fake_ops(calls))
    assert len(loader) == -(-40 // B)
    C.seed_sampler(3)
    C.seed_items(aug)
    first = next(iter(loader))
    assert calls == ["image", "pose"]
    assert random.random() == float(GOLD["item_%s_probe" % aug]) and float(torch.rand(1)) == float(GOLD["item_%s_torch_probe" % aug])
    assert isinstance(first, tuple) and len(first) == 2
    for side, d in enumerate(first):
        assert sorted(d) == ["origin", "pid", "posemap", "target"]
        assert tuple(d["origin"].shape) == tuple(d["target"].shape) == (B, 3, C.H, C.W) and tuple(d["posemap"].shape) == (B, C.J, C.H, C.W)
        assert d["pid"].dtype == torch.int64 and tuple(d["pid"].shape) == (B, 1)
        for n in range(B):
            assert _same_item({k: v[n].numpy() for k, v in d.items()}, aug, n, side), (aug, n, side)
    assert first[0]["origin"].untyped_storage().data_ptr() == first[1]["target"].untyped_storage().data_ptr()      # one allocation


def test_pair_loader_epochs_and_short_last_batch():
    from reid.utils.data.device_pairs import DevicePairLoader
    loader = DevicePairLoader(_cpu_bank(), C.TRAINVAL, C.PID_IMGS, 16, neg_pos_ratio=3, ops=_fake_ops([]))
    assert len(loader) == 3
    C.seed_sampler(3)
    random.seed(1)
    for epoch in range(2):
        sizes, pids = [], [[], []]
        for b in loader:
            sizes.append(b[0]["origin"].shape[0])
            for side in (0, 1):
                pids[side] += b[side]["pid"].view(-1).tolist()
        assert sizes == [16, 16, 8]                                    # the short last batch is kept
        ref = GOLD["pairs_r3_e%d" % epoch]
        assert pids[0] == [C.PIDS[a] for a in ref[:, 0]] and pids[1] == [C.PIDS[b] for b in ref[:, 1]], epoch
    with pytest.raises(KeyError, match="00000002_00_9999.jpg"):
        DevicePairLoader(_cpu_bank(), C.TRAINVAL, {p: v + ["00000002_00_9999.png"] if p == 2 else v for p, v in C.PID_IMGS.items()}, 4,
                         ops=_fake_ops([]))
    from clustercontrast.utils.data.device_bank import DeviceImageBank
    with pytest.raises(ValueError, match="landmark"):
        DevicePairLoader(DeviceImageBank.from_arrays(GOLD["planes"], C.NAMES, C.PIDS, C.CAMS, device="cpu"), C.TRAINVAL, C.PID_IMGS, 4,
                         ops=_fake_ops([]))


def test_fd_test_loader_and_get_data_device(toy_dirs):
    from reid.utils.data.device_pairs import DeviceFDTestLoader, DevicePairLoader, get_data_device
    calls = []
    entries = [C.TRAINVAL[k] for k in (7, 0, 3, 3, 9)]
    batches = list(DeviceFDTestLoader(_cpu_bank(), entries, 2, ops=_fake_ops(calls)))
    assert calls == ["reid"] * 3 and [len(b) for b in batches] == [4, 4, 4] and [b[0].shape[0] for b in batches] == [2, 2, 1]
    assert torch.cat([b[0] for b in batches]).numpy().tobytes() == HM.ordered_batch(GOLD["planes"], [7, 0, 3, 3, 9], LUT).tobytes()
    assert sum((b[1] for b in batches), []) == [e[0] for e in entries]
    assert torch.cat([b[2] for b in batches]).tolist() == [e[1] for e in entries]
    assert torch.cat([b[3] for b in batches]).tolist() == [e[2] for e in entries]
    images, poses = toy_dirs
    ds = types.SimpleNamespace(trainval=C.TRAINVAL[:8], trainval_query={p: [n for n in v if n in C.NAMES[:8]] for p, v in C.PID_IMGS.items()
                                                                       if p != 7},
                               query=[C.TRAINVAL[8]], gallery=[C.TRAINVAL[9], C.TRAINVAL[8]], images_dir=images, poses_dir=poses)
    os.remove(os.path.join(poses, os.path.splitext(C.NAMES[9])[0] + ".txt"))        # a gallery image needs no landmark file
    try:
        got, train, test = get_data_device(ds, C.H, C.W, 4, "gauss", workers=1, device="cpu")
    finally:
        with open(os.path.join(poses, os.path.splitext(C.NAMES[9])[0] + ".txt"), "w") as f:
            f.write("\n".join(C.landmark_lines(9)) + "\n")
    assert got is ds and isinstance(train, DevicePairLoader) and isinstance(test, DeviceFDTestLoader)
    assert train.bank is test.bank and len(train.bank) == 10 and len(train) == 8 and len(test) == 1
    assert train.pose_aug == "gauss" and train.sampler.neg_pos_ratio == 3
    rows = [train.bank.row[n] for n in C.NAMES]
    assert np.array_equal(train.bank.reid.numpy()[rows], GOLD["planes"])
    assert np.array_equal(train.bank.landmarks.numpy()[rows[:8]], GOLD["landmarks"][:8]) and (train.bank.landmarks.numpy()[rows[8:]] == -1).all()


# ---- planted defects ------------------------------------------------------------------------------------------------------------
def test_paste_at_the_sized_box_is_told_apart():
    random.seed(C.ERASE_SEED)
    got = np.stack([_paste(HM.erase_draw(C.H, C.W, defect="paste_at_x1y1")) for _ in range(C.ERASE_CALLS)])
    assert random.random() == float(GOLD["erase_probe"])               # the same draws ...
    assert not np.array_equal(got, GOLD["erase_white"])                # ... another image


@pytest.mark.parametrize("defect", ["paste_at_x1y1", "rect_after_flip", "colour_after_normalize", "partner_first", "tflip_before_partner"])
def test_item_defects_are_told_apart(defect):
    hit = []
    for aug in C.AUGS:
        items, probe, _ = _model_items(aug, defect)
        hit += [_same_item(it, aug, n, side) for n, pair in enumerate(items) for side, it in enumerate(pair)]
    assert not all(hit), defect


@pytest.mark.parametrize("ratio", C.RATIOS)
def test_numeric_pid_order_is_told_apart(ratio):
    C.seed_sampler(ratio)
    index_map, pairs = HM.pair_list(C.TRAINVAL, ratio, defect="numeric_pid_order")
    assert index_map != GOLD["index_map_r%d" % ratio].tolist()
    assert pairs != [tuple(p) for p in GOLD["pairs_r%d_e0" % ratio].tolist()]


# ---- the wrappers' host validation ----------------------------------------------------------------------------------------------
class _Recorder(object):
    """stands in for rg_hip.lib.lib: records every entry point a wrapper reaches"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("rg_"):
            raise AttributeError(name)
        return lambda *a: self.calls.append(name)


GOOD_I = (1, 0, 0, 2, 1, 10, 5, 0x00FF10)          # inside 12 x 6
GOOD_P = (1, 1, 3, 0)                              # sigma 1: radius 4 <= min(12, 6)


@pytest.fixture
def recorder(monkeypatch):
    import rg_hip.ops.databank as DB
    rec = _Recorder()
    monkeypatch.setattr(DB, "lib", rec)
    return rec


def test_good_fd_draws_pack_into_one_buffer():
    d = ops.fd_draws([0, 6, 3], [GOOD_I, (0,) * 8, (0, 0, 0, 11, 5, 1, 1, 2 ** 24 - 1)], [4, 1], [GOOD_P, (0, 1, -1, 0)])
    d.check_images("t", 7, 12, 6)
    d.check_poses("t", 7, 5, 12, 6)
    assert d.host.dtype == torch.int32 and d.host.numel() == 3 * 9 + 2 * 5
    assert d.host[24:27].tolist() == [0, 6, 3] and d.host[27:35].tolist() == list(GOOD_P) + [0, 1, -1, 0] and d.host[35:].tolist() == [4, 1]
    for view in (d.idx, d.params, d.pose_idx, d.pose_params):
        assert view.untyped_storage().data_ptr() == d.host.untyped_storage().data_ptr()
    only_images = ops.fd_draws([1, 2])
    assert only_images.params.tolist() == [[0] * 8] * 2 and only_images.pose_idx.numel() == 0
    with pytest.raises(ValueError):
        only_images.check_poses("t", 7, 5, 12, 6)
    for bad in (lambda: ops.fd_draws(), lambda: ops.fd_draws([0], torch.zeros(1, 7, dtype=torch.int64)), lambda: ops.fd_draws(None, None, [0]),
                lambda: ops.fd_draws([0], torch.zeros(1, 8)), lambda: ops.fd_draws([2 ** 31]), lambda: ops.fd_draws([0, 1], [GOOD_I])):
        with pytest.raises(ValueError):
            bad()


BAD_IMAGE_ROWS = [
    (-1, GOOD_I), (7, GOOD_I),
    (0, (2, 0, 0, 2, 1, 10, 5, 0)), (0, (-1, 0, 0, 2, 1, 10, 5, 0)),                        # flip
    (0, (0, 0, 0, -1, 0, 2, 2, 0)), (0, (0, 0, 0, 0, -1, 2, 2, 0)),                        # rectangle origin
    (0, (0, 0, 0, 3, 0, 10, 2, 0)), (0, (0, 0, 0, 0, 2, 2, 5, 0)),                         # past the far edges
    (0, (0, 0, 0, 0, 0, -2, 2, 0)), (0, (0, 0, 0, 0, 0, 2, -2, 0)), (0, (0, 0, 0, 0, 0, 2, 0, 0)),
    (0, (0, 0, 0, 2 ** 31 - 1, 0, 2, 2, 0)),                                               # would wrap in int32 arithmetic
    (0, (0, 0, 0, 0, 0, 0, 0, -1)), (0, (0, 0, 0, 0, 0, 0, 0, 2 ** 24)),                   # rgb
]
BAD_POSE_ROWS = [
    (-1, GOOD_P), (7, GOOD_P), (0, (2, 1, 3, 0)), (0, (-1, 1, 3, 0)),
    (0, (0, 0, -1, 0)), (0, (0, -5, -1, 0)),                                               # sigma < 1
    (0, (0, 2, -1, 0)),                                                                    # radius 8 > min(12, 6)
    (0, (0, 1, 5, 0)), (0, (0, 1, -2, 0)),                                                 # erased joint outside [-1, 5)
]


@pytest.mark.parametrize("idx,row", BAD_IMAGE_ROWS)
def test_bad_image_draws_raise_before_anything_is_launched(recorder, idx, row):
    bank = torch.zeros((7, 12, 6, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.bank_fd_image_batch(bank, ops.fd_draws([0, idx, 1], [GOOD_I, row, GOOD_I]), torch.from_numpy(LUT))
    assert recorder.calls == []


@pytest.mark.parametrize("idx,row", BAD_POSE_ROWS)
def test_bad_pose_draws_raise_before_anything_is_launched(recorder, idx, row):
    table = torch.zeros((7, 5, 2), dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.bank_fd_pose_batch(table, ops.fd_draws(None, None, [0, idx, 1], [GOOD_P, row, GOOD_P]), 12, 6)
    assert recorder.calls == []


def test_bad_geometry_raises_before_anything_is_launched(recorder):
    table = torch.zeros((7, 5, 2), dtype=torch.int32)
    good = ops.fd_draws([0], [GOOD_I], [0], [GOOD_P])
    for h, w in ((1025, 6), (12, 1025), (0, 6)):
        with pytest.raises(ValueError):
            ops.bank_fd_pose_batch(table, good, h, w)
    with pytest.raises(ValueError):                                    # N > 65535
        ops.bank_fd_pose_batch(table, ops.fd_draws(None, None, torch.zeros(65536, dtype=torch.int64),
                                                   torch.tensor([GOOD_P], dtype=torch.int64).repeat(65536, 1)), 12, 6)
    with pytest.raises(ValueError):
        ops.bank_fd_pose_batch(table.long(), good, 12, 6)
    with pytest.raises(ValueError):
        ops.bank_fd_image_batch(torch.zeros((7, 12, 6), dtype=torch.uint8), good, torch.from_numpy(LUT))
    with pytest.raises(TypeError):
        ops.bank_fd_image_batch(torch.zeros((7, 12, 6, 3), dtype=torch.uint8), ops.bank_draws([0], None), torch.from_numpy(LUT))
    with pytest.raises(RuntimeError, match="GPU"):                     # good draws, but the bank is not on a device: still no launch
        ops.bank_fd_image_batch(torch.zeros((7, 12, 6, 3), dtype=torch.uint8), good, torch.from_numpy(LUT))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.bank_fd_pose_batch(table, good, 12, 6)
    assert recorder.calls == []


def test_module_does_not_shadow_the_reference_module_names():
    import reid.utils.data as D
    here = os.path.dirname(os.path.abspath(D.__file__))
    assert os.path.isfile(os.path.join(here, "device_pairs.py"))
    for name in ("sampler.py", "preprocessor.py", "transforms.py"):
        assert not os.path.exists(os.path.join(here, name))
    assert D.DevicePairLoader.__module__ == "reid.utils.data.device_pairs" and D.get_data_device and D.RandomPairSampler and D.FDRandomErase
