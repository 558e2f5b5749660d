"""tests/bank_hostmodel.py tied down without a GPU, bit for bit everywhere:

  (a) against the reference's transform composition written out line by line in torch on PIL images (Resize -> Pad -> RandomCrop
      -> ToTensor -> Normalize -> RandomErasing -> torch.flip; F.resize -> ToTensor -> Normalize -> flip for the GAN image;
      cords_to_map -> flip for the pose maps), on planes built by DeviceImageBank's own host staging;
  (b) against planted defects: each of seven wrong variants of the ReID definition must differ from that composition;
  (c) the table equals the elementwise torch expression at all 3 x 256 entries.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import bank_hostmodel as HM

REID_SIZE, GAN_SIZE, PAD = (32, 16), (16, 8), 3
NATIVE = [(128, 64), (301, 140), (90, 70)]              # (height, width): the data set's own, a larger one, one that is not 2:1
# (flip, top, left, er0, ec0, eh, ew): corners of the offset range, rectangles at the edges, asymmetric in every respect
DRAWS = [(0, 0, 0, 0, 0, 0, 0), (1, 6, 0, 2, 1, 5, 3), (0, 0, 6, 27, 13, 5, 3), (1, 3, 5, 0, 9, 31, 7), (1, 6, 6, 31, 15, 1, 1),
         (0, 2, 4, 1, 0, 31, 15)]


def _images(tmp_path):
    """seeded random images with structure (so that a resize is not noise -> grey), one file format per size"""
    Image = pytest.importorskip("PIL.Image")
    g = np.random.RandomState(5)
    entries = []
    for k, (h, w) in enumerate(NATIVE * 2):
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([(yy * 255 // h), (xx * 255 // w), ((yy + 2 * xx) % 256)], axis=2) + g.randint(-40, 40, size=(h, w, 3))
        name = "%04d_c%ds1_%06d.%s" % (k + 3, k % 3 + 1, k, "png" if k % 2 else "jpg")
        Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(os.path.join(str(tmp_path), name))
        entries.append((name, k + 3, k % 3))
    return entries


def _pose_file(tmp_path, entries):
    g = np.random.RandomState(6)
    path = os.path.join(str(tmp_path), "pose.csv")
    with open(path, "w") as f:
        f.write("name:keypoints_y:keypoints_x\n")
        for k, (name, _, _) in enumerate(entries):
            h, w = (NATIVE * 2)[k]
            ys, xs = g.randint(0, h, size=18), g.randint(0, w, size=18)
            ys[k % 18] = -1                                   # a missing joint, marked in one coordinate or in both
            xs[(k + 5) % 18] = -1
            ys[(k + 5) % 18] = -1 if k % 2 else ys[(k + 5) % 18]
            f.write("%s: %s: %s\n" % (name, json.dumps([int(v) for v in ys]), json.dumps([int(v) for v in xs])))
    return path


@pytest.fixture(scope="module")
def staged(tmp_path_factory):
    from clustercontrast.utils.data import device_bank as B
    tmp = tmp_path_factory.mktemp("bank")
    entries = _images(tmp)
    pose = _pose_file(tmp, entries)
    st = B.stage_files(entries, str(tmp), REID_SIZE, GAN_SIZE, pose, workers=3)
    return str(tmp), entries, pose, st


def _reference_reid(path, draw):
    """the reference's train transform and Preprocessor flip, one torchvision step per line, on the PIL image"""
    from PIL import Image, ImageOps
    flip, top, left, er0, ec0, eh, ew = draw
    H, W = REID_SIZE
    img = Image.open(path).convert("RGB")
    img = img.resize((W, H), Image.BICUBIC)                                   # T.Resize((h, w), interpolation=BICUBIC)
    img = ImageOps.expand(img, border=PAD, fill=0)                            # T.Pad(pad)
    img = img.crop((left, top, left + W, top + H))                            # T.RandomCrop((h, w)) at the drawn offset
    t = torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).contiguous().float().div(255)        # T.ToTensor
    mean, std = torch.tensor(HM.REID_MEAN, dtype=torch.float32), torch.tensor(HM.REID_STD, dtype=torch.float32)
    t = t.sub(mean[:, None, None]).div(std[:, None, None])                    # T.Normalize
    if eh > 0:                                                                # RandomErasing at the drawn rectangle
        for c in range(3):
            t[c, er0:er0 + eh, ec0:ec0 + ew] = HM.REID_MEAN[c]
    if flip:
        t = torch.flip(t, [2])                                                # Preprocessor.__getitem__, flip_all
    return t.numpy()


def _reference_gan(path, flip):
    from PIL import Image
    img = Image.open(path).convert("RGB")
    img = img.resize((GAN_SIZE[1], GAN_SIZE[0]), Image.BILINEAR)              # F.resize(Xs, load_size)
    t = torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).contiguous().float().div(255)
    half = torch.tensor(HM.GAN_MEAN, dtype=torch.float32)
    t = t.sub(half[:, None, None]).div(half[:, None, None])
    return (torch.flip(t, [2]) if flip else t).numpy()


def _reference_pose(cords, old_size, flip, sigma=6):
    """cords_to_map (pose_utils.py:51-70) evaluated point by point, then np.transpose(pose, (2, 0, 1)) and torch.flip(Ps, [2])"""
    H, W = GAN_SIZE
    cords = np.asarray(cords).astype(float)
    result = np.zeros((H, W, cords.shape[0]), dtype="float32")
    for i, point in enumerate(cords):
        if point[0] == -1 or point[1] == -1:
            continue
        p0, p1 = int(point[0] / old_size[0] * H), int(point[1] / old_size[1] * W)
        for yy in range(H):
            for xx in range(W):
                result[yy, xx, i] = np.exp(-((yy - p0) ** 2 + (xx - p1) ** 2) / (2 * sigma ** 2))
    t = torch.from_numpy(np.transpose(result, (2, 0, 1)).copy())
    return (torch.flip(t, [2]) if flip else t).numpy()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_staging_is_one_decode_and_two_pil_resizes(staged):
    from PIL import Image
    root, entries, _, st = staged
    assert st["reid_u8"].shape == (6,) + REID_SIZE + (3,) and st["reid_u8"].dtype == np.uint8
    assert st["gan_u8"].shape == (6,) + GAN_SIZE + (3,) and st["gan_u8"].dtype == np.uint8
    assert [tuple(o) for o in st["old_sizes"]] == NATIVE * 2
    assert st["fnames"] == [e[0] for e in entries] and st["pids"] == [e[1] for e in entries] and st["camids"] == [e[2] for e in entries]
    img = Image.open(os.path.join(root, entries[1][0])).convert("RGB")
    assert _same(st["reid_u8"][1], np.asarray(img.resize(REID_SIZE[::-1], Image.BICUBIC)))
    assert _same(st["gan_u8"][1], np.asarray(img.resize(GAN_SIZE[::-1], Image.BILINEAR)))


def test_staging_keeps_an_image_that_already_has_the_size(tmp_path):
    from clustercontrast.utils.data import device_bank as B
    Image = pytest.importorskip("PIL.Image")
    a = np.random.RandomState(1).randint(0, 256, size=(16, 8, 3)).astype(np.uint8)
    Image.fromarray(a).save(str(tmp_path / "0001_c1s1_000001.png"))
    st = B.stage_files([("0001_c1s1_000001.png", 1, 0)], str(tmp_path), (16, 8), (16, 8), workers=1)
    assert _same(st["reid_u8"][0], a) and _same(st["gan_u8"][0], a)


def test_reid_model_equals_the_reference_composition(staged):
    root, entries, _, st = staged
    lut, fill = HM.bank_lut(HM.REID_MEAN, HM.REID_STD), np.asarray(HM.REID_MEAN, dtype=np.float32)
    idx = [3, 0, 5, 1, 1, 4]
    got = HM.reid_batch_model(st["reid_u8"], idx, DRAWS, lut, fill, REID_SIZE[0], REID_SIZE[1], PAD)
    for n, (m, draw) in enumerate(zip(idx, DRAWS)):
        assert _same(got[n], _reference_reid(os.path.join(root, entries[m][0]), draw)), (n, m, draw)


def test_test_time_form_equals_resize_totensor_normalize(staged):
    root, entries, _, st = staged
    lut = HM.bank_lut(HM.REID_MEAN, HM.REID_STD)
    got = HM.reid_batch_model(st["reid_u8"], [2, 4], np.zeros((2, 8), dtype=np.int64), lut, np.zeros(3, np.float32), REID_SIZE[0],
                              REID_SIZE[1], 0)
    for n, m in enumerate([2, 4]):
        from PIL import Image
        img = Image.open(os.path.join(root, entries[m][0])).convert("RGB").resize(REID_SIZE[::-1], Image.BICUBIC)
        t = torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).contiguous().float().div(255)
        t = t.sub(torch.tensor(HM.REID_MEAN)[:, None, None]).div(torch.tensor(HM.REID_STD)[:, None, None])
        assert _same(got[n], t.numpy())


def test_gan_model_equals_the_reference_composition(staged):
    root, entries, _, st = staged
    idx, flips = [5, 2, 2, 0], [1, 0, 1, 0]
    got = HM.gan_batch_model(st["gan_u8"], idx, flips, HM.bank_lut(HM.GAN_MEAN, HM.GAN_STD))
    for n, (m, f) in enumerate(zip(idx, flips)):
        assert _same(got[n], _reference_gan(os.path.join(root, entries[m][0]), f)), (n, m, f)


def test_pose_centres_and_model_equal_the_reference(staged):
    from clustercontrast.utils.data import device_bank as B
    from clustercontrast.utils.data.device_pose import _centres
    _, entries, pose, st = staged
    centres = B.stage_centres(st["cords"], st["old_sizes"], GAN_SIZE)
    assert centres.dtype == np.int32 and centres.shape == (6, 18, 2)
    for m in range(6):
        want = np.clip(_centres(st["cords"][m], GAN_SIZE, tuple(int(v) for v in st["old_sizes"][m]), None), -2 ** 31, 2 ** 31 - 1)
        assert (centres[m] == want).all()
        assert (centres[m] == HM.MISSING).any(axis=1).sum() == 2            # the two planted missing joints, and only those
    idx, flips = [4, 1, 1], [1, 0, 1]
    got = HM.pose_batch_model(centres, idx, flips, 6, GAN_SIZE[0], GAN_SIZE[1])
    for n, (m, f) in enumerate(zip(idx, flips)):
        assert _same(got[n], _reference_pose(st["cords"][m], st["old_sizes"][m], f)), (n, m, f)


# ---- (b) planted defects ------------------------------------------------------------------------------------------------------
DEFECTS = ["flip_before_erasing", "padding_zero", "top_left_swapped", "hwc_as_chw", "lut_channel_0", "rect_far_edge", "gan_lut"]


def _variant(bank, idx, params, H, W, pad, defect=None):
    """the ReID definition with one switchable mistake"""
    lut = HM.bank_lut(HM.GAN_MEAN, HM.GAN_STD) if defect == "gan_lut" else HM.bank_lut(HM.REID_MEAN, HM.REID_STD)
    fill = np.asarray(HM.REID_MEAN, dtype=np.float32)
    M, Hs, Ws, _ = bank.shape
    out = np.empty((len(idx), 3, H, W), dtype=np.float32)
    far = 1 if defect == "rect_far_edge" else 0
    for n in range(len(idx)):
        flip, top, left, er0, ec0, eh, ew = [int(v) for v in params[n][:7]]
        if defect == "top_left_swapped":
            top, left = left, top
        plane = bank[idx[n]]
        chw = plane.reshape(3, Hs, Ws)
        for c in range(3):
            lc = 0 if defect == "lut_channel_0" else c
            for y in range(H):
                for x in range(W):
                    xs = W - 1 - x if flip else x
                    xe = x if defect == "flip_before_erasing" else xs
                    if eh > 0 and er0 <= y < er0 + eh + far and ec0 <= xe < ec0 + ew + far:
                        out[n, c, y, x] = fill[c]
                        continue
                    r, q = top + y - pad, left + xs - pad
                    if r < 0 or r >= Hs or q < 0 or q >= Ws:
                        out[n, c, y, x] = np.float32(0.0) if defect == "padding_zero" else lut[lc][0]
                    else:
                        out[n, c, y, x] = lut[lc][chw[c][r][q] if defect == "hwc_as_chw" else plane[r][q][c]]
    return out


@pytest.fixture(scope="module")
def composition(staged):
    root, entries, _, st = staged
    idx = [3, 0, 5, 1, 1, 4]
    ref = np.stack([_reference_reid(os.path.join(root, entries[m][0]), d) for m, d in zip(idx, DRAWS)])
    return st["reid_u8"], idx, ref


def test_the_variant_without_a_defect_is_the_model(composition):
    bank, idx, ref = composition
    lut, fill = HM.bank_lut(HM.REID_MEAN, HM.REID_STD), np.asarray(HM.REID_MEAN, dtype=np.float32)
    assert _same(_variant(bank, idx, DRAWS, REID_SIZE[0], REID_SIZE[1], PAD), ref)
    assert _same(HM.reid_batch_model(bank, idx, DRAWS, lut, fill, REID_SIZE[0], REID_SIZE[1], PAD), ref)


@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defect_is_caught(composition, defect):
    bank, idx, ref = composition
    got = _variant(bank, idx, DRAWS, REID_SIZE[0], REID_SIZE[1], PAD, defect)
    wrong = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
    print("%s: %d of %d elements differ from the reference composition" % (defect, wrong, ref.size))
    assert wrong > 0, "the comparison with the reference composition does not see %s" % defect


# ---- (c) the table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mean,std", [(HM.REID_MEAN, HM.REID_STD), (HM.GAN_MEAN, HM.GAN_STD)], ids=["reid", "gan"])
def test_lut_equals_the_elementwise_expression(mean, std):
    from rg_hip import ops
    lut = ops.bank_lut(mean, std)
    assert lut.dtype == torch.float32 and tuple(lut.shape) == (3, 256) and lut.is_contiguous()
    assert _same(lut.numpy(), HM.bank_lut(mean, std))
    for c in range(3):
        for b in range(256):
            # ToTensor on one byte, then Normalize on that one value
            v = torch.tensor([b], dtype=torch.uint8).float().div(255)
            v = v.sub(torch.as_tensor(mean[c], dtype=torch.float32)).div(torch.as_tensor(std[c], dtype=torch.float32))
            assert lut[c, b].numpy().tobytes() == v[0].numpy().tobytes(), (c, b)
