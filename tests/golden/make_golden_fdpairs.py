"""Generates tests/golden/reference_fdpairs.npz by running the REFERENCE's own FD-GAN stage-II input pipeline on the toy data set
of cases_fdpairs.py (build container only; the reference tree does not exist where the tests run):

  * FD/reid/utils/data/sampler.py        `RandomPairSampler`                       (index_map, len(), two epochs per ratio)
  * FD/reid/utils/data/transforms.py     `RectScale`, `RandomSizedEarser`          (the planes; erased white images)
  * FD/reid/utils/data/preprocessor.py   `Preprocessor._load_landmark`, `Preprocessor.__getitem__((i, j))`  (tables; whole items)

The three files are loaded by path (the recipe of make_golden_datagen.py); `Sampler.__init__` gets the constructor the reference
was written against (make_golden_bank.py).  transforms.py does `from torchvision.transforms import *` and the Preprocessor composes
four of torchvision's classes; torchvision is not installed, so the placeholder module carries four minimal stand-ins.  THOSE FOUR
— Compose, ToTensor, Normalize, RandomHorizontalFlip — ARE TORCHVISION'S, NOT THE REFERENCE'S, restated here from their documented
behaviour: ToTensor = HWC bytes -> CHW float32 / 255; Normalize = (x - mean) / std per channel in float32; RandomHorizontalFlip =
`torch.rand(1) < p` on torch's default generator, then the PIL transpose.  That last draw follows torchvision's current source and
was not verified against a torchvision run.

Nothing from the reference is copied: the file stores inputs (decoded toy images) and the reference's outputs.  After each seeded
sequence one `random.random()` is stored, which pins how much of the generator the sequence consumed.

Usage:  python tests/golden/make_golden_fdpairs.py [path of the reference's FD-GAN tree]
"""
from __future__ import absolute_import, print_function

import importlib.util
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from tests.golden import cases_fdpairs as C  # noqa: E402

FD = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/FD-GAN-master"


# ---- torchvision's four, not the reference's ------------------------------------------------------------------------------------
class Compose(object):
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, img):
        for t in self.transforms:
            img = t(img)
        return img


class ToTensor(object):
    def __call__(self, pic):
        return torch.from_numpy(np.asarray(pic, dtype=np.uint8).copy()).permute(2, 0, 1).contiguous().float().div(255)


class Normalize(object):
    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, t):
        mean = torch.as_tensor(self.mean, dtype=torch.float32).view(-1, 1, 1)
        std = torch.as_tensor(self.std, dtype=torch.float32).view(-1, 1, 1)
        return t.clone().sub_(mean).div_(std)


class RandomHorizontalFlip(object):
    def __init__(self, p=0.5):
        self.p = p

    def __call__(self, img):
        if torch.rand(1) < self.p:
            return img.transpose(Image.FLIP_LEFT_RIGHT)
        return img


def _placeholders():
    tv = types.ModuleType("torchvision")
    tvt = types.ModuleType("torchvision.transforms")
    tvt.Compose, tvt.ToTensor, tvt.Normalize, tvt.RandomHorizontalFlip = Compose, ToTensor, Normalize, RandomHorizontalFlip
    tvt.__all__ = ["Compose", "ToTensor", "Normalize", "RandomHorizontalFlip"]
    tv.transforms = tvt
    sys.modules["torchvision"] = tv
    sys.modules["torchvision.transforms"] = tvt


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    _placeholders()
    for name, path in (("reid", FD + "/reid"), ("reid.utils", FD + "/reid/utils"), ("reid.utils.data", FD + "/reid/utils/data")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    T = load(FD + "/reid/utils/data/transforms.py", "reid.utils.data.transforms")
    sys.modules["reid.utils.data"].transforms = T
    P = load(FD + "/reid/utils/data/preprocessor.py", "reid.utils.data.preprocessor")
    S = load(FD + "/reid/utils/data/sampler.py", "fd_ref_sampler")
    S.Sampler.__init__ = lambda self, data_source=None: None

    out = {}
    with tempfile.TemporaryDirectory(prefix="fdpairs_") as root:
        images, poses = os.path.join(root, "images"), os.path.join(root, "poses")
        os.mkdir(images)
        os.mkdir(poses)
        for k, name in enumerate(C.NAMES):
            Image.fromarray(C.source_image(k)).save(os.path.join(images, name), quality=92)
            with open(os.path.join(poses, os.path.splitext(name)[0] + ".txt"), "w") as f:
                f.write("\n".join(C.landmark_lines(k)) + "\n")
        pre = P.Preprocessor(C.TRAINVAL, root=images, with_pose=True, pose_root=poses, pid_imgs=C.PID_IMGS, height=C.H, width=C.W)

        # decoded originals, RectScale planes, landmark tables
        scale = T.RectScale(C.H, C.W)
        planes, tables = [], []
        for k, name in enumerate(C.NAMES):
            img = Image.open(os.path.join(images, name)).convert("RGB")
            assert (img.size[1], img.size[0]) == C.SIZES[k]
            out["orig_%d" % k] = np.asarray(img, dtype=np.uint8).copy()
            planes.append(np.asarray(scale(img), dtype=np.uint8).copy())
            lm = pre._load_landmark(os.path.join(poses, os.path.splitext(name)[0] + ".txt"), C.H / img.size[1], C.W / img.size[0])
            tables.append(lm.numpy().astype(np.int32))
        out["planes"] = np.stack(planes)
        out["landmarks"] = np.stack(tables)
        print("planes", out["planes"].shape, "landmarks", out["landmarks"].shape, "missing entries", int((out["landmarks"] < 0).sum()))

        # the pair sampler
        for ratio in C.RATIOS:
            s = S.RandomPairSampler(C.TRAINVAL, neg_pos_ratio=ratio)
            out["index_map_r%d" % ratio] = np.asarray([s.index_map[i] for i in range(len(C.TRAINVAL))], dtype=np.int64)
            out["len_r%d" % ratio] = np.int64(len(s))
            C.seed_sampler(ratio)
            for epoch in range(2):
                out["pairs_r%d_e%d" % (ratio, epoch)] = np.asarray([(int(a), int(b)) for a, b in s], dtype=np.int64)
            print("sampler ratio", ratio, "index_map", out["index_map_r%d" % ratio].tolist(), "len", len(s))

        # the eraser on a white image
        er = T.RandomSizedEarser()
        random.seed(C.ERASE_SEED)
        erased = [np.asarray(er(Image.new("RGB", (C.W, C.H), (255, 255, 255))), dtype=np.uint8).copy() for _ in range(C.ERASE_CALLS)]
        out["erase_white"] = np.stack(erased)
        out["erase_probe"] = np.float64(random.random())
        print("eraser:", sum(int((e != 255).any()) for e in erased), "of", C.ERASE_CALLS, "calls leave a visible rectangle")

        # whole items
        for aug in C.AUGS:
            pairs = out["pairs_r3_e0"][:C.ITEM_PAIRS[aug]]
            pre.pose_aug = aug
            C.seed_items(aug)
            for n, (i, j) in enumerate(pairs):
                for side, item in enumerate(pre[(int(i), int(j))]):
                    key = "item_%s_%d_%d_" % (aug, n, side)
                    maps = item["posemap"].numpy()
                    assert maps.dtype == np.float32 and maps.shape == (C.J, C.H, C.W)
                    out[key + "origin"] = item["origin"].numpy()
                    out[key + "target"] = item["target"].numpy()
                    out[key + "posemap"] = maps[:, ::C.MAP_STRIDE, ::C.MAP_STRIDE].copy()
                    out[key + "posemap_sum"] = maps.astype(np.float64).sum((1, 2))
                    out[key + "posemap_argmax"] = np.array([int(m.argmax()) for m in maps])
                    out[key + "pid"] = item["pid"].numpy()
            out["item_%s_probe" % aug] = np.float64(random.random())
            out["item_%s_torch_probe" % aug] = np.float64(float(torch.rand(1)))
            print("items", aug, "pairs", pairs.tolist())
    path = os.path.join(HERE, "reference_fdpairs.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
