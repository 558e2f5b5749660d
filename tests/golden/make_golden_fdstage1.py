"""Generates tests/golden/reference_fdstage1.npz by running the REFERENCE's own FD-GAN stage-I input pipeline on the toy data of
cases_fdstage1.py (build container only; the reference tree does not exist where the tests run):

  * FD/reid/utils/data/transforms.py     `RandomSizedRectCrop`, `RandomSizedEarser`     (boxes; crop outputs)
  * FD/reid/utils/data/sampler.py        `RandomPairSampler`                            (the pairs the items are drawn for)
  * FD/reid/utils/data/preprocessor.py   `Preprocessor.__getitem__((i, j))` with baseline.py's train transform  (whole items)

The files are loaded by path and torchvision's four classes are stood in for exactly as make_golden_fdpairs.py does it (its
docstring says what they are and that the flip's draw was not verified against a torchvision run).  RandomSizedRectCrop does not
return its box: `PIL.Image.Image.crop` is wrapped for the duration of a call to note the box it is given; a call that never crops
is the fallback, the whole image.

Nothing from the reference is copied: the file stores the reference's outputs.  After each seeded sequence one `random.random()`
is stored, which pins how much of the generator the sequence consumed.

Usage:  python tests/golden/make_golden_fdstage1.py [path of the reference's FD-GAN tree]
"""
from __future__ import absolute_import, print_function

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
from tests.golden import cases_fdstage1 as C  # noqa: E402
from tests.golden import make_golden_fdpairs as G  # noqa: E402  (the placeholders and the loader by path)

FD = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/FD-GAN-master"


class NoteBox(object):
    """while active, PIL's crop notes the box it is called with"""

    def __enter__(self):
        self.box, self.inner = None, Image.Image.crop
        note = self

        def crop(img, box=None):
            note.box = tuple(int(v) for v in box)
            return note.inner(img, box)
        Image.Image.crop = crop
        return self

    def __exit__(self, *exc):
        Image.Image.crop = self.inner


def cropped(transform, img):
    """(x1, y1, w, h) of one call and its output image"""
    with NoteBox() as note:
        out = transform(img)
    if note.box is None:
        return (0, 0, img.size[0], img.size[1]), out
    x1, y1, x2, y2 = note.box
    return (x1, y1, x2 - x1, y2 - y1), out


def main():
    G._placeholders()
    for name, path in (("reid", FD + "/reid"), ("reid.utils", FD + "/reid/utils"), ("reid.utils.data", FD + "/reid/utils/data")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    T = G.load(FD + "/reid/utils/data/transforms.py", "reid.utils.data.transforms")
    sys.modules["reid.utils.data"].transforms = T
    P = G.load(FD + "/reid/utils/data/preprocessor.py", "reid.utils.data.preprocessor")
    S = G.load(FD + "/reid/utils/data/sampler.py", "fd_ref_sampler")
    S.Sampler.__init__ = lambda self, data_source=None: None

    out = {"images_sum": np.uint64(C.images_sum())}

    # the boxes
    for name, (hs, ws, draws, seed) in C.BOXES.items():
        t = T.RandomSizedRectCrop(256, 128)
        img = Image.new("RGB", (ws, hs), (90, 120, 30))
        random.seed(seed)
        boxes = []
        for _ in range(draws):
            box, res = cropped(t, img)
            assert res.size == (128, 256)
            boxes.append(box)
        out["boxes_" + name] = np.asarray(boxes, dtype=np.int64)
        out["boxes_%s_probe" % name] = np.float64(random.random())
        whole = sum(1 for b in boxes if b == (0, 0, ws, hs))
        print("boxes", name, len(boxes), "draws,", whole, "whole images")

    # crop outputs
    for name, (k, ho, wo, draws, full, seed) in C.CROPS.items():
        t = T.RandomSizedRectCrop(ho, wo)
        random.seed(seed)
        boxes, sums = [], []
        for n in range(draws):
            box, res = cropped(t, Image.fromarray(C.source_image(k)))
            a = np.asarray(res, dtype=np.uint8)
            assert a.shape == (ho, wo, 3)
            boxes.append(box)
            sums.append(C.byte_sum(a))
            if n < full:
                out["crop_%s_%d" % (name, n)] = a.copy()
        out["crop_%s_boxes" % name] = np.asarray(boxes, dtype=np.int64)
        out["crop_%s_sums" % name] = np.asarray(sums, dtype=np.uint64)
        out["crop_%s_probe" % name] = np.float64(random.random())
        print("crops", name, "boxes", boxes[:3], "...")

    # whole items: baseline.py's train transform through the Preprocessor
    with tempfile.TemporaryDirectory(prefix="fdstage1_") as root:
        for k, name in enumerate(C.NAMES):
            Image.fromarray(C.source_image(k)).save(os.path.join(root, name), format="PNG")
            back = np.asarray(Image.open(os.path.join(root, name)).convert("RGB"), dtype=np.uint8)
            assert np.array_equal(back, C.source_image(k))
        normalizer = T.Normalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
        transform = T.Compose([T.RandomSizedRectCrop(C.H, C.W), T.RandomSizedEarser(), T.RandomHorizontalFlip(), T.ToTensor(),
                               normalizer])
        pre = P.Preprocessor(C.TRAIN, root=root, transform=transform)
        s = S.RandomPairSampler(C.TRAIN, neg_pos_ratio=C.RATIO)
        C.seed_sampler()
        pairs = np.asarray([(int(a), int(b)) for a, b in s], dtype=np.int64)
        out["pairs"] = pairs
        C.seed_items()
        sums = []
        for n, (i, j) in enumerate(pairs[:C.ITEM_PAIRS]):
            for side, (img, fname, pid, camid) in enumerate(pre[(int(i), int(j))]):
                a = img.numpy()
                assert a.dtype == np.float32 and a.shape == (3, C.H, C.W)
                assert (fname, pid, camid) == C.TRAIN[int((i, j)[side])]
                sums.append(C.byte_sum(a))
                if n < C.ITEM_FULL:
                    out["item_%d_%d" % (n, side)] = a.copy()
        out["item_sums"] = np.asarray(sums, dtype=np.uint64).reshape(-1, 2)
        out["item_probe"] = np.float64(random.random())
        out["item_torch_probe"] = np.float64(float(torch.rand(1)))
        print("items of pairs", pairs[:C.ITEM_PAIRS].tolist())
    path = os.path.join(HERE, "reference_fdstage1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
