"""FD-GAN stage II's pair loaders on the MI355X (csrc/databank.hip: rg_bank_fd_image_batch, rg_bank_fd_pose_batch):

  * the image kernel bit for bit against tests/fd_pairs_hostmodel.py at four plane sizes (16-byte rows, two element-wise tails, one
    of several blocks), N in {1, 5, 64}, with the patches planted at their edges;
  * the pose kernel bit for bit against ops.pose_maps(mode=0) + flip_images on the gathered landmarks and within 2e-7 of
    oracle.ref_datagen.o_generate_pose_map (the bound tests/test_datagen_gpu.py holds the existing kernel to);
  * DevicePairLoader against the reference's own items (tests/golden/reference_fdpairs.npz), launch accounting at the rg_hip.lib
    boundary, the allocation bound of a batch, byte-equal repeats and side-stream runs, the host check in front of the launch;
  * DeviceFDTestLoader, and a stage-2 FDGANModel fed by a loader batch.
"""
import os
import random

import numpy as np
import pytest
import torch

from tests import fd_pairs_hostmodel as HM
from tests.golden import cases_fdpairs as C

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_fdpairs.npz"))
LUT = HM.bank_lut(HM.REID_MEAN, HM.REID_STD)
M = 7
POSE_TOL = 2e-7


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


def _planes(H, W, seed=0):
    """[M, H, W, 3] uint8: plane 0 all 0, plane 1 all 255, the rest tell images, channels, rows and columns apart"""
    m, r, q, c = np.meshgrid(np.arange(M), np.arange(H), np.arange(W), np.arange(3), indexing="ij")
    a = (53 * m + 37 * r + 11 * q + 101 * c + (r * q) % 7) % 256
    a = (a + np.random.RandomState(seed).randint(0, 3, size=a.shape)) % 256
    a[0], a[1] = 0, 255
    return a.astype(np.uint8)


def _indices(N):
    """repeated and non-monotone bank rows; the all-0 and the all-255 plane among the first five"""
    return [(6, 0, 6, 1, 3, 2, 5, 4)[n % 8] if n % 11 else 4 for n in range(N)]


def _edge_draws(N, H, W):
    """(flip, 0, 0, er0, ec0, eh, ew, rgb) per sample: a patch at the origin, one that ends on the right edge, one on the bottom edge
    (where the clipped paste ends), a single pixel, a full-width one, none; colours 0, 0xFFFFFF and three distinct bytes; both flips
    in every batch of more than one sample"""
    h2, w2 = max(H // 3, 1), max(W // 3, 1)
    rects = [(0, 0, h2, w2), (1, W - w2, h2, w2), (H - h2, 1, h2, w2), (H // 2, W // 2, 1, 1), (2, 0, h2, W), (0, 0, 0, 0),
             (H - 1, W - 1, 1, 1)]
    colours = [0x030201, 0, 0xFFFFFF, 0x10F080, 0x0000FF]
    out = []
    for n in range(N):
        k = n + 1 if N > 1 else 1                        # a single sample: flipped, the patch that ends on the right edge
        out.append((k % 2, 0, 0) + rects[k % len(rects)] + (colours[(k // 2) % len(colours)],))
    return out


_IMAGE_CACHE = {}
IMAGE_SIZES = {"vec8x8": (8, 8), "tail7x6": (7, 6), "tail9x10": (9, 10), "blocks64x32": (64, 32)}
IMAGE_CASES = [(g, n) for g in IMAGE_SIZES for n in (1, 5, 64)]


def _image_case(name, N):
    """(planes, idx, draws, host-model batch), computed once per case and left unchanged"""
    if (name, N) not in _IMAGE_CACHE:
        H, W = IMAGE_SIZES[name]
        planes, idx, draws = _planes(H, W), _indices(N), _edge_draws(N, H, W)
        ref = HM.fd_image_model(planes, idx, draws, LUT)
        ref.setflags(write=False)
        _IMAGE_CACHE[(name, N)] = (planes, idx, draws, ref)
    return _IMAGE_CACHE[(name, N)]


@pytest.fixture(scope="module")
def lut(dev):
    from rg_hip import ops
    t = ops.bank_lut(HM.REID_MEAN, HM.REID_STD)
    assert t.numpy().tobytes() == LUT.tobytes()
    return t.to(dev)


@pytest.mark.parametrize("name,N", IMAGE_CASES, ids=["%s-n%d" % c for c in IMAGE_CASES])
def test_image_batch_equals_the_host_model(dev, lut, name, N):
    from rg_hip import ops
    H, W = IMAGE_SIZES[name]
    planes, idx, draws, ref = _image_case(name, N)
    if N > 1:
        assert {d[0] for d in draws} == {0, 1} and any(d[5] == 0 for d in draws) and any(d[4] + d[6] == W and d[4] > 0 for d in draws)
        assert any(d[3] + d[5] == H and d[3] > 0 for d in draws) and {0, 0xFFFFFF, 0x030201} <= {d[7] for d in draws}
    got = ops.bank_fd_image_batch(torch.from_numpy(planes).to(dev), ops.fd_draws(idx, draws), lut)
    assert got.dtype == torch.float32 and tuple(got.shape) == (N, 3, H, W)
    wrong = int((got.cpu().numpy().view(np.uint32) != ref.view(np.uint32)).sum())
    print("%s N=%d: %d of %d elements differ from the host model" % (name, N, wrong, ref.size))
    assert wrong == 0


# ---- the pose kernel ------------------------------------------------------------------------------------------------------------
def _landmarks(H, W, J=18):
    g = np.random.RandomState(4)
    t = np.stack([g.randint(0, H, size=(M, J)), g.randint(0, W, size=(M, J))], axis=2).astype(np.int64)
    t[0, :4] = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]                    # the four corners: both mirror images
    t[0, 4:8] = [(1, W // 2), (H - 2, W // 2), (H // 2, 1), (H // 2, W - 2)]         # one pixel off each border
    t[1, 3] = (-1, -1)                                                             # not detected: both, or one coordinate
    t[2, 0, 1] = -1
    t[2, 5, 0] = -1
    t[3, 1] = (H, W // 2)                                                          # a coordinate at H / W: outside, missing
    t[3, 2] = (H // 2, W)
    t[5] = -1                                                                      # an image without any joint
    return t.astype(np.int32)


POSE_CASES = [(64, 32, 7), (50, 27, 7), (256, 128, 3)]


@pytest.mark.parametrize("H,W,N", POSE_CASES)
def test_pose_batch_equals_pose_maps_then_flip_and_the_oracle(dev, H, W, N):
    from rg_hip import ops
    from reid.utils.data.device_pipeline import flip_images
    table = _landmarks(H, W)
    idx = [0, 3, 2, 0, 5, 1, 6][:N]
    pp = [(1, 4, -1, 0), (0, 5, 0, 0), (1, 6, 5, 0), (0, 6, 17, 0), (1, 5, 2, 0), (0, 4, 3, 0), (1, 5, -1, 0)][:N]
    assert {p[1] for p in pp} == {4, 5, 6} and {p[0] for p in pp} == {0, 1}
    dtable = torch.from_numpy(table).to(dev)
    got = ops.bank_fd_pose_batch(dtable, ops.fd_draws(None, None, idx, pp), H, W)
    assert got.dtype == torch.float32 and tuple(got.shape) == (N, 18, H, W)
    gathered = dtable[torch.tensor(idx, device=dev)].clone()
    for n, p in enumerate(pp):
        if p[2] >= 0:
            gathered[n, p[2]] = -1
    sig = torch.tensor([float(p[1]) for p in pp], dtype=torch.float32).to(dev)
    want = flip_images(ops.pose_maps(gathered.contiguous(), sig, H, W, mode=0), [p[0] for p in pp])
    assert _bytes(got) == _bytes(want)
    ref = HM.fd_pose_model(table, idx, pp, H, W)
    err = float(np.abs(got.cpu().numpy() - ref).max())
    print("%dx%d N=%d: max |kernel - scipy| = %.3g" % (H, W, N, err))
    assert err <= POSE_TOL
    assert np.array_equal(got.cpu().numpy() == 0, ref == 0)               # same support (4-sigma truncation, reflections)
    assert float(got[1, 0].abs().max()) == 0.0 and float(got[1, 1].abs().max()) == 0.0 and float(got[1, 2].abs().max()) == 0.0
    assert float(got[0, 0].max()) == 1.0 and float(got[2, 5].abs().max()) == 0.0


# ---- the loader on the reference's toy set --------------------------------------------------------------------------------------
def _toy_bank(dev):
    from clustercontrast.utils.data.device_bank import DeviceImageBank
    return DeviceImageBank.from_arrays(GOLD["planes"], C.NAMES, C.PIDS, C.CAMS, landmarks=GOLD["landmarks"], device=dev)


@pytest.mark.parametrize("aug", C.AUGS)
def test_pair_loader_batches_equal_the_reference_items(dev, aug):
    from reid.utils.data.device_pairs import DevicePairLoader
    B = C.ITEM_PAIRS[aug]
    loader = DevicePairLoader(_toy_bank(dev), C.TRAINVAL, C.PID_IMGS, B, neg_pos_ratio=3, pose_aug=aug)
    C.seed_sampler(3)
    C.seed_items(aug)
    first = next(iter(loader))
    assert random.random() == float(GOLD["item_%s_probe" % aug]) and float(torch.rand(1)) == float(GOLD["item_%s_torch_probe" % aug])
    for side, d in enumerate(first):
        assert all(d[k].is_cuda for k in ("origin", "target", "posemap", "pid"))
        assert d["pid"].dtype == torch.int64 and tuple(d["pid"].shape) == (B, 1)
        for n in range(B):
            key = "item_%s_%d_%d_" % (aug, n, side)
            assert _bytes(d["origin"][n]) == GOLD[key + "origin"].tobytes(), key
            assert _bytes(d["target"][n]) == GOLD[key + "target"].tobytes(), key
            maps = d["posemap"][n].cpu().numpy()
            err = float(np.abs(maps[:, ::C.MAP_STRIDE, ::C.MAP_STRIDE] - GOLD[key + "posemap"]).max())
            serr = float(np.abs(maps.astype(np.float64).sum((1, 2)) - GOLD[key + "posemap_sum"]).max())
            print("%s: max |map - reference| %.3g, max |sum - reference| %.3g" % (key, err, serr))
            assert err <= POSE_TOL and serr <= POSE_TOL * C.H * C.W, key
            assert d["pid"][n].tolist() == GOLD[key + "pid"].tolist(), key


def test_pair_loader_two_epochs_equal_the_reference_pair_lists(dev):
    from reid.utils.data.device_pairs import DevicePairLoader
    loader = DevicePairLoader(_toy_bank(dev), C.TRAINVAL, C.PID_IMGS, 16, neg_pos_ratio=3)
    seen, inner = [], loader._batch
    loader._batch = lambda pairs: seen.append(list(pairs)) or inner(pairs)
    C.seed_sampler(3)
    for epoch in range(2):
        del seen[:]
        sizes = [b[0]["origin"].shape[0] for b in loader]
        assert sizes == [16, 16, 8] and len(loader) == 3
        assert sum(seen, []) == [tuple(p) for p in GOLD["pairs_r3_e%d" % epoch].tolist()], epoch


def _count_all(monkeypatch):
    from rg_hip.lib import lib
    from tests.test_mp_models_gpu import _wrap
    lib.load()
    return _wrap(monkeypatch, lib, [n for n in lib.protos if n not in ("rg_last_error",)])


def test_launch_accounting(dev, monkeypatch):
    """at the rg_hip.lib boundary a batch is ONE image launch and ONE pose launch; a test batch one ReID gather"""
    from reid.utils.data.device_pairs import DeviceFDTestLoader, DevicePairLoader
    bank = _toy_bank(dev)
    loader = DevicePairLoader(bank, C.TRAINVAL, C.PID_IMGS, 4, pose_aug="gauss")
    it = iter(loader)
    calls = _count_all(monkeypatch)
    for _ in range(2):
        next(it)
        n = {k: len(v) for k, v in calls.items() if v}
        assert n == {"rg_bank_fd_image_batch": 1, "rg_bank_fd_pose_batch": 1}, n
        for v in calls.values():
            del v[:]
    assert len(list(DeviceFDTestLoader(bank, C.TRAINVAL, 4))) == 3
    n = {k: len(v) for k, v in calls.items() if v}
    assert n == {"rg_bank_reid_batch": 3}, n


def test_allocation_bound(dev):
    """the device memory a batch takes is its two output allocations plus the packed draws and the pids: no intermediate batch"""
    from reid.utils.data.device_pairs import DevicePairLoader
    B = 2                                                        # every tensor below 1 MiB: the allocator splits its blocks exactly
    loader = DevicePairLoader(_toy_bank(dev), C.TRAINVAL, C.PID_IMGS, B, pose_aug="erase")
    it = iter(loader)
    out = next(it)                                               # table uploaded, library loaded
    del out
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    d1, d2 = next(it)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base

    def block(nbytes):                                           # the caching allocator hands out multiples of 512 bytes
        return -(-nbytes // 512) * 512
    assert d1["origin"].untyped_storage().data_ptr() == d2["target"].untyped_storage().data_ptr()           # one allocation of four views
    assert d1["posemap"].untyped_storage().data_ptr() == d2["posemap"].untyped_storage().data_ptr()
    returned = block(4 * B * 3 * C.H * C.W * 4) + block(2 * B * C.J * C.H * C.W * 4)
    small = block((9 * 4 * B + 5 * 2 * B) * 4) + block(2 * B * 8)          # int32 draws + rows of both launches, int64 pids
    print("batch: peak %d bytes over the baseline; returned %d, parameters %d" % (peak, returned, small))
    assert peak <= returned + small
    assert d1["origin"].numel() * 4 > small                       # an fp32 intermediate would not fit under the bound


def test_outputs_are_reproducible_and_stream_independent(dev, lut):
    from rg_hip import ops
    planes, idx, draws, ref = _image_case("blocks64x32", 5)
    bank = torch.from_numpy(planes).to(dev)
    table = torch.from_numpy(_landmarks(64, 32)).to(dev)
    d = ops.fd_draws(idx, draws, [0, 3, 2, 6], [(1, 4, -1, 0), (0, 5, 0, 0), (1, 6, 5, 0), (0, 5, -1, 0)], device=dev)

    def run():
        return ops.bank_fd_image_batch(bank, d, lut), ops.bank_fd_pose_batch(table, d, 64, 32)
    first = [_bytes(t) for t in run()]
    assert first[0] == ref.tobytes()
    assert [_bytes(t) for t in run()] == first
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = run()
    side.synchronize()
    assert [_bytes(t) for t in out] == first


def test_bad_draws_never_reach_the_device(dev, lut, monkeypatch):
    from rg_hip import ops
    bank = torch.from_numpy(_planes(8, 8)).to(dev)
    table = torch.from_numpy(_landmarks(64, 32)).to(dev)
    calls = _count_all(monkeypatch)
    good = (1, 0, 0, 2, 1, 3, 2, 0x123456)
    for idx, row in [(7, good), (-1, good), (0, (2, 0, 0, 0, 0, 0, 0, 0)), (0, (0, 0, 0, 6, 0, 3, 2, 0)), (0, (0, 0, 0, 0, 7, 3, 2, 0)),
                     (0, (0, 0, 0, -1, 0, 3, 2, 0)), (0, (0, 0, 0, 0, 0, 3, 0, 0)), (0, (0, 0, 0, 0, 0, 0, 0, 2 ** 24)),
                     (0, (0, 0, 0, 0, 0, 0, 0, -1))]:
        with pytest.raises(ValueError):
            ops.bank_fd_image_batch(bank, ops.fd_draws([0, idx], [good, row]), lut)
    goodp = (1, 5, 3, 0)
    for idx, row in [(7, goodp), (-1, goodp), (0, (2, 5, 3, 0)), (0, (0, 0, 3, 0)), (0, (0, 9, 3, 0)), (0, (0, 5, 18, 0)),
                     (0, (0, 5, -2, 0))]:
        with pytest.raises(ValueError):
            ops.bank_fd_pose_batch(table, ops.fd_draws(None, None, [0, idx], [goodp, row]), 64, 32)      # sigma 9: radius 36 > 32
    with pytest.raises(ValueError):
        ops.bank_fd_pose_batch(table, ops.fd_draws(None, None, [0], [goodp]), 2048, 32)
    with pytest.raises(ValueError):
        ops.bank_fd_image_batch(bank, ops.fd_draws(None, None, [0], [goodp]), lut)                       # no image rows
    with pytest.raises(TypeError):
        ops.bank_fd_image_batch(bank, ops.bank_draws([0], None), lut)
    assert not any(calls.values()), {k: len(v) for k, v in calls.items() if v}


def test_fd_test_loader_equals_the_host_model(dev):
    from reid.utils.data.device_pairs import DeviceFDTestLoader
    entries = [C.TRAINVAL[k] for k in (7, 0, 3, 3, 9, 1, 8)]
    batches = list(DeviceFDTestLoader(_toy_bank(dev), entries, 3))
    assert [b[0].shape[0] for b in batches] == [3, 3, 1] and all(len(b) == 4 for b in batches)
    assert _bytes(torch.cat([b[0] for b in batches])) == HM.ordered_batch(GOLD["planes"], [7, 0, 3, 3, 9, 1, 8], LUT).tobytes()
    assert sum((b[1] for b in batches), []) == [e[0] for e in entries]
    assert torch.cat([b[2] for b in batches]).tolist() == [e[1] for e in entries]
    assert torch.cat([b[3] for b in batches]).tolist() == [e[2] for e in entries]


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def test_fdgan_step_fed_by_the_pair_loader(dev):
    """set_input(batch) on a stage-2 FDGANModel at 2 pairs of 256x128: the model's tensors are the host model's composition of the
    same draws, and one optimize_parameters() ends with finite losses"""
    from clustercontrast.utils.data.device_bank import DeviceImageBank
    from fdgan.model import FDGANModel
    from reid.utils.data.device_pairs import DevicePairLoader
    from tests.test_paths_gpu import _fd_opt
    H, W, J, B = 256, 128, 18, 2
    g = np.random.RandomState(11)
    pids = [4, 4, 15, 15, 15, 123, 123]
    names = ["%08d_%02d_%04d.jpg" % (p, k % 3, k) for k, p in enumerate(pids)]
    trainval = [(n, p, k % 3) for k, (n, p) in enumerate(zip(names, pids))]
    pid_imgs = {}
    for n, p in zip(names, pids):
        pid_imgs.setdefault(p, []).append(n)
    planes = g.randint(0, 256, size=(len(pids), H, W, 3)).astype(np.uint8)
    table = np.stack([g.randint(0, H, size=(len(pids), J)), g.randint(0, W, size=(len(pids), J))], axis=2).astype(np.int32)
    table[:, 7] = -1
    bank = DeviceImageBank.from_arrays(planes, names, pids, [k % 3 for k in range(len(pids))], landmarks=table, device=dev)
    loader = DevicePairLoader(bank, trainval, pid_imgs, B, neg_pos_ratio=3, pose_aug="gauss")
    np.random.seed(5)
    random.seed(6)
    torch.manual_seed(7)
    batch = next(iter(loader))
    # the host model: the same pairs, the same draws
    np.random.seed(5)
    random.seed(6)
    torch.manual_seed(7)
    pairs = HM.pair_list(trainval, 3)[1][:B]
    items = [[HM.item(planes, table, trainval, pid_imgs, i, "gauss", LUT) for i in pair] for pair in pairs]
    side = [{k: np.stack([items[n][s][k] for n in range(B)]) for k in ("origin", "target", "posemap", "pid")} for s in (0, 1)]
    labels = (side[0]["pid"] == side[1]["pid"]).reshape(-1)
    assert labels.tolist() == [1, 0]                                  # the positive pair, then a negative
    want_origin = np.concatenate([side[0]["origin"], side[1]["origin"]])
    want_target = np.concatenate([side[0]["target"], np.where(labels[:, None, None, None], side[0]["target"], side[1]["target"])])
    want_pose = np.concatenate([side[0]["posemap"], np.where(labels[:, None, None, None], side[0]["posemap"], side[1]["posemap"])])

    torch.manual_seed(1)
    model = FDGANModel(_fd_opt(B, arch="resnet50"))
    model.reset_model_status()
    model.set_input(batch)
    assert _bytes(model.origin) == want_origin.tobytes() and _bytes(model.target) == want_target.tobytes()
    err = float(np.abs(model.posemap.cpu().numpy() - want_pose).max())
    print("posemap: max |model input - host model| = %.3g" % err)
    assert err <= POSE_TOL and tuple(model.posemap.shape) == (2 * B, J, H, W)
    assert model.labels.view(-1).cpu().tolist() == [1, 0]
    model.optimize_parameters()
    errors = model.get_current_errors()
    print("losses", {k: round(float(v), 5) for k, v in errors.items()})
    assert errors and all(np.isfinite(float(v)) for v in errors.values())
