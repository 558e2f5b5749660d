"""Device-resident image bank (csrc/databank.hip): finished fp32 batches gathered from uint8 planes that stay in HBM.

The indices and the augmentation draws are made on the host.  `bank_draws` packs them into ONE int32 host buffer (params [N, 8]
followed by idx [N]) that crosses to the device in one copy; the three batch wrappers check the HOST copy against the geometry
they are about to launch with and raise ValueError before anything is enqueued — a bad draw never reaches the device.

FD-GAN stage II's two entries follow the same rule with a buffer of their own shape: `fd_draws` packs the image rows' params and
indices and the map rows' pose params and indices into one int32 buffer (`FDDraws`), checked by `bank_fd_image_batch` and
`bank_fd_pose_batch` before they launch.

FD-GAN stage I reads a RAW bank (every image at its own size) and resamples the drawn box in the kernel: `fd_crop_draws` packs the
rows, boxes, flips and patches into one int32 buffer [N, 12] (`FDCropDraws`), checked by `bank_fd_crop_batch` against the host copy
of the bank's size table before it launches."""
from __future__ import absolute_import

import torch

from ._base import _chk, _chk_rr, _p, _stream, lib


def bank_lut(mean, std):
    """[3, 256] fp32 host table: ToTensor + Normalize of every byte value, in exactly the reference's arithmetic
    (`img.float().div(255)` then `sub_(mean).div_(std)`, both in fp32)."""
    v = torch.arange(256, dtype=torch.float32).div(255)
    m = torch.as_tensor(mean, dtype=torch.float32).view(-1, 1)
    s = torch.as_tensor(std, dtype=torch.float32).view(-1, 1)
    if m.numel() != 3 or s.numel() != 3:
        raise ValueError("bank_lut: three means and three standard deviations expected")
    return v.view(1, 256).sub(m).div(s).contiguous()


class BankDraws(object):
    """One batch's bank rows and draws: `idx` int32 [N] and `params` int32 [N, 8] = (flip, top, left, er0, ec0, eh, ew, 0) as
    views of one host buffer, and (after `to`) the same two views of its single device copy."""

    __slots__ = ("host", "idx", "params", "idx_dev", "params_dev", "_ok")

    def __init__(self, idx, params):
        idx = torch.as_tensor(idx).reshape(-1)
        n = idx.numel()
        if n == 0:
            raise ValueError("bank_draws: an empty batch")
        if idx.is_cuda or idx.dtype not in (torch.int32, torch.int64):
            raise ValueError("bank_draws: idx must be a host tensor of int32 / int64 (the draws are checked on the host)")
        if n and (int(idx.min()) < -2 ** 31 or int(idx.max()) >= 2 ** 31):
            raise ValueError("bank_draws: idx does not fit int32")
        host = self.host = torch.zeros(n * 9, dtype=torch.int32)
        self.params, self.idx = host[:n * 8].view(n, 8), host[n * 8:]
        self.idx.copy_(idx)
        if params is not None:
            params = torch.as_tensor(params)
            if params.is_cuda or params.dtype not in (torch.int32, torch.int64) or params.dim() != 2 or params.shape[0] != n \
                    or params.shape[1] not in (7, 8):
                raise ValueError("bank_draws: params must be a host integer tensor [N, 7] or [N, 8]")
            if params.numel() and (int(params.min()) < -2 ** 31 or int(params.max()) >= 2 ** 31):
                raise ValueError("bank_draws: params do not fit int32")
            self.params[:, :params.shape[1]].copy_(params)
        self.idx_dev = self.params_dev = None
        self._ok = set()

    def to(self, device):
        """the one host->device copy of the batch"""
        n = self.idx.numel()
        dev = self.host.to(device, non_blocking=True)
        self.params_dev, self.idx_dev = dev[:n * 8].view(n, 8), dev[n * 8:]
        return self

    def check(self, who, M, geometry=None):
        """ValueError unless 0 <= idx < M, flip in {0, 1} and, with geometry = (Hs, Ws, H, W, pad), 0 <= top <= 2 pad + Hs - H,
        0 <= left <= 2 pad + Ws - W and every rectangle (eh > 0) has ew > 0 and lies inside [0, H) x [0, W)."""
        key = (M, geometry)
        if key in self._ok:
            return
        idx, p = self.idx, self.params
        if int(idx.min()) < 0 or int(idx.max()) >= M:
            raise ValueError("%s: bank row index outside [0, %d)" % (who, M))
        if bool(((p[:, 0] != 0) & (p[:, 0] != 1)).any()):
            raise ValueError("%s: flip must be 0 or 1" % who)
        if geometry is not None:
            Hs, Ws, H, W, pad = geometry
            if bool(((p[:, 1] < 0) | (p[:, 1] > 2 * pad + Hs - H)).any()):
                raise ValueError("%s: top outside [0, %d]" % (who, 2 * pad + Hs - H))
            if bool(((p[:, 2] < 0) | (p[:, 2] > 2 * pad + Ws - W)).any()):
                raise ValueError("%s: left outside [0, %d]" % (who, 2 * pad + Ws - W))
            er0, ec0, eh, ew = p[:, 3].long(), p[:, 4].long(), p[:, 5].long(), p[:, 6].long()
            if bool((eh < 0).any()) or bool((ew < 0).any()):
                raise ValueError("%s: negative erase rectangle size" % who)
            on = eh > 0
            if bool((on & ((ew <= 0) | (er0 < 0) | (ec0 < 0) | (er0 + eh > H) | (ec0 + ew > W))).any()):
                raise ValueError("%s: erase rectangle outside the %dx%d output" % (who, H, W))
        self._ok.add(key)


def bank_draws(idx, params=None, device=None):
    """BankDraws of host `idx` [N] and `params` [N, 8] (None: all zero, the test-time transform), uploaded when `device` is given."""
    d = BankDraws(idx, params)
    return d if device is None else d.to(device)


def _chk_bank(who, bank_u8):
    if not torch.is_tensor(bank_u8) or bank_u8.dtype != torch.uint8 or bank_u8.dim() != 4 or bank_u8.shape[3] != 3:
        raise ValueError("%s: the bank must be a uint8 tensor [M, H, W, 3]" % who)
    return _chk_rr(bank_u8, "bank", dtype=torch.uint8, dim=4)


def _chk_draws(who, draws, device):
    if not isinstance(draws, BankDraws):
        raise TypeError("%s: draws must come from ops.bank_draws (they are checked on the host before the launch)" % who)
    if draws.idx_dev is None:
        draws.to(device)
    if draws.idx_dev.device != device:
        raise RuntimeError("%s: the draws were uploaded to %s, the bank lives on %s" % (who, draws.idx_dev.device, device))
    return draws


def _chk_lut(who, lut):
    lut = _chk(lut, "lut")
    if tuple(lut.shape) != (3, 256):
        raise ValueError("%s: lut must be [3, 256]" % who)
    return lut


def bank_reid_batch(bank_u8, draws, lut, fill, out_hw, pad=0):
    """[N, 3, H, W] fp32: Pad(pad) -> RandomCrop((H, W)) -> ToTensor -> Normalize -> RandomErasing -> flip of the bank rows
    draws.idx with draws.params [N, 8] = (flip, top, left, er0, ec0, eh, ew, -); one launch (rg_bank_reid_batch)."""
    bank_u8 = _chk_bank("bank_reid_batch", bank_u8)
    M, Hs, Ws = bank_u8.shape[0], bank_u8.shape[1], bank_u8.shape[2]
    H, W = int(out_hw[0]), int(out_hw[1])
    pad = int(pad)
    if pad < 0 or H <= 0 or W <= 0 or H > Hs + 2 * pad or W > Ws + 2 * pad:
        raise ValueError("bank_reid_batch: crop %dx%d does not fit the %dx%d plane padded by %d" % (H, W, Hs, Ws, pad))
    draws = _chk_draws("bank_reid_batch", draws, bank_u8.device)
    draws.check("bank_reid_batch", M, (Hs, Ws, H, W, pad))
    lut = _chk_lut("bank_reid_batch", lut)
    fill = _chk(fill, "fill")
    if fill.numel() != 3:
        raise ValueError("bank_reid_batch: three fill values expected")
    N = draws.idx.numel()
    out = torch.empty((N, 3, H, W), dtype=torch.float32, device=bank_u8.device)
    lib.rg_bank_reid_batch(_p(bank_u8), M, Hs, Ws, _p(draws.idx_dev), _p(draws.params_dev), _p(lut), _p(fill), _p(out), N, H, W, pad,
                           _stream())
    return out


def bank_gan_batch(bank_u8, draws, lut):
    """[N, 3, Hg, Wg] fp32: ToTensor -> Normalize -> flip of the bank rows draws.idx (flip = draws.params[:, 0]); one launch."""
    bank_u8 = _chk_bank("bank_gan_batch", bank_u8)
    M, Hg, Wg = bank_u8.shape[0], bank_u8.shape[1], bank_u8.shape[2]
    draws = _chk_draws("bank_gan_batch", draws, bank_u8.device)
    draws.check("bank_gan_batch", M)
    lut = _chk_lut("bank_gan_batch", lut)
    N = draws.idx.numel()
    out = torch.empty((N, 3, Hg, Wg), dtype=torch.float32, device=bank_u8.device)
    lib.rg_bank_gan_batch(_p(bank_u8), M, Hg, Wg, _p(draws.idx_dev), _p(draws.params_dev), 8, _p(lut), _p(out), N, _stream())
    return out


def bank_pose_batch(centres, draws, height, width, sigma=6.0):
    """[N, J, Hg, Wg] fp32 pose maps of the bank rows draws.idx from the int32 centre table [M, J, 2] (INT32_MIN: missing joint),
    flipped where draws.params[:, 0] is set: pose_maps(mode=1) + flip_images on the gathered centres, in one launch."""
    if not torch.is_tensor(centres) or centres.dtype != torch.int32 or centres.dim() != 3 or centres.shape[2] != 2:
        raise ValueError("bank_pose_batch: centres must be an int32 tensor [M, J, 2]")
    centres = _chk_rr(centres, "centres", dtype=torch.int32, dim=3)
    M, J = centres.shape[0], centres.shape[1]
    height, width = int(height), int(width)
    if not (0 < height <= 1024 and 0 < width <= 1024):
        raise ValueError("bank_pose_batch: map size must be within 1024x1024")
    if not float(sigma) > 0:
        raise ValueError("bank_pose_batch: sigma must be positive")
    draws = _chk_draws("bank_pose_batch", draws, centres.device)
    draws.check("bank_pose_batch", M)
    N = draws.idx.numel()
    if N > 65535:
        raise ValueError("bank_pose_batch: at most 65535 samples per launch")
    out = torch.empty((N, J, height, width), dtype=torch.float32, device=centres.device)
    lib.rg_bank_pose_batch(_p(centres), M, J, _p(draws.idx_dev), _p(draws.params_dev), 8, float(sigma), _p(out), N, height, width,
                           _stream())
    return out


# ---- FD-GAN stage II: rg_bank_fd_image_batch / rg_bank_fd_pose_batch ------------------------------------------------------------
class FDDraws(object):
    """One FD-GAN batch's rows and draws in ONE int32 host buffer, [params [Ni, 8] | idx [Ni] | pose_params [Np, 4] | pose_idx [Np]]:
    `params` = (flip, 0, 0, er0, ec0, eh, ew, rgb) per image row, `pose_params` = (flip, sigma, erased joint or -1, 0) per map row
    (either part may be empty), and after `to` the same four views of its single device copy."""

    __slots__ = ("host", "idx", "params", "pose_idx", "pose_params", "idx_dev", "params_dev", "pose_idx_dev", "pose_params_dev", "_ok")

    @staticmethod
    def _ints(who, t, cols):
        t = torch.as_tensor(t)
        if t.numel() == 0:
            t = torch.zeros((0,) if cols is None else (0, cols), dtype=torch.int64)
        if t.is_cuda or t.dtype not in (torch.int32, torch.int64):
            raise ValueError("fd_draws: %s must be a host tensor of int32 / int64 (the draws are checked on the host)" % who)
        if cols is None:
            t = t.reshape(-1)
        elif t.dim() != 2 or t.shape[1] != cols:
            raise ValueError("fd_draws: %s must be [N, %d]" % (who, cols))
        if t.numel() and (int(t.min()) < -2 ** 31 or int(t.max()) >= 2 ** 31):
            raise ValueError("fd_draws: %s does not fit int32" % who)
        return t

    def __init__(self, idx=None, params=None, pose_idx=None, pose_params=None):
        idx = self._ints("idx", [] if idx is None else idx, None)
        pose_idx = self._ints("pose_idx", [] if pose_idx is None else pose_idx, None)
        ni, npose = idx.numel(), pose_idx.numel()
        if ni + npose == 0:
            raise ValueError("fd_draws: an empty batch")
        host = self.host = torch.zeros(ni * 9 + npose * 5, dtype=torch.int32)
        self.params, self.idx = host[:ni * 8].view(ni, 8), host[ni * 8:ni * 9]
        self.pose_params, self.pose_idx = host[ni * 9:ni * 9 + npose * 4].view(npose, 4), host[ni * 9 + npose * 4:]
        self.idx.copy_(idx)
        self.pose_idx.copy_(pose_idx)
        if params is not None:
            params = self._ints("params", params, 8)
            if params.shape[0] != ni:
                raise ValueError("fd_draws: %d rows of params for %d image rows" % (params.shape[0], ni))
            self.params.copy_(params)
        if pose_params is not None:
            pose_params = self._ints("pose_params", pose_params, 4)
            if pose_params.shape[0] != npose:
                raise ValueError("fd_draws: %d rows of pose_params for %d map rows" % (pose_params.shape[0], npose))
            self.pose_params.copy_(pose_params)
        elif npose:
            raise ValueError("fd_draws: pose_idx without pose_params (sigma has no default)")
        self.idx_dev = self.params_dev = self.pose_idx_dev = self.pose_params_dev = None
        self._ok = set()

    def to(self, device):
        """the one host->device copy of the batch"""
        ni, npose = self.idx.numel(), self.pose_idx.numel()
        dev = self.host.to(device, non_blocking=True)
        self.params_dev, self.idx_dev = dev[:ni * 8].view(ni, 8), dev[ni * 8:ni * 9]
        self.pose_params_dev, self.pose_idx_dev = dev[ni * 9:ni * 9 + npose * 4].view(npose, 4), dev[ni * 9 + npose * 4:]
        return self

    def check_images(self, who, M, H, W):
        """ValueError unless there is an image row, 0 <= idx < M, flip in {0, 1}, every rectangle (eh > 0) has ew > 0 and lies inside
        [0, H) x [0, W), and 0 <= rgb < 2^24."""
        key = ("image", M, H, W)
        if key in self._ok:
            return
        idx, p = self.idx, self.params
        if idx.numel() == 0:
            raise ValueError("%s: the draws hold no image rows" % who)
        if int(idx.min()) < 0 or int(idx.max()) >= M:
            raise ValueError("%s: bank row index outside [0, %d)" % (who, M))
        if bool(((p[:, 0] != 0) & (p[:, 0] != 1)).any()):
            raise ValueError("%s: flip must be 0 or 1" % who)
        er0, ec0, eh, ew = p[:, 3].long(), p[:, 4].long(), p[:, 5].long(), p[:, 6].long()
        if bool((eh < 0).any()) or bool((ew < 0).any()):
            raise ValueError("%s: negative patch size" % who)
        on = eh > 0
        if bool((on & ((ew <= 0) | (er0 < 0) | (ec0 < 0) | (er0 + eh > H) | (ec0 + ew > W))).any()):
            raise ValueError("%s: patch outside the %dx%d plane" % (who, H, W))
        if bool(((p[:, 7] < 0) | (p[:, 7] >= 2 ** 24)).any()):
            raise ValueError("%s: rgb must be R | G << 8 | B << 16 in [0, 2^24)" % who)
        self._ok.add(key)

    def check_poses(self, who, M, J, H, W):
        """ValueError unless there is a map row, at most 65535 of them, 0 <= pose_idx < M, flip in {0, 1}, sigma >= 1 with
        int(4 sigma + 0.5) <= min(H, W) (the closed form holds the first mirror image only) and -1 <= erased joint < J."""
        key = ("pose", M, J, H, W)
        if key in self._ok:
            return
        idx, p = self.pose_idx, self.pose_params
        if idx.numel() == 0:
            raise ValueError("%s: the draws hold no map rows" % who)
        if idx.numel() > 65535:
            raise ValueError("%s: at most 65535 samples per launch" % who)
        if int(idx.min()) < 0 or int(idx.max()) >= M:
            raise ValueError("%s: landmark row index outside [0, %d)" % (who, M))
        if bool(((p[:, 0] != 0) & (p[:, 0] != 1)).any()):
            raise ValueError("%s: flip must be 0 or 1" % who)
        sig = p[:, 1].long()
        if bool((sig < 1).any()):
            raise ValueError("%s: sigma must be an integer >= 1" % who)
        if int(4.0 * int(sig.max()) + 0.5) > min(H, W):
            raise ValueError("%s: sigma %d needs a radius of %d > min(%d, %d): only the first mirror image is modelled"
                             % (who, int(sig.max()), int(4.0 * int(sig.max()) + 0.5), H, W))
        if bool(((p[:, 2] < -1) | (p[:, 2] >= J)).any()):
            raise ValueError("%s: erased joint outside [-1, %d)" % (who, J))
        self._ok.add(key)


def fd_draws(idx=None, params=None, pose_idx=None, pose_params=None, device=None):
    """FDDraws of host image rows `idx` [Ni] with `params` [Ni, 8] (None: all zero) and map rows `pose_idx` [Np] with `pose_params`
    [Np, 4], uploaded when `device` is given."""
    d = FDDraws(idx, params, pose_idx, pose_params)
    return d if device is None else d.to(device)


def _chk_fd_draws(who, draws, device):
    if not isinstance(draws, FDDraws):
        raise TypeError("%s: draws must come from ops.fd_draws (they are checked on the host before the launch)" % who)
    if draws.idx_dev is None:
        draws.to(device)
    if draws.idx_dev.device != device:
        raise RuntimeError("%s: the draws were uploaded to %s, the bank lives on %s" % (who, draws.idx_dev.device, device))
    return draws


def bank_fd_image_batch(bank_u8, draws, lut):
    """[Ni, 3, H, W] fp32: FD-GAN stage II's RectScale'd planes `bank_u8` [M, H, W, 3] -> RandomSizedEarser's colour patch (on the
    bytes) -> flip -> ToTensor -> Normalize of the rows draws.idx with draws.params [Ni, 8] = (flip, 0, 0, er0, ec0, eh, ew, rgb);
    one launch (rg_bank_fd_image_batch)."""
    if not torch.is_tensor(bank_u8) or bank_u8.dtype != torch.uint8 or bank_u8.dim() != 4 or bank_u8.shape[3] != 3:
        raise ValueError("bank_fd_image_batch: the bank must be a uint8 tensor [M, H, W, 3]")
    M, H, W = bank_u8.shape[0], bank_u8.shape[1], bank_u8.shape[2]
    if not isinstance(draws, FDDraws):
        raise TypeError("bank_fd_image_batch: draws must come from ops.fd_draws (they are checked on the host before the launch)")
    draws.check_images("bank_fd_image_batch", M, H, W)           # the draws first: a bad one is refused wherever the bank lives
    bank_u8 = _chk_bank("bank_fd_image_batch", bank_u8)
    draws = _chk_fd_draws("bank_fd_image_batch", draws, bank_u8.device)
    lut = _chk_lut("bank_fd_image_batch", lut)
    N = draws.idx.numel()
    out = torch.empty((N, 3, H, W), dtype=torch.float32, device=bank_u8.device)
    lib.rg_bank_fd_image_batch(_p(bank_u8), M, H, W, _p(draws.idx_dev), _p(draws.params_dev), _p(lut), _p(out), N, _stream())
    return out


def bank_fd_pose_batch(landmarks, draws, height, width):
    """[Np, J, H, W] fp32 FD-GAN pose maps of the rows draws.pose_idx of the int32 landmark table [M, J, 2] = (row, col) (-1: not
    detected) with draws.pose_params [Np, 4] = (flip, sigma, erased joint or -1, 0): pose_maps(mode=0) + flip_images on the gathered
    landmarks, in one launch (rg_bank_fd_pose_batch)."""
    if not torch.is_tensor(landmarks) or landmarks.dtype != torch.int32 or landmarks.dim() != 3 or landmarks.shape[2] != 2:
        raise ValueError("bank_fd_pose_batch: landmarks must be an int32 tensor [M, J, 2]")
    M, J = landmarks.shape[0], landmarks.shape[1]
    height, width = int(height), int(width)
    if not (0 < height <= 1024 and 0 < width <= 1024):
        raise ValueError("bank_fd_pose_batch: map size must be within 1024x1024")
    if not isinstance(draws, FDDraws):
        raise TypeError("bank_fd_pose_batch: draws must come from ops.fd_draws (they are checked on the host before the launch)")
    draws.check_poses("bank_fd_pose_batch", M, J, height, width)
    landmarks = _chk_rr(landmarks, "landmarks", dtype=torch.int32, dim=3)
    draws = _chk_fd_draws("bank_fd_pose_batch", draws, landmarks.device)
    N = draws.pose_idx.numel()
    out = torch.empty((N, J, height, width), dtype=torch.float32, device=landmarks.device)
    lib.rg_bank_fd_pose_batch(_p(landmarks), M, J, _p(draws.pose_idx_dev), _p(draws.pose_params_dev), _p(out), N, height, width,
                              _stream())
    return out


# ---- FD-GAN stage I: rg_bank_fd_crop_batch --------------------------------------------------------------------------------------
FD_CROP_WHOLE, FD_CROP_STRIPS = 0, 1
FD_CROP_INTS = 12


def fd_crop_strip_width(hmax, width):
    """output columns a workgroup of rg_bank_fd_crop_batch takes for crops of up to `hmax` rows: `width` (whole samples) or a
    smaller multiple of 4 (strips); ValueError where width is no multiple of 4 or no strip fits the LDS tile"""
    sw = int(lib.rg_bank_fd_crop_regime(int(hmax), int(width)))
    if sw < 4:
        raise ValueError("bank_fd_crop_batch: output width %d must be a multiple of 4 and 12 x %d bytes must fit the LDS tile"
                         % (int(width), int(hmax)))
    return sw


def fd_crop_regime(hmax, width):
    """the form `bank_fd_crop_batch` takes for crops of up to `hmax` rows at this output width: FD_CROP_WHOLE (a workgroup
    resamples a whole sample: outputs up to 32 columns wide) or FD_CROP_STRIPS (a strip of at most 32 output columns, fewer where
    the LDS tile of `hmax` rows is the limit)"""
    return FD_CROP_WHOLE if fd_crop_strip_width(hmax, width) == int(width) else FD_CROP_STRIPS


class FDCropDraws(object):
    """One stage-I batch's rows and draws in ONE int32 host buffer [N, 12] = (bank row, x1, y1, w, h, flip, er0, ec0, eh, ew, rgb,
    0), and (after `to`) its single device copy."""

    __slots__ = ("host", "dev")

    def __init__(self, rows):
        rows = torch.as_tensor(rows)
        if rows.is_cuda or rows.dtype not in (torch.int32, torch.int64):
            raise ValueError("fd_crop_draws: the draws must be a host tensor of int32 / int64 (they are checked on the host)")
        if rows.dim() != 2 or rows.shape[1] != 11 or rows.shape[0] == 0:
            raise ValueError("fd_crop_draws: the draws must be [N, 11] with N > 0, got %s" % (tuple(rows.shape),))
        if int(rows.min()) < -2 ** 31 or int(rows.max()) >= 2 ** 31:
            raise ValueError("fd_crop_draws: the draws do not fit int32")
        self.host = torch.zeros((rows.shape[0], FD_CROP_INTS), dtype=torch.int32)
        self.host[:, :11].copy_(rows)
        self.dev = None

    def to(self, device):
        """the one host->device copy of the batch"""
        self.dev = self.host.to(device, non_blocking=True)
        return self

    def check(self, who, sizes, H, W):
        """ValueError unless, against the HOST size table `sizes` int [M, 2] = (H_m, W_m): 0 <= row < M, 1 <= w, 1 <= h, x1 >= 0,
        y1 >= 0, x1 + w <= W_m, y1 + h <= H_m, flip in {0, 1}, every patch (eh > 0) has ew > 0 and lies inside [0, H) x [0, W),
        and 0 <= rgb < 2^24."""
        p = self.host.long()
        M = int(sizes.shape[0])
        if int(p[:, 0].min()) < 0 or int(p[:, 0].max()) >= M:
            raise ValueError("%s: bank row index outside [0, %d)" % (who, M))
        hw = torch.as_tensor(sizes).long()[p[:, 0]]
        x1, y1, w, h = p[:, 1], p[:, 2], p[:, 3], p[:, 4]
        if bool(((w < 1) | (h < 1) | (x1 < 0) | (y1 < 0) | (x1 + w > hw[:, 1]) | (y1 + h > hw[:, 0])).any()):
            raise ValueError("%s: crop box outside its image" % who)
        if bool(((p[:, 5] != 0) & (p[:, 5] != 1)).any()):
            raise ValueError("%s: flip must be 0 or 1" % who)
        er0, ec0, eh, ew = p[:, 6], p[:, 7], p[:, 8], p[:, 9]
        if bool((eh < 0).any()) or bool((ew < 0).any()):
            raise ValueError("%s: negative patch size" % who)
        if bool(((eh > 0) & ((ew <= 0) | (er0 < 0) | (ec0 < 0) | (er0 + eh > H) | (ec0 + ew > W))).any()):
            raise ValueError("%s: patch outside the %dx%d output" % (who, H, W))
        if bool(((p[:, 10] < 0) | (p[:, 10] >= 2 ** 24)).any()):
            raise ValueError("%s: rgb must be R | G << 8 | B << 16 in [0, 2^24)" % who)


def fd_crop_draws(rows, device=None):
    """FDCropDraws of host `rows` [N, 11] = (bank row, x1, y1, w, h, flip, er0, ec0, eh, ew, rgb), uploaded when `device` is given."""
    d = FDCropDraws(rows)
    return d if device is None else d.to(device)


def bank_fd_crop_batch(raw, draws, lut):
    """[N, 3, H, W] fp32: FD-GAN stage I's RandomSizedRectCrop (crop, then PIL's bilinear resize to raw.size = (H, W), in integers)
    -> RandomSizedEarser's colour patch (on the bytes) -> flip -> ToTensor -> Normalize of the images of the raw bank `raw`
    (DeviceRawBank: data, offsets, sizes, sizes_host, table_x, table_y, size) named by draws.host [N, 12]; one launch
    (rg_bank_fd_crop_batch)."""
    H, W = int(raw.size[0]), int(raw.size[1])
    if not isinstance(draws, FDCropDraws):
        raise TypeError("bank_fd_crop_batch: draws must come from ops.fd_crop_draws (they are checked on the host before the launch)")
    draws.check("bank_fd_crop_batch", raw.sizes_host, H, W)      # the draws first: a bad one is refused wherever the bank lives
    data = _chk_rr(raw.data, "raw bank", dtype=torch.uint8, dim=1)
    offsets = _chk_rr(raw.offsets, "offsets", dtype=torch.int64, dim=1)
    sizes = _chk_rr(raw.sizes, "sizes", dtype=torch.int32, dim=2)
    tx, ty = _chk_rr(raw.table_x, "table_x", dtype=torch.int32, dim=3), _chk_rr(raw.table_y, "table_y", dtype=torch.int32, dim=3)
    M = sizes.shape[0]
    if offsets.numel() != M or sizes.shape[1] != 2 or tx.shape[1] != W or ty.shape[1] != H or tx.shape[2] < 3 or ty.shape[2] < 3:
        raise ValueError("bank_fd_crop_batch: offsets %s, sizes %s, tables %s / %s disagree with each other or the %dx%d output"
                         % (tuple(offsets.shape), tuple(sizes.shape), tuple(tx.shape), tuple(ty.shape), H, W))
    N = draws.host.shape[0]
    if N > 65535:
        raise ValueError("bank_fd_crop_batch: at most 65535 samples per launch")
    hmax = int(draws.host[:, 4].max())
    if int(draws.host[:, 3].max()) > tx.shape[0] - 1 or hmax > ty.shape[0] - 1:
        raise ValueError("bank_fd_crop_batch: a crop is larger than the coefficient tables (%d x %d)" % (ty.shape[0] - 1, tx.shape[0] - 1))
    fd_crop_strip_width(hmax, W)
    if draws.dev is None:
        draws.to(data.device)
    if draws.dev.device != data.device:
        raise RuntimeError("bank_fd_crop_batch: the draws were uploaded to %s, the bank lives on %s" % (draws.dev.device, data.device))
    lut = _chk_lut("bank_fd_crop_batch", lut)
    out = torch.empty((N, 3, H, W), dtype=torch.float32, device=data.device)
    lib.rg_bank_fd_crop_batch(_p(data), _p(offsets), _p(sizes), M, _p(tx), tx.shape[2], tx.shape[0] - 1, _p(ty), ty.shape[2],
                              ty.shape[0] - 1, _p(draws.dev), _p(lut), _p(out), N, H, W, hmax, _stream())
    return out
