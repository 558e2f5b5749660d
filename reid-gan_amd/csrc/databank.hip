// Device-resident image bank: finished fp32 NCHW batches gathered from uint8 planes that stay in HBM for the whole run.
// What the reference does per drawn sample on the host (CC/examples/cluster_contrast_gan_train_usl_infomap.py:71-186,
// CC/clustercontrast/utils/data/preprocessor.py:99-199) after its deterministic resize:
//   Pad(pad, black) -> RandomCrop((H, W)) -> ToTensor -> Normalize -> RandomErasing -> torch.flip(img, [2])     the ReID view
//   ToTensor -> Normalize((.5,.5,.5), (.5,.5,.5)) -> torch.flip                                                 the GAN image
//   cords_to_map (pose_utils.py:51-70) -> torch.flip                                                            the pose maps
// The resize precedes every random draw, so it is done once when the bank is built; what is left per batch is a gather.
// ToTensor + Normalize of a byte has 256 possible results per channel: they arrive as a table built by torch with the
// reference's own arithmetic, and the image kernels do no floating-point arithmetic at all — the batch equals the host
// pipeline's bit for bit by construction.  Each entry is one launch, with no workspace, no atomic and no intermediate batch.
//
// Layout: a stored plane is [Hs][Ws][3] bytes (interleaved RGB as PIL / numpy give it), so the three channels of a pixel
// and of its neighbours come from one 3*Ws-byte row; a thread takes 4 consecutive output columns of one output row for all
// three channels (12 neighbouring bytes in, three 16-byte stores out — the output, 12x the input, is what the kernel is
// bound by).  Where W % 4 != 0 the rows of the output planes are not 16-byte aligned and a thread takes one column.
//
// FD-GAN stage II (FD/train.py:21-44, FD/reid/utils/data/preprocessor.py:63-98) draws pairs of items, each
//   RectScale -> RandomSizedEarser (a colour patch pasted on the BYTES) -> RandomHorizontalFlip -> ToTensor -> Normalize     origin
//   RectScale -> flip -> ToTensor -> Normalize                                                                               target
//   _generate_pose_map of the target's landmarks (one joint erased, or sigma drawn) -> np.flip(maps, 2)                      posemap
// RectScale again precedes every draw: rg_bank_fd_image_batch is the image gather with the patch looked up in the table by its
// colour bytes, rg_bank_fd_pose_batch the filtered-impulse form of the maps (pose_profiles.h) from a per-image landmark table.
#include "pose_profiles.h"
#include "rg_common.h"

namespace {

constexpr int MAXDIM = rg::POSE_MAXDIM;      // Hg, Wg <= MAXDIM for the pose maps (profiles live in LDS, as csrc/datagen.hip)
enum { KIND_GAN = 0, KIND_REID = 1, KIND_FD = 2 };

// One output pixel of channel c.  (y, xs): output row and PRE-FLIP output column.  `plane` is the sample's stored plane or
// nullptr (index outside the bank: the wrapper refuses it before the launch; here it reads nothing).
// KIND_REID: the rectangle holds fill3[c] (RandomErasing after Normalize); KIND_FD: it holds the table entry of byte c of `rgb`
// (RandomSizedEarser pastes bytes before ToTensor / Normalize); KIND_GAN: no rectangle.
template <int KIND>
__device__ __forceinline__ float bank_pixel(const unsigned char* __restrict__ plane, const float* lut, const float* fill3, int c,
                                            int y, int xs, int Hs, int Ws, int top, int left, int pad, int er0, int ec0, int eh,
                                            int ew, int rgb) {
    if (KIND != KIND_GAN) {
        if (eh > 0 && y >= er0 && y < er0 + eh && xs >= ec0 && xs < ec0 + ew)
            return KIND == KIND_FD ? lut[c * 256 + ((rgb >> (8 * c)) & 255)] : fill3[c];
    }
    const int r = top + y - pad, q = left + xs - pad;
    int b = 0;                                        // outside the stored plane: the padding is black BEFORE Normalize
    if (plane && (unsigned)r < (unsigned)Hs && (unsigned)q < (unsigned)Ws) b = plane[((int64_t)r * Ws + q) * 3 + c];
    return lut[c * 256 + b];
}

// VEC: 4 output columns per thread (W % 4 == 0), else 1.  KIND_REID: params[N][8] = (flip, top, left, er0, ec0, eh, ew, -);
// KIND_FD: params[N][8] = (flip, -, -, er0, ec0, eh, ew, rgb) and the view is the whole plane; KIND_GAN: params points at the
// flips with `pstride` ints between samples, and the view is the whole plane.
template <int KIND, int VEC>
__global__ __launch_bounds__(256) void bank_image_kernel(const unsigned char* __restrict__ bank, int M, int Hs, int Ws,
                                                         const int* __restrict__ idx, const int* __restrict__ params, int pstride,
                                                         const float* __restrict__ lut_g, const float* __restrict__ fill,
                                                         float* __restrict__ out, int H, int W, int pad, int64_t items) {
    __shared__ float lut[768];
    __shared__ float fill3[3];
    for (int i = threadIdx.x; i < 768; i += 256) lut[i] = lut_g[i];
    if (threadIdx.x < 3) fill3[threadIdx.x] = (KIND == KIND_REID && fill) ? fill[threadIdx.x] : 0.f;
    __syncthreads();
    const int Wv = W / VEC;
    const int64_t plane_bytes = (int64_t)Hs * Ws * 3;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (int64_t)gridDim.x * 256) {
        const int xv = (int)(i % Wv);
        int64_t t = i / Wv;
        const int y = (int)(t % H);
        const int n = (int)(t / H);
        const int* p = params + (int64_t)n * pstride;
        const int flip = p[0];
        int top = 0, left = 0, er0 = 0, ec0 = 0, eh = 0, ew = 0, rgb = 0;
        if (KIND == KIND_REID) {
            top = p[1], left = p[2], er0 = p[3], ec0 = p[4], eh = p[5], ew = p[6];
        }
        if (KIND == KIND_FD) {
            er0 = p[3], ec0 = p[4], eh = p[5], ew = p[6], rgb = p[7];
        }
        const int m = idx[n];
        const unsigned char* plane = (unsigned)m < (unsigned)M ? bank + (int64_t)m * plane_bytes : nullptr;
        float* o = out + (((int64_t)n * 3) * H + y) * W + xv * VEC;
        const int64_t cstride = (int64_t)H * W;
        if (VEC == 4) {
            for (int c = 0; c < 3; ++c) {
                float4 v;
                float* vp = reinterpret_cast<float*>(&v);
                for (int k = 0; k < 4; ++k) {
                    const int x = xv * 4 + k;
                    vp[k] = bank_pixel<KIND>(plane, lut, fill3, c, y, flip ? W - 1 - x : x, Hs, Ws, top, left, pad, er0, ec0, eh, ew, rgb);
                }
                *reinterpret_cast<float4*>(o + c * cstride) = v;
            }
        } else {
            for (int c = 0; c < 3; ++c)
                o[c * cstride] = bank_pixel<KIND>(plane, lut, fill3, c, y, flip ? W - 1 - xv : xv, Hs, Ws, top, left, pad, er0, ec0, eh, ew,
                                                rgb);
        }
    }
}

template <int KIND>
int launch_image(const char* who, const unsigned char* bank, int M, int Hs, int Ws, const int* idx, const int* params, int pstride,
                 const float* lut, const float* fill, float* out, int N, int H, int W, int pad, hipStream_t stream) {
    const bool vec = (W % 4 == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
    const int64_t items = (int64_t)N * H * (vec ? W / 4 : W);
    int64_t g = rg::cdiv64(items, 256);
    if (g > 16384) g = 16384;
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 12.0 * N * (double)H * W + 3.0 * N * (double)H * W);
    if (vec)
        hipLaunchKernelGGL((bank_image_kernel<KIND, 4>), dim3((unsigned)g), dim3(256), 0, stream, bank, M, Hs, Ws, idx, params, pstride,
                           lut, fill, out, H, W, pad, items);
    else
        hipLaunchKernelGGL((bank_image_kernel<KIND, 1>), dim3((unsigned)g), dim3(256), 0, stream, bank, M, Hs, Ws, idx, params, pstride,
                           lut, fill, out, H, W, pad, items);
    return rg::check_launch(who);
}

// grid (J, N): one workgroup per (sample, joint); the mode-1 expression of pose_maps_kernel (csrc/datagen.hip) — two float64
// profiles, one exp per row / column, their product rounded to float32 — read at (y, flip ? W-1-x : x).
__global__ __launch_bounds__(256) void bank_pose_kernel(const int* __restrict__ centres, int M, const int* __restrict__ idx,
                                                        const int* __restrict__ flips, int fstride, float sigma,
                                                        float* __restrict__ out, int J, int H, int W) {
    __shared__ double fy[MAXDIM], fx[MAXDIM];
    const int j = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const int m = idx[n];
    float* o = out + ((int64_t)n * J + j) * H * W;
    int cy = INT32_MIN, cx = INT32_MIN;
    if ((unsigned)m < (unsigned)M) {
        cy = centres[((int64_t)m * J + j) * 2 + 0];
        cx = centres[((int64_t)m * J + j) * 2 + 1];
    }
    if (cy == INT32_MIN || cx == INT32_MIN) {          // missing joint -> zeros (uniform per block)
        for (int i = tid; i < H * W; i += 256) o[i] = 0.f;
        return;
    }
    const int flip = flips[(int64_t)n * fstride];
    const double sg = (double)sigma;
    const double inv = -1.0 / (2.0 * sg * sg);
    for (int i = tid; i < H; i += 256) fy[i] = exp((double)(i - cy) * (double)(i - cy) * inv);
    for (int i = tid; i < W; i += 256) fx[i] = exp((double)(i - cx) * (double)(i - cx) * inv);
    __syncthreads();
    for (int i = tid; i < H * W; i += 256) {
        const int y = i / W, x = i - y * W;
        o[i] = (float)(fy[y] * fx[flip ? W - 1 - x : x]);
    }
}

// grid (J, N): one workgroup per (sample, joint); the mode-0 expression of pose_maps_kernel (csrc/datagen.hip) through the shared
// profile code of pose_profiles.h, with the sample's own sigma, read at (y, flip ? W-1-x : x).  pp[N][4] = (flip, sigma, erased
// joint or -1, -).  VEC 4: a thread writes 4 neighbouring columns of a row with one 16-byte store (W % 4 == 0).
template <int VEC>
__global__ __launch_bounds__(256) void bank_fd_pose_kernel(const int* __restrict__ landmarks, int M, const int* __restrict__ idx,
                                                           const int* __restrict__ pp, float* __restrict__ out, int J, int H, int W) {
    __shared__ double fy[MAXDIM], fx[MAXDIM];
    __shared__ double red[8];
    const int j = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const int m = idx[n];
    const int flip = pp[n * 4 + 0], sigma = pp[n * 4 + 1], erased = pp[n * 4 + 2];
    float* o = out + ((int64_t)n * J + j) * H * W;
    int cy = -1, cx = -1;
    if ((unsigned)m < (unsigned)M) {
        cy = landmarks[((int64_t)m * J + j) * 2 + 0];
        cx = landmarks[((int64_t)m * J + j) * 2 + 1];
    }
    const int items = H * W / VEC;
    // erased, undetected (-1) or outside the map -> zeros (uniform per block)
    if (j == erased || cy < 0 || cx < 0 || cy >= H || cx >= W) {
        if (VEC == 4) {
            for (int i = tid; i < items; i += 256) reinterpret_cast<float4*>(o)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            for (int i = tid; i < items; i += 256) o[i] = 0.f;
        }
        return;
    }
    const double inv = rg::fd_pose_profiles(fy, fx, red, cy, cx, H, W, (double)sigma);
    if (VEC == 4) {
        const int Wv = W / 4;
        for (int i = tid; i < items; i += 256) {
            const int y = i / Wv, x0 = (i - y * Wv) * 4;
            const double row = fy[y];
            float4 v;
            float* vp = reinterpret_cast<float*>(&v);
            for (int k = 0; k < 4; ++k) {
                const int x = x0 + k;
                vp[k] = (float)(row * fx[flip ? W - 1 - x : x] * inv);
            }
            reinterpret_cast<float4*>(o)[i] = v;
        }
    } else {
        for (int i = tid; i < items; i += 256) {
            const int y = i / W, x = i - y * W;
            o[i] = (float)(fy[y] * fx[flip ? W - 1 - x : x] * inv);
        }
    }
}

// ---- FD-GAN stage I: RandomSizedRectCrop -> RandomSizedEarser -> flip -> ToTensor -> Normalize from the RAW images -------------
// The resize follows the draw here (img.crop(box).resize((W, H), BILINEAR)), so there is no resized plane to gather from: the
// kernel resamples the drawn box itself, with PIL's own integer rule.  PIL's coefficients of an axis depend on (input length,
// output length) alone because the resample box is always the whole crop; the host builds them once for every input length that
// can occur (device_bank.pil_bilinear_table) as rows of `stride` ints (lo, cnt, k_0 .. k_{stride-3}), row (n, j) at
// (n * out_len + j) * stride, and the device does integer multiply-adds only:
//     out = min(255, (2^21 + sum_x in[lo + x] * k_x) >> 22)        (k_x >= 0, so the sum is never negative)
// grid (strips, N).  A workgroup takes SW neighbouring PRE-FLIP output columns of one sample: pass 1 resamples the crop's h rows
// to those columns into an LDS tile of bytes [3][h][SW] (planar, so four neighbouring columns of a channel are one dword),
// pass 2 resamples the tile's columns to the H output rows, lays the eraser's patch over the bytes, looks them up in the
// Normalize table and writes 4 columns per thread with one 16-byte store (reversed for a flipped sample).  SW is the
// largest multiple of 4 up to FD_CROP_COLS whose tile of hmax rows fits FD_CROP_LDS; an output no wider than that is one
// workgroup per sample, anything else is cut into strips (the recipe's 128 columns into 4: 119 us against 220 us for 512 samples
// from one workgroup each, profiles/fd_stage1_loader.txt).
constexpr int FD_CROP_LDS = 60 * 1024;      // the tile's share of a 64 KiB workgroup, so two workgroups fit a CU's 160 KiB
constexpr int FD_CROP_INTS = 12;            // (row, x1, y1, w, h, flip, er0, ec0, eh, ew, rgb, -) per sample
constexpr int FD_CROP_BITS = 22;

constexpr int FD_CROP_COLS = 32;            // widest strip: 4 strips of a 128-column sample keep 8 workgroups on a CU, not 2

// columns per workgroup for crops of up to hmax rows: W (one workgroup per sample), a smaller multiple of 4 (strips), 0 (none fits)
int fd_crop_strip(int hmax, int W) {
    int sw = (FD_CROP_LDS / (3 * hmax)) & ~3;
    if (sw > FD_CROP_COLS) sw = FD_CROP_COLS;
    return sw >= W ? W : sw;
}

__global__ __launch_bounds__(256) void bank_fd_crop_kernel(const unsigned char* __restrict__ bank, const int64_t* __restrict__ offs,
                                                           const int* __restrict__ sizes, int M, const int* __restrict__ tabx,
                                                           int sx, int nx, const int* __restrict__ taby, int sy, int ny,
                                                           const int* __restrict__ draws, const float* __restrict__ lut_g,
                                                           float* __restrict__ out, int H, int W, int SW, int hmax) {
    extern __shared__ __align__(16) unsigned char tile[];        // [3][h][SW] bytes of pass 1
    __shared__ float lut[768];
    const int tid = threadIdx.x, n = blockIdx.y;
    const int c0 = blockIdx.x * SW;                              // first pre-flip output column of this strip
    const int sw = min(SW, W - c0);
    for (int i = tid; i < 768; i += 256) lut[i] = lut_g[i];
    const int* d = draws + (int64_t)n * FD_CROP_INTS;
    const int m = d[0], x1 = d[1], y1 = d[2], w = d[3], flip = d[5];
    const int er0 = d[6], ec0 = d[7], eh = d[8], ew = d[9], rgb = d[10];
    int h = d[4];
    // the wrapper refuses every draw outside the image before the launch; here such a sample reads nothing and comes out black
    bool ok = (unsigned)m < (unsigned)M && w >= 1 && h >= 1 && w <= nx && h <= ny && h <= hmax && x1 >= 0 && y1 >= 0;
    int Wm = 0;
    if (ok) {
        Wm = sizes[2 * m + 1];
        ok = y1 <= sizes[2 * m] - h && x1 <= Wm - w;
    }
    if (!ok) h = 0;
    if (ok) {
        const unsigned char* src = bank + offs[m] + ((int64_t)y1 * Wm + x1) * 3;
        const int* tx = tabx + ((int64_t)w * W + c0) * sx;
        for (int i = tid; i < h * sw * 3; i += 256) {
            const int cc = i % sw, t = i / sw;
            const int ch = t % 3, row = t / 3;
            const int* e = tx + cc * sx;
            const int cnt = e[1];
            const unsigned char* p = src + ((int64_t)row * Wm + e[0]) * 3 + ch;
            int acc = 1 << (FD_CROP_BITS - 1);
            for (int x = 0; x < cnt; ++x) acc += (int)p[x * 3] * e[2 + x];
            tile[(ch * h + row) * SW + cc] = (unsigned char)min(acc >> FD_CROP_BITS, 255);
        }
    }
    __syncthreads();
    const int* ty = taby + (int64_t)h * H * sy;
    const int groups = sw >> 2;
    for (int i = tid; i < 3 * H * groups; i += 256) {
        const int q = i % groups, t = i / groups;
        const int r = t % H, ch = t / H;
        int acc[4] = {1 << (FD_CROP_BITS - 1), 1 << (FD_CROP_BITS - 1), 1 << (FD_CROP_BITS - 1), 1 << (FD_CROP_BITS - 1)};
        if (ok) {
            const int* e = ty + r * sy;
            const int lo = e[0], cnt = e[1];
            for (int x = 0; x < cnt; ++x) {
                const unsigned v = *reinterpret_cast<const unsigned*>(tile + (ch * h + lo + x) * SW + 4 * q);
                const int k = e[2 + x];
                for (int j = 0; j < 4; ++j) acc[j] += (int)((v >> (8 * j)) & 255u) * k;
            }
        }
        const int cp = c0 + 4 * q;                               // pre-flip columns cp .. cp + 3
        const bool in_rows = eh > 0 && r >= er0 && r < er0 + eh;
        float f[4];
        for (int j = 0; j < 4; ++j) {
            int b = min(acc[j] >> FD_CROP_BITS, 255);
            if (in_rows && cp + j >= ec0 && cp + j < ec0 + ew) b = (rgb >> (8 * ch)) & 255;
            f[j] = lut[ch * 256 + b];
        }
        float* o = out + (((int64_t)n * 3 + ch) * H + r) * W;
        if (flip)
            *reinterpret_cast<float4*>(o + (W - 4 - cp)) = make_float4(f[3], f[2], f[1], f[0]);
        else
            *reinterpret_cast<float4*>(o + cp) = make_float4(f[0], f[1], f[2], f[3]);
    }
}

}  // namespace

extern "C" int rg_bank_reid_batch(const unsigned char* bank_u8, int M, int Hs, int Ws, const int* idx, const int* params,
                                  const float* lut, const float* fill, float* out, int N, int H, int W, int pad,
                                  hipStream_t stream) {
    RG_REQUIRE(bank_u8 && idx && params && lut && fill && out, "rg_bank_reid_batch: null argument");
    RG_REQUIRE(M > 0 && Hs > 0 && Ws > 0 && N > 0 && H > 0 && W > 0 && pad >= 0, "rg_bank_reid_batch: bad sizes");
    RG_REQUIRE(H <= Hs + 2 * pad && W <= Ws + 2 * pad, "rg_bank_reid_batch: crop %dx%d larger than the padded plane", H, W);
    return launch_image<KIND_REID>("rg_bank_reid_batch", bank_u8, M, Hs, Ws, idx, params, 8, lut, fill, out, N, H, W, pad, stream);
}

extern "C" int rg_bank_gan_batch(const unsigned char* bank_u8, int M, int Hg, int Wg, const int* idx, const int* flip,
                                 int flip_stride, const float* lut, float* out, int N, hipStream_t stream) {
    RG_REQUIRE(bank_u8 && idx && flip && lut && out, "rg_bank_gan_batch: null argument");
    RG_REQUIRE(M > 0 && Hg > 0 && Wg > 0 && N > 0 && flip_stride >= 0, "rg_bank_gan_batch: bad sizes");
    return launch_image<KIND_GAN>("rg_bank_gan_batch", bank_u8, M, Hg, Wg, idx, flip, flip_stride, lut, nullptr, out, N, Hg, Wg, 0,
                               stream);
}

extern "C" int rg_bank_pose_batch(const int* centres, int M, int J, const int* idx, const int* flip, int flip_stride, float sigma,
                                  float* out, int N, int Hg, int Wg, hipStream_t stream) {
    RG_REQUIRE(centres && idx && flip && out, "rg_bank_pose_batch: null argument");
    RG_REQUIRE(M > 0 && J > 0 && N > 0 && Hg > 0 && Wg > 0 && flip_stride >= 0, "rg_bank_pose_batch: bad sizes");
    RG_REQUIRE(Hg <= MAXDIM && Wg <= MAXDIM, "rg_bank_pose_batch: Hg, Wg must be <= %d", MAXDIM);
    RG_REQUIRE(N <= 65535, "rg_bank_pose_batch: N > 65535");
    RG_REQUIRE(sigma > 0.f, "rg_bank_pose_batch: sigma must be positive");
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 4.0 * N * (double)J * Hg * Wg);
    hipLaunchKernelGGL(bank_pose_kernel, dim3(J, N), dim3(256), 0, stream, centres, M, idx, flip, flip_stride, sigma, out, J, Hg, Wg);
    return rg::check_launch("rg_bank_pose_batch");
}

extern "C" int rg_bank_fd_image_batch(const unsigned char* bank_u8, int M, int H, int W, const int* idx, const int* params,
                                      const float* lut, float* out, int N, hipStream_t stream) {
    RG_REQUIRE(bank_u8 && idx && params && lut && out, "rg_bank_fd_image_batch: null argument");
    RG_REQUIRE(M > 0 && H > 0 && W > 0 && N > 0, "rg_bank_fd_image_batch: bad sizes");
    return launch_image<KIND_FD>("rg_bank_fd_image_batch", bank_u8, M, H, W, idx, params, 8, lut, nullptr, out, N, H, W, 0, stream);
}

extern "C" int rg_bank_fd_pose_batch(const int* landmarks, int M, int J, const int* idx, const int* pose_params, float* out, int N,
                                     int H, int W, hipStream_t stream) {
    RG_REQUIRE(landmarks && idx && pose_params && out, "rg_bank_fd_pose_batch: null argument");
    RG_REQUIRE(M > 0 && J > 0 && N > 0 && H > 0 && W > 0, "rg_bank_fd_pose_batch: bad sizes");
    RG_REQUIRE(H <= MAXDIM && W <= MAXDIM, "rg_bank_fd_pose_batch: H, W must be <= %d", MAXDIM);
    RG_REQUIRE(N <= 65535, "rg_bank_fd_pose_batch: N > 65535");
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 4.0 * N * (double)J * H * W);
    if ((W % 4 == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0))
        hipLaunchKernelGGL(bank_fd_pose_kernel<4>, dim3(J, N), dim3(256), 0, stream, landmarks, M, idx, pose_params, out, J, H, W);
    else
        hipLaunchKernelGGL(bank_fd_pose_kernel<1>, dim3(J, N), dim3(256), 0, stream, landmarks, M, idx, pose_params, out, J, H, W);
    return rg::check_launch("rg_bank_fd_pose_batch");
}

extern "C" int64_t rg_bank_fd_crop_regime(int hmax, int W) {
    if (hmax <= 0 || W <= 0 || (W & 3)) return -1;
    const int sw = fd_crop_strip(hmax, W);
    return sw >= 4 ? sw : -1;
}

extern "C" int rg_bank_fd_crop_batch(const unsigned char* bank_u8, const int64_t* offsets, const int* sizes, int M, const int* table_x,
                                     int stride_x, int nmax_x, const int* table_y, int stride_y, int nmax_y, const int* draws,
                                     const float* lut, float* out, int N, int H, int W, int hmax, hipStream_t stream) {
    RG_REQUIRE(bank_u8 && offsets && sizes && table_x && table_y && draws && lut && out, "rg_bank_fd_crop_batch: null argument");
    RG_REQUIRE(M > 0 && N > 0 && H > 0 && W > 0 && nmax_x > 0 && nmax_y > 0, "rg_bank_fd_crop_batch: bad sizes");
    RG_REQUIRE(stride_x >= 3 && stride_y >= 3, "rg_bank_fd_crop_batch: a table row holds (lo, cnt, k_0 ...)");
    RG_REQUIRE(W % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0,
               "rg_bank_fd_crop_batch: W must be a multiple of 4 and out 16-byte aligned (16-byte row stores)");
    RG_REQUIRE(N <= 65535, "rg_bank_fd_crop_batch: N > 65535");
    RG_REQUIRE(hmax >= 1 && hmax <= nmax_y, "rg_bank_fd_crop_batch: hmax %d outside [1, %d]", hmax, nmax_y);
    const int sw = fd_crop_strip(hmax, W);
    RG_REQUIRE(sw >= 4, "rg_bank_fd_crop_batch: a 4-column strip of %d rows does not fit %d bytes of LDS", hmax, FD_CROP_LDS);
    const int strips = (W + sw - 1) / sw;
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 12.0 * N * (double)H * W + 3.0 * N * (double)H * W);
    hipLaunchKernelGGL(bank_fd_crop_kernel, dim3(strips, N), dim3(256), (size_t)3 * hmax * sw, stream, bank_u8, offsets, sizes, M,
                       table_x, stride_x, nmax_x, table_y, stride_y, nmax_y, draws, lut, out, H, W, sw, hmax);
    return rg::check_launch("rg_bank_fd_crop_batch");
}
