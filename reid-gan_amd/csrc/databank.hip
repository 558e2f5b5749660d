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
#include "rg_common.h"

namespace {

constexpr int MAXDIM = 1024;      // Hg, Wg <= MAXDIM for the pose maps (profiles live in LDS, as csrc/datagen.hip)

// One output pixel of channel c.  (y, xs): output row and PRE-FLIP output column.  `plane` is the sample's stored plane or
// nullptr (index outside the bank: the wrapper refuses it before the launch; here it reads nothing).
template <bool REID>
__device__ __forceinline__ float bank_pixel(const unsigned char* __restrict__ plane, const float* lut, const float* fill3, int c,
                                            int y, int xs, int Hs, int Ws, int top, int left, int pad, int er0, int ec0, int eh,
                                            int ew) {
    if (REID) {
        if (eh > 0 && y >= er0 && y < er0 + eh && xs >= ec0 && xs < ec0 + ew) return fill3[c];
    }
    const int r = top + y - pad, q = left + xs - pad;
    int b = 0;                                        // outside the stored plane: the padding is black BEFORE Normalize
    if (plane && (unsigned)r < (unsigned)Hs && (unsigned)q < (unsigned)Ws) b = plane[((int64_t)r * Ws + q) * 3 + c];
    return lut[c * 256 + b];
}

// VEC: 4 output columns per thread (W % 4 == 0), else 1.  REID: params[N][8] = (flip, top, left, er0, ec0, eh, ew, -);
// otherwise params points at the flips with `pstride` ints between samples, and the view is the whole plane.
template <bool REID, int VEC>
__global__ __launch_bounds__(256) void bank_image_kernel(const unsigned char* __restrict__ bank, int M, int Hs, int Ws,
                                                         const int* __restrict__ idx, const int* __restrict__ params, int pstride,
                                                         const float* __restrict__ lut_g, const float* __restrict__ fill,
                                                         float* __restrict__ out, int H, int W, int pad, int64_t items) {
    __shared__ float lut[768];
    __shared__ float fill3[3];
    for (int i = threadIdx.x; i < 768; i += 256) lut[i] = lut_g[i];
    if (threadIdx.x < 3) fill3[threadIdx.x] = (REID && fill) ? fill[threadIdx.x] : 0.f;
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
        int top = 0, left = 0, er0 = 0, ec0 = 0, eh = 0, ew = 0;
        if (REID) {
            top = p[1], left = p[2], er0 = p[3], ec0 = p[4], eh = p[5], ew = p[6];
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
                    vp[k] = bank_pixel<REID>(plane, lut, fill3, c, y, flip ? W - 1 - x : x, Hs, Ws, top, left, pad, er0, ec0, eh, ew);
                }
                *reinterpret_cast<float4*>(o + c * cstride) = v;
            }
        } else {
            for (int c = 0; c < 3; ++c)
                o[c * cstride] = bank_pixel<REID>(plane, lut, fill3, c, y, flip ? W - 1 - xv : xv, Hs, Ws, top, left, pad, er0, ec0, eh, ew);
        }
    }
}

template <bool REID>
int launch_image(const char* who, const unsigned char* bank, int M, int Hs, int Ws, const int* idx, const int* params, int pstride,
                 const float* lut, const float* fill, float* out, int N, int H, int W, int pad, hipStream_t stream) {
    const bool vec = (W % 4 == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
    const int64_t items = (int64_t)N * H * (vec ? W / 4 : W);
    int64_t g = rg::cdiv64(items, 256);
    if (g > 16384) g = 16384;
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 12.0 * N * (double)H * W + 3.0 * N * (double)H * W);
    if (vec)
        hipLaunchKernelGGL((bank_image_kernel<REID, 4>), dim3((unsigned)g), dim3(256), 0, stream, bank, M, Hs, Ws, idx, params, pstride,
                           lut, fill, out, H, W, pad, items);
    else
        hipLaunchKernelGGL((bank_image_kernel<REID, 1>), dim3((unsigned)g), dim3(256), 0, stream, bank, M, Hs, Ws, idx, params, pstride,
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

}  // namespace

extern "C" int rg_bank_reid_batch(const unsigned char* bank_u8, int M, int Hs, int Ws, const int* idx, const int* params,
                                  const float* lut, const float* fill, float* out, int N, int H, int W, int pad,
                                  hipStream_t stream) {
    RG_REQUIRE(bank_u8 && idx && params && lut && fill && out, "rg_bank_reid_batch: null argument");
    RG_REQUIRE(M > 0 && Hs > 0 && Ws > 0 && N > 0 && H > 0 && W > 0 && pad >= 0, "rg_bank_reid_batch: bad sizes");
    RG_REQUIRE(H <= Hs + 2 * pad && W <= Ws + 2 * pad, "rg_bank_reid_batch: crop %dx%d larger than the padded plane", H, W);
    return launch_image<true>("rg_bank_reid_batch", bank_u8, M, Hs, Ws, idx, params, 8, lut, fill, out, N, H, W, pad, stream);
}

extern "C" int rg_bank_gan_batch(const unsigned char* bank_u8, int M, int Hg, int Wg, const int* idx, const int* flip,
                                 int flip_stride, const float* lut, float* out, int N, hipStream_t stream) {
    RG_REQUIRE(bank_u8 && idx && flip && lut && out, "rg_bank_gan_batch: null argument");
    RG_REQUIRE(M > 0 && Hg > 0 && Wg > 0 && N > 0 && flip_stride >= 0, "rg_bank_gan_batch: bad sizes");
    return launch_image<false>("rg_bank_gan_batch", bank_u8, M, Hg, Wg, idx, flip, flip_stride, lut, nullptr, out, N, Hg, Wg, 0,
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
