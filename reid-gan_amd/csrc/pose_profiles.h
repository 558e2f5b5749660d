// FD-GAN's pose map of one joint as two float64 profiles: the closed form of `_generate_pose_map`
// (FD/reid/utils/data/preprocessor.py:114-131 — unit impulse -> scipy gaussian_filter(sigma, truncate 4, mode 'reflect') -> / max),
// which is separable: map[y][x] = fy[y] * fx[x] / (max fy * max fx).  Shared by rg_pose_maps mode 0 (csrc/datagen.hip) and
// rg_bank_fd_pose_batch (csrc/databank.hip), so the two give the same bits.
#pragma once
#include "rg_common.h"

namespace rg {

constexpr int POSE_MAXDIM = 1024;      // H, W <= POSE_MAXDIM (the profiles live in LDS)

// scipy's 1-D Gaussian correlate of a unit impulse at `c` on [0, n) with 'reflect' extension (d c b a | a b c d | d c b a):
// out[i] = sum_{k=-r..r} w[k] * [reflect(i + k) == c],  w[k] = exp(-k^2 / (2 sigma^2)) / sum_k(...)   (float64, as numpy)
// Only the first mirror image on each side is counted: exact while r <= n.
__device__ inline double impulse_response(int i, int c, int n, int r, double sigma, double wsum) {
    double v = 0.0;
    const double inv = -0.5 / (sigma * sigma);
    int k = c - i;                                  // inside the array
    if (k >= -r && k <= r) v += exp(inv * (double)k * (double)k) / wsum;
    k = -1 - c - i;                                 // mirror image below 0: i + k = -1 - c
    if (k >= -r && k <= r && i + k < 0) v += exp(inv * (double)k * (double)k) / wsum;
    k = 2 * n - 1 - c - i;                          // mirror image above n-1: i + k = 2n - 1 - c
    if (k >= -r && k <= r && i + k >= n) v += exp(inv * (double)k * (double)k) / wsum;
    return v;
}

// Called by all 256 threads of a workgroup with 0 <= cy < H, 0 <= cx < W: fills fy[H], fx[W] (LDS) and returns
// 1 / (max fy * max fx), so that map[y][x] = (float)(fy[y] * fx[x] * inv).  red: 8 doubles of LDS.  Ends behind a barrier.
__device__ __forceinline__ double fd_pose_profiles(double* fy, double* fx, double* red, int cy, int cx, int H, int W, double sg) {
    const int tid = threadIdx.x;
    const int r = (int)(4.0 * sg + 0.5);                 // scipy: int(truncate * sd + 0.5)
    // kernel normalisation sum_k exp(-k^2 / 2 sigma^2), summed in scipy's order (k ascending) by one thread
    if (tid == 0) {
        double acc = 0.0;
        for (int k = -r; k <= r; ++k) acc += exp(-0.5 / (sg * sg) * (double)k * (double)k);
        red[0] = acc;
    }
    __syncthreads();
    const double wsum = red[0];
    __syncthreads();
    for (int i = tid; i < H; i += 256) fy[i] = impulse_response(i, cy, H, r, sg, wsum);
    for (int i = tid; i < W; i += 256) fx[i] = impulse_response(i, cx, W, r, sg, wsum);
    __syncthreads();
    // map.max() = max(fy) * max(fx) (all entries >= 0)
    double my = 0.0, mx = 0.0;
    for (int i = tid; i < H; i += 256) my = fmax(my, fy[i]);
    for (int i = tid; i < W; i += 256) mx = fmax(mx, fx[i]);
    for (int off = 32; off > 0; off >>= 1) {
        my = fmax(my, __shfl_xor(my, off, 64));
        mx = fmax(mx, __shfl_xor(mx, off, 64));
    }
    if ((tid & 63) == 0) {
        red[tid >> 6] = my;
        red[4 + (tid >> 6)] = mx;
    }
    __syncthreads();
    my = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    mx = fmax(fmax(red[4], red[5]), fmax(red[6], red[7]));
    return 1.0 / (my * mx);
}

}  // namespace rg
