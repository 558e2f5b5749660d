// What the thin-layer kernels of conv_fwd.hip (conv_fwd_k1_kernel) and conv_wgrad.hip (conv_wgrad_k1_kernel) share.
#pragma once
#include "conv_core.h"

namespace {

// ---------------------------------------------------------------------------------------------
// One-output-channel convolutions (the PatchGAN heads: FD/fdgan/networks.py:225-226 Conv(512 -> 1, 4, 1, 1),
// CC/dual_gan/models/networks.py:946 ResDiscriminator's final conv): a 32-row MFMA tile would be 97 % padding and the
// layer is a 30 MB read with 0.2 GFLOP, so these are direct VALU kernels bound by the read of x.  Lanes run along the
// output pixels (coalesced rows of x, every element re-used KH*KW times out of L1); the input channels (forward) or
// the pixels (weight gradient) are sliced across blockIdx.y and the slices are summed by the ordinary split-K
// finishing kernels (same partial layout [slice][M = 1][n]), in fixed order: deterministic.
// ---------------------------------------------------------------------------------------------
struct ThinP {
    const float* x;
    const float* a;      // fwd: w [1][C][KH][KW]; wgrad: dy [N][1][P][Q]
    float* partial;
    int N, C, H, W, P, Q, SH, SW, PH, PW, per_slice;
    unsigned x_bytes;
    FastDiv d_pq, d_q;
};

// layers with <= 4 output channels: filter sizes with an instantiation
static bool thin_filter(const ConvGeom& g) {
    return g.K >= 1 && g.K <= 4 && ((g.KH == 4 && g.KW == 4 && g.K == 1) || (g.KH == 3 && g.KW == 3));
}
#define THIN_DISPATCH(KERNEL, g, grid, stream, t)                                                     \
    do {                                                                                              \
        if (g.KH == 4) hipLaunchKernelGGL((KERNEL<4, 4, 1>), grid, dim3(256), 0, stream, t);          \
        else if (g.K == 1) hipLaunchKernelGGL((KERNEL<3, 3, 1>), grid, dim3(256), 0, stream, t);      \
        else if (g.K == 2) hipLaunchKernelGGL((KERNEL<3, 3, 2>), grid, dim3(256), 0, stream, t);      \
        else if (g.K == 3) hipLaunchKernelGGL((KERNEL<3, 3, 3>), grid, dim3(256), 0, stream, t);      \
        else hipLaunchKernelGGL((KERNEL<3, 3, 4>), grid, dim3(256), 0, stream, t);                    \
    } while (0)
static void thin_fill(ThinP& t, const float* x, const float* a, float* partial, const ConvGeom& g, int per_slice) {
    t.x = x; t.a = a; t.partial = partial;
    t.N = g.N; t.C = g.C; t.H = g.H; t.W = g.W; t.P = g.P; t.Q = g.Q; t.SH = g.SH; t.SW = g.SW; t.PH = g.PH; t.PW = g.PW;
    t.per_slice = per_slice;
    t.x_bytes = x_bytes(g);
    t.d_pq = make_fastdiv(g.P * g.Q);
    t.d_q = make_fastdiv(g.Q);
}

}  // namespace
