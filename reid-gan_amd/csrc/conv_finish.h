// Split-K finishing kernels of the forward / data-gradient GEMMs (partial tiles -> output with the fused epilogue) and their launch;
// included by conv_fwd.hip and conv_dgrad.hip after conv_core.h.
#pragma once
#include "conv_core.h"

namespace {

// out[(img*M + m)*PIX + pix] = act((sum_s partial[s][m][n]) * scale[m] + shift[m] + res), n = img*PIX + pix
__global__ __launch_bounds__(256) void conv_splitk_finish_kernel(const float* __restrict__ partial,
                                                                 float* __restrict__ out, int M, int Ng, int PIX,
                                                                 FastDiv d_pix, int splits, Epilogue ep) {
    const int64_t total = (int64_t)M * Ng;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int m = (int)(i / Ng);
        const int n = (int)(i - (int64_t)m * Ng);
        float v = 0.f;
        for (int s = 0; s < splits; ++s) v += partial[(int64_t)s * total + i];
        const int im = fdiv(n, d_pix);
        const int pix = n - im * PIX;
        const int64_t o = ((int64_t)im * M + m) * PIX + pix;
        if (ep.scale) v *= ep.scale[m];
        if (ep.shift) v += ep.shift[m];
        if (ep.res) v += ep.res[o];
        v = rg_apply_act(v, ep.act, ep.slope);
        if (ep.mask && !(ep.mask[o] > 0.f)) v = 0.f;
        out[o] = v;
    }
}

// The same for Ng % 4 == 0 and PIX % 4 == 0 (every layer of the networks here): four consecutive columns per thread — they stay in
// one image and one row, so partials, residual, mask and output move as float4 — and the partial loads of four splits are in flight
// together.  Same left-to-right sum over the splits per element: same values as the scalar kernel.
__global__ __launch_bounds__(256) void conv_splitk_finish_vec_kernel(const float* __restrict__ partial, float* __restrict__ out,
                                                                     int M, int Ng, int PIX, FastDiv d_pix, FastDiv d_ng4,
                                                                     int splits, Epilogue ep) {
    const int ng4 = Ng >> 2;
    const int64_t total4 = (int64_t)M * ng4;
    const int64_t sstride4 = total4;                    // float4 units between splits
    const float4* p4 = reinterpret_cast<const float4*>(partial);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (int64_t)gridDim.x * blockDim.x) {
        const int m = fdiv((int)i, d_ng4);
        const int n = ((int)i - m * ng4) << 2;
        const float4 v = splitk_sum4(p4, sstride4, i, splits);
        const int im = fdiv(n, d_pix);
        const int pix = n - im * PIX;
        splitk_epilogue_store4(out, ((int64_t)im * M + m) * PIX + pix, m, v, ep);
    }
}

// the vector finisher (and the in-kernel finish, which moves float4s as well) takes 16-byte aligned buffers and float4 rows
static bool finish_vec_ok(const float* partial, const float* out, int M, int Ng, int PIX, const Epilogue& ep) {
    return rg::conv::aligned16(partial, out, ep.res, ep.mask) && (Ng & 3) == 0 && (PIX & 3) == 0 && (int64_t)M * Ng < (1ll << 31);
}

// the arrival counters of a one-class split-K launch (rg_conv_splitk_arrivals), or nullptr: a finishing launch follows
static unsigned* splitk_arrivals(hipStream_t stream, int tiles, const float* partial, const float* out, int M, int Ng, int PIX,
                                 const Epilogue& ep) {
    if (!finish_vec_ok(partial, out, M, Ng, PIX, ep) || ep.rowsum) return nullptr;
    return rg::conv::splitk_arrivals(stream, tiles);
}

static void launch_finish(hipStream_t stream, const float* partial, float* out, int M, int Ng, int PIX, const FastDiv& d_pix,
                          int splits, const Epilogue& ep) {
    if (finish_vec_ok(partial, out, M, Ng, PIX, ep)) {
        hipLaunchKernelGGL(conv_splitk_finish_vec_kernel, dim3(finish_grid((int64_t)M * (Ng >> 2))), dim3(256), 0, stream, partial, out,
                           M, Ng, PIX, d_pix, make_fastdiv(Ng >> 2), splits, ep);
        return;
    }
    hipLaunchKernelGGL(conv_splitk_finish_kernel, dim3(finish_grid((int64_t)M * Ng)), dim3(256), 0, stream, partial, out, M, Ng, PIX,
                       d_pix, splits, ep);
}

}  // namespace
