// Depthwise 3x3 convolution, stride 1 or 2, pad 1, no bias (RepLKNet stem[1], stem[3] and the
// transitions' second conv, networks/replknet_adapter.py:414-416, 451-453).  MIOpen serves these grouped
// strided convs with its naive reference kernels (170-340 us each on MI355X); they are plain HBM-bound
// stencils: one thread per output (fwd) / input (dgrad) pixel, 9 wave-uniform taps per channel from SGPRs.
#include "common.h"

namespace {

// Inference epilogue (ppea_dwconv3x3_fwd_affine_*): y = act(s[c] * conv + o[c]) -- the eval-mode BatchNorm (+ ReLU) that
// follows stem[1], stem[3] and transitions[.][1], applied to the fp32 accumulator before the store.
struct Aff { const float* s; const float* o; int relu; };
template <bool AFF>
__device__ __forceinline__ float aff1(float v, float a, float b, int relu) {
    if constexpr (AFF) { v = fmaf(a, v, b); if (relu) v = fmaxf(v, 0.f); }
    return v;
}

template <typename T, int S, bool AFF>
__device__ __forceinline__ void dw3_fwd_body(const T* __restrict__ x, const float* __restrict__ w,
                                             T* __restrict__ y, int C, int H, int W, int Ho, int Wo, Aff af) {
    const int plane = blockIdx.y;                          // n * C + c
    const int c = plane % C;
    float fa = 1.f, fb = 0.f;
    if constexpr (AFF) { fa = af.s[c]; fb = af.o[c]; }
    const float* wc = w + c * 9;
    float k[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) k[i] = wc[i];
    const T* xp = x + (long)plane * H * W;
    T* yp = y + (long)plane * Ho * Wo;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < Ho * Wo; i += gridDim.x * 256) {
        const int oy = i / Wo, ox = i - oy * Wo;
        const int iy0 = oy * S - 1, ix0 = ox * S - 1;
        float acc = 0.f;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int iy = iy0 + u;
            if (iy < 0 || iy >= H) continue;
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                const int ix = ix0 + v;
                if (ix >= 0 && ix < W) acc = fmaf(k[u * 3 + v], ld_f32<T>(xp + (long)iy * W + ix), acc);
            }
        }
        st_f32<T>(yp + i, aff1<AFF>(acc, fa, fb, af.relu));
    }
}
template <typename T, int S>
__global__ __launch_bounds__(256) void dw3_fwd(const T* __restrict__ x, const float* __restrict__ w,
                                               T* __restrict__ y, int C, int H, int W, int Ho, int Wo) {
    dw3_fwd_body<T, S, false>(x, w, y, C, H, W, Ho, Wo, Aff{nullptr, nullptr, 0});
}
template <typename T, int S>
__global__ __launch_bounds__(256) void dw3_fwd_aff(const T* __restrict__ x, const float* __restrict__ w,
                                                   T* __restrict__ y, int C, int H, int W, int Ho, int Wo, Aff af) {
    dw3_fwd_body<T, S, true>(x, w, y, C, H, W, Ho, Wo, af);
}

// dx[iy][ix] = sum_{u,v} w[u][v] * dy[oy][ox]  with  oy*S - 1 + u = iy,  ox*S - 1 + v = ix
template <typename T, int S>
__global__ __launch_bounds__(256) void dw3_bwd(const T* __restrict__ dy, const float* __restrict__ w,
                                               T* __restrict__ dx, int C, int H, int W, int Ho, int Wo) {
    const int plane = blockIdx.y;
    const int c = plane % C;
    const float* wc = w + c * 9;
    float k[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) k[i] = wc[i];
    const T* dp = dy + (long)plane * Ho * Wo;
    T* xp = dx + (long)plane * H * W;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < H * W; i += gridDim.x * 256) {
        const int iy = i / W, ix = i - iy * W;
        float acc = 0.f;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int ty = iy + 1 - u;
            if (ty < 0 || (ty % S) != 0) continue;
            const int oy = ty / S;
            if (oy >= Ho) continue;
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                const int tx = ix + 1 - v;
                if (tx < 0 || (tx % S) != 0) continue;
                const int ox = tx / S;
                if (ox < Wo) acc = fmaf(k[u * 3 + v], ld_f32<T>(dp + (long)oy * Wo + ox), acc);
            }
        }
        st_f32<T>(xp + i, acc);
    }
}


// ---- bf16, 8 outputs per thread ---------------------------------------------------------------------------
// The stem runs these at 96x320 / 192x640 on [12,128,...] tensors (94 MB in, 94 MB out): one 16-byte load per
// input row piece (+ one scalar per side), one 16-byte store; the row taps stay in registers.
struct Bf8 { float v[8]; };
__device__ __forceinline__ Bf8 ld8(const uint16_t* p) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    Bf8 r;
    r.v[0] = __uint_as_float(u.x << 16); r.v[1] = __uint_as_float(u.x & 0xffff0000u);
    r.v[2] = __uint_as_float(u.y << 16); r.v[3] = __uint_as_float(u.y & 0xffff0000u);
    r.v[4] = __uint_as_float(u.z << 16); r.v[5] = __uint_as_float(u.z & 0xffff0000u);
    r.v[6] = __uint_as_float(u.w << 16); r.v[7] = __uint_as_float(u.w & 0xffff0000u);
    return r;
}
__device__ __forceinline__ void st8(uint16_t* p, const float (&a)[8]) {
    uint32_t h[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = f32_to_bf16(a[i]);
    *reinterpret_cast<uint4*>(p) = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
}

// stride 1 (forward, and data gradient with the taps reversed by the caller flag FLIP): W % 8 == 0
template <bool FLIP, bool AFF>
__device__ __forceinline__ void dw3v_s1_body(const uint16_t* __restrict__ x, const float* __restrict__ w,
                                             uint16_t* __restrict__ y, int C, int H, int W, long total, Aff af) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int W8 = W >> 3;
    const int x0 = (int)(idx % W8) * 8;
    const int oy = (int)((idx / W8) % H);
    const long plane = idx / ((long)W8 * H);
    const float* wc = w + (plane % C) * 9;
    float k[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) k[i] = FLIP ? wc[8 - i] : wc[i];
    const uint16_t* xp = x + plane * (long)H * W;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int iy = oy - 1 + u;
        if (iy < 0 || iy >= H) continue;
        const uint16_t* row = xp + (long)iy * W;
        const Bf8 c = ld8(row + x0);
        float in[10];
        in[0] = x0 > 0 ? bf16_to_f32(row[x0 - 1]) : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) in[j + 1] = c.v[j];
        in[9] = x0 + 8 < W ? bf16_to_f32(row[x0 + 8]) : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            acc[j] = fmaf(k[u * 3 + 2], in[j + 2], fmaf(k[u * 3 + 1], in[j + 1], fmaf(k[u * 3], in[j], acc[j])));
    }
    if constexpr (AFF) {
        const float fa = af.s[plane % C], fb = af.o[plane % C];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = aff1<true>(acc[j], fa, fb, af.relu);
    }
    st8(y + (plane * H + oy) * (long)W + x0, acc);
}
template <bool FLIP>
__global__ __launch_bounds__(256) void dw3v_s1(const uint16_t* __restrict__ x, const float* __restrict__ w,
                                               uint16_t* __restrict__ y, int C, int H, int W, long total) {
    dw3v_s1_body<FLIP, false>(x, w, y, C, H, W, total, Aff{nullptr, nullptr, 0});
}
__global__ __launch_bounds__(256) void dw3v_s1_aff(const uint16_t* __restrict__ x, const float* __restrict__ w,
                                                   uint16_t* __restrict__ y, int C, int H, int W, long total, Aff af) {
    dw3v_s1_body<false, true>(x, w, y, C, H, W, total, af);
}

// stride 2 forward: Wo % 8 == 0, W == 2 * Wo
template <bool AFF>
__device__ __forceinline__ void dw3v_s2_fwd_body(const uint16_t* __restrict__ x, const float* __restrict__ w,
                                                 uint16_t* __restrict__ y, int C, int H, int W, int Ho, int Wo,
                                                 long total, Aff af) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int W8 = Wo >> 3;
    const int x0 = (int)(idx % W8) * 8;
    const int oy = (int)((idx / W8) % Ho);
    const long plane = idx / ((long)W8 * Ho);
    const float* wc = w + (plane % C) * 9;
    float k[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) k[i] = wc[i];
    const uint16_t* xp = x + plane * (long)H * W;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int iy = 2 * oy - 1 + u;
        if (iy < 0 || iy >= H) continue;
        const uint16_t* row = xp + (long)iy * W + 2 * x0;
        const Bf8 a = ld8(row), b = ld8(row + 8);
        float in[17];
        in[0] = x0 > 0 ? bf16_to_f32(row[-1]) : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) { in[j + 1] = a.v[j]; in[j + 9] = b.v[j]; }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            acc[j] = fmaf(k[u * 3 + 2], in[2 * j + 2], fmaf(k[u * 3 + 1], in[2 * j + 1], fmaf(k[u * 3], in[2 * j], acc[j])));
    }
    if constexpr (AFF) {
        const float fa = af.s[plane % C], fb = af.o[plane % C];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = aff1<true>(acc[j], fa, fb, af.relu);
    }
    st8(y + (plane * Ho + oy) * (long)Wo + x0, acc);
}
__global__ __launch_bounds__(256) void dw3v_s2_fwd(const uint16_t* __restrict__ x, const float* __restrict__ w,
                                                   uint16_t* __restrict__ y, int C, int H, int W, int Ho, int Wo,
                                                   long total) {
    dw3v_s2_fwd_body<false>(x, w, y, C, H, W, Ho, Wo, total, Aff{nullptr, nullptr, 0});
}
__global__ __launch_bounds__(256) void dw3v_s2_fwd_aff(const uint16_t* __restrict__ x, const float* __restrict__ w,
                                                       uint16_t* __restrict__ y, int C, int H, int W, int Ho, int Wo,
                                                       long total, Aff af) {
    dw3v_s2_fwd_body<true>(x, w, y, C, H, W, Ho, Wo, total, af);
}

// stride 2 data gradient: dx[iy][ix] = sum w[u][v] dy[(iy+1-u)/2][(ix+1-v)/2] over even numerators; W % 8 == 0
__global__ __launch_bounds__(256) void dw3v_s2_bwd(const uint16_t* __restrict__ dy, const float* __restrict__ w,
                                                   uint16_t* __restrict__ dx, int C, int H, int W, int Ho, int Wo,
                                                   long total) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int W8 = W >> 3;
    const int x0 = (int)(idx % W8) * 8;
    const int iy = (int)((idx / W8) % H);
    const long plane = idx / ((long)W8 * H);
    const float* wc = w + (plane % C) * 9;
    float k[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) k[i] = wc[i];
    const uint16_t* dp = dy + plane * (long)Ho * Wo;
    const int ox0 = x0 >> 1;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int ty = iy + 1 - u;
        if (ty < 0 || (ty & 1)) continue;
        const int oy = ty >> 1;
        if (oy >= Ho) continue;
        const uint16_t* row = dp + (long)oy * Wo + ox0;
        const uint2 q = *reinterpret_cast<const uint2*>(row);
        float d[5];
        d[0] = __uint_as_float(q.x << 16); d[1] = __uint_as_float(q.x & 0xffff0000u);
        d[2] = __uint_as_float(q.y << 16); d[3] = __uint_as_float(q.y & 0xffff0000u);
        d[4] = ox0 + 4 < Wo ? bf16_to_f32(row[4]) : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if ((j & 1) == 0) acc[j] = fmaf(k[u * 3 + 1], d[j >> 1], acc[j]);                 // ix even: v = 1
            else acc[j] = fmaf(k[u * 3 + 2], d[(j - 1) >> 1], fmaf(k[u * 3], d[(j + 1) >> 1], acc[j]));   // v = 2, 0
        }
    }
    st8(dx + (plane * H + iy) * (long)W + x0, acc);
}

// ---- dispatch ----------------------------------------------------------------------------------------------
// ONE choice of kernel for the forward, the data gradient and the affine forward (ppea_dwconv3x3_plan is this function):
//   DW3_GENERIC    dw3_fwd / dw3_bwd / dw3_fwd_aff<T, stride>: one thread per pixel, grid (<= 64, planes)
//   DW3_V_S1       dw3v_s1<FLIP> / dw3v_s1_aff: bf16, stride 1, W % 8 == 0
//   DW3_V_S2_FWD   dw3v_s2_fwd / dw3v_s2_fwd_aff: bf16, stride 2, H and W even, Wo % 8 == 0
//   DW3_V_S2_BWD   dw3v_s2_bwd: the data gradient of the same shapes
enum { DW3_GENERIC = 0, DW3_V_S1 = 1, DW3_V_S2_FWD = 2, DW3_V_S2_BWD = 3 };
enum { DW3_MODE_FWD = 0, DW3_MODE_BWD = 1, DW3_MODE_AFFINE = 2 };
inline bool dw3_shape_ok(int N, int C, int H, int W, int stride) {
    return N > 0 && C > 0 && H > 0 && W > 0 && (stride == 1 || stride == 2);
}
inline int dw3_plan(int elem_bytes, int mode, int N, int C, int H, int W, int stride) {
    if ((elem_bytes != 2 && elem_bytes != 4) || mode < DW3_MODE_FWD || mode > DW3_MODE_AFFINE) return PPEA_ERR_UNSUPPORTED;
    if (!dw3_shape_ok(N, C, H, W, stride) || (long)N * C > 65535) return PPEA_ERR_UNSUPPORTED;   // planes ride on gridDim.y
    if (elem_bytes == 2) {                                 // bf16: 8 outputs per thread when the rows allow it
        const int Wo = (W + 2 - 3) / stride + 1;
        if (stride == 1 && (W & 7) == 0) return DW3_V_S1;
        if (stride == 2 && (W & 1) == 0 && (H & 1) == 0 && (Wo & 7) == 0) return mode == DW3_MODE_BWD ? DW3_V_S2_BWD : DW3_V_S2_FWD;
    }
    return DW3_GENERIC;
}

template <typename T>
int run(bool bwd, const void* a, const float* w, void* o, int N, int C, int H, int W, int stride, void* stream) {
    const int arm = dw3_plan((int)sizeof(T), bwd ? DW3_MODE_BWD : DW3_MODE_FWD, N, C, H, W, stride);
    if (arm < 0) return arm;
    const int Ho = (H + 2 - 3) / stride + 1, Wo = (W + 2 - 3) / stride + 1;
    const long planes = (long)N * C;
    hipStream_t st = (hipStream_t)stream;
    const uint16_t* in = (const uint16_t*)a;
    uint16_t* out = (uint16_t*)o;
    switch (arm) {
    case DW3_V_S1: {
        const long total = planes * H * (W >> 3);
        const unsigned blocks = (unsigned)((total + 255) / 256);
        if (!bwd) hipLaunchKernelGGL(dw3v_s1<false>, dim3(blocks), dim3(256), 0, st, in, w, out, C, H, W, total);
        else hipLaunchKernelGGL(dw3v_s1<true>, dim3(blocks), dim3(256), 0, st, in, w, out, C, H, W, total);
        return launch_status();
    }
    case DW3_V_S2_FWD: {
        const long total = planes * Ho * (Wo >> 3);
        hipLaunchKernelGGL(dw3v_s2_fwd, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, in, w, out, C, H, W, Ho, Wo, total);
        return launch_status();
    }
    case DW3_V_S2_BWD: {
        const long total = planes * H * (W >> 3);
        hipLaunchKernelGGL(dw3v_s2_bwd, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, in, w, out, C, H, W, Ho, Wo, total);
        return launch_status();
    }
    default: break;
    }
    const int work = bwd ? H * W : Ho * Wo;
    int bx = (work + 255) / 256;
    if (bx > 64) bx = 64;
    dim3 g(bx, (unsigned)planes);
    if (!bwd) {
        if (stride == 1) hipLaunchKernelGGL((dw3_fwd<T, 1>), g, dim3(256), 0, st, (const T*)a, w, (T*)o, C, H, W, Ho, Wo);
        else hipLaunchKernelGGL((dw3_fwd<T, 2>), g, dim3(256), 0, st, (const T*)a, w, (T*)o, C, H, W, Ho, Wo);
    } else {
        if (stride == 1) hipLaunchKernelGGL((dw3_bwd<T, 1>), g, dim3(256), 0, st, (const T*)a, w, (T*)o, C, H, W, Ho, Wo);
        else hipLaunchKernelGGL((dw3_bwd<T, 2>), g, dim3(256), 0, st, (const T*)a, w, (T*)o, C, H, W, Ho, Wo);
    }
    return launch_status();
}

template <typename T>
int run_affine(const void* a, const float* w, const float* s, const float* o, int relu, void* out_, int N, int C, int H, int W,
               int stride, void* stream) {
    if (!dw3_shape_ok(N, C, H, W, stride)) return PPEA_ERR_UNSUPPORTED;
    if (a == nullptr || w == nullptr || s == nullptr || o == nullptr || out_ == nullptr) return PPEA_ERR_ARG;
    const int arm = dw3_plan((int)sizeof(T), DW3_MODE_AFFINE, N, C, H, W, stride);
    if (arm < 0) return arm;
    const int Ho = (H + 2 - 3) / stride + 1, Wo = (W + 2 - 3) / stride + 1;
    const long planes = (long)N * C;
    hipStream_t st = (hipStream_t)stream;
    const Aff af{s, o, relu};
    const uint16_t* in = (const uint16_t*)a;
    uint16_t* out = (uint16_t*)out_;
    switch (arm) {
    case DW3_V_S1: {
        const long total = planes * H * (W >> 3);
        hipLaunchKernelGGL(dw3v_s1_aff, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, in, w, out, C, H, W, total, af);
        return launch_status();
    }
    case DW3_V_S2_FWD: {
        const long total = planes * Ho * (Wo >> 3);
        hipLaunchKernelGGL(dw3v_s2_fwd_aff, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, in, w, out, C, H, W, Ho,
                           Wo, total, af);
        return launch_status();
    }
    default: break;
    }
    int bx = (Ho * Wo + 255) / 256;
    if (bx > 64) bx = 64;
    dim3 g(bx, (unsigned)planes);
    if (stride == 1) hipLaunchKernelGGL((dw3_fwd_aff<T, 1>), g, dim3(256), 0, st, (const T*)a, w, (T*)out_, C, H, W, Ho, Wo, af);
    else hipLaunchKernelGGL((dw3_fwd_aff<T, 2>), g, dim3(256), 0, st, (const T*)a, w, (T*)out_, C, H, W, Ho, Wo, af);
    return launch_status();
}

// ---- filter gradient (full fine-tuning) --------------------------------------------------------------------
// dw[c][u][v] = sum_{n,oy,ox} dy[n][c][oy][ox] * x[n][c][oy*S+u-1][ox*S+v-1].  grid (C, parts): a part is a band of
// (n, oy) rows; every thread keeps nine fp32 sums over its pixels, the block reduces them (wave shuffles, then the four
// waves in order) into ws[c][part][9].  dwconv3x3_bwd_filter_sum adds the parts in index order: no atomics, a bitwise function of
// the inputs.
template <typename T, int S>
__global__ __launch_bounds__(256) void dwconv3x3_bwd_filter(const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ ws,
                                                 int N, int C, int H, int W, int Ho, int Wo, int rows_per_part) {
    const int c = blockIdx.x, part = blockIdx.y, parts = gridDim.y;
    const long rows = (long)N * Ho;
    const long r0 = (long)part * rows_per_part;
    long r1 = r0 + rows_per_part;
    if (r1 > rows) r1 = rows;
    float acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = 0.f;
    // a wave per (n, oy) row, its lanes over the columns: one division per row and none per pixel
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (long row = r0 + wave; row < r1; row += 4) {
        const int n = (int)(row / Ho), oy = (int)(row - (long)n * Ho);
        const T* dp = dy + (((long)n * C + c) * Ho + oy) * Wo;
        const T* xp = x + ((long)n * C + c) * H * W;
        const int iy0 = oy * S - 1;
        for (int ox = lane; ox < Wo; ox += 64) {
            const float g = ld_f32<T>(dp + ox);
            const int ix0 = ox * S - 1;
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int iy = iy0 + u;
                if (iy < 0 || iy >= H) continue;
#pragma unroll
                for (int v = 0; v < 3; ++v) {
                    const int ix = ix0 + v;
                    if (ix >= 0 && ix < W) acc[u * 3 + v] = fmaf(g, ld_f32<T>(xp + (long)iy * W + ix), acc[u * 3 + v]);
                }
            }
        }
    }
    __shared__ float red[4][9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const float s = wave_sum(acc[t]);
        if (lane == 0) red[wave][t] = s;
    }
    __syncthreads();
    if (threadIdx.x < 9)
        ws[((long)c * parts + part) * 9 + threadIdx.x] =
            ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

__global__ __launch_bounds__(256) void dwconv3x3_bwd_filter_sum(const float* __restrict__ ws, float* __restrict__ dw, int total, int parts) {
    const int i = blockIdx.x * 256 + threadIdx.x;          // c * 9 + t
    if (i >= total) return;
    const int c = i / 9, t = i - c * 9;
    float s = 0.f;
    for (int p = 0; p < parts; ++p) s += ws[((long)c * parts + p) * 9 + t];
    dw[i] = s;
}

inline bool wgrad_shape_ok(int N, int C, int H, int W, int stride) {
    return N > 0 && C > 0 && H > 0 && W > 0 && (stride == 1 || stride == 2) && C <= 65535 * 32;
}
// rows of (n, oy) per part: at least ~8192 output pixels per block, at most 64 parts per channel
inline int wgrad_rows_per_part(int N, int Ho, int Wo) {
    const long rows = (long)N * Ho;
    long parts = ((long)rows * Wo + 8191) / 8192;
    if (parts < 1) parts = 1;
    if (parts > 64) parts = 64;
    if (parts > rows) parts = rows;
    return (int)((rows + parts - 1) / parts);
}
inline int wgrad_parts(int N, int Ho, int Wo) {
    const long rows = (long)N * Ho;
    const int rpp = wgrad_rows_per_part(N, Ho, Wo);
    return (int)((rows + rpp - 1) / rpp);
}

template <typename T>
int run_wgrad(const void* x, const void* dy, float* dw, void* workspace, int N, int C, int H, int W, int stride, void* stream) {
    if (!wgrad_shape_ok(N, C, H, W, stride)) return PPEA_ERR_UNSUPPORTED;
    if (x == nullptr || dy == nullptr || dw == nullptr || workspace == nullptr) return PPEA_ERR_ARG;
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const int rpp = wgrad_rows_per_part(N, Ho, Wo), parts = wgrad_parts(N, Ho, Wo);
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    const dim3 g((unsigned)C, (unsigned)parts);
    if (stride == 1)
        hipLaunchKernelGGL((dwconv3x3_bwd_filter<T, 1>), g, dim3(256), 0, st, (const T*)x, (const T*)dy, ws, N, C, H, W, Ho, Wo, rpp);
    else
        hipLaunchKernelGGL((dwconv3x3_bwd_filter<T, 2>), g, dim3(256), 0, st, (const T*)x, (const T*)dy, ws, N, C, H, W, Ho, Wo, rpp);
    const int r = launch_status();
    if (r != 0) return r;
    hipLaunchKernelGGL(dwconv3x3_bwd_filter_sum, dim3((unsigned)((C * 9 + 255) / 256)), dim3(256), 0, st, ws, dw, C * 9, parts);
    return launch_status();
}

}  // namespace

extern "C" {
// Filter gradient (full fine-tuning, --fullft_reb): dw [C,1,3,3] fp32 = sum_{n,oy,ox} dy[n,c,oy,ox] * x[n,c,oy*s+u-1,ox*s+v-1]
// (zero outside the plane); x [N,C,H,W], dy [N,C,Ho,Wo].  `workspace`: ppea_dwconv3x3_bwd_filter_workspace_bytes bytes of
// device scratch for the per-part sums, added in a fixed order by a second launch (no atomics).  dw is overwritten.
long ppea_dwconv3x3_bwd_filter_workspace_bytes(int N, int C, int H, int W, int stride) {
    if (!wgrad_shape_ok(N, C, H, W, stride)) return PPEA_ERR_UNSUPPORTED;
    return (long)C * wgrad_parts(N, (H - 1) / stride + 1, (W - 1) / stride + 1) * 9 * (long)sizeof(float);
}
int ppea_dwconv3x3_bwd_filter_f32(const void* x, const void* dy, float* dw, void* workspace, int N, int C, int H, int W,
                                  int stride, void* stream) {
    return run_wgrad<float>(x, dy, dw, workspace, N, C, H, W, stride, stream);
}
int ppea_dwconv3x3_bwd_filter_bf16(const void* x, const void* dy, float* dw, void* workspace, int N, int C, int H, int W,
                                   int stride, void* stream) {
    return run_wgrad<uint16_t>(x, dy, dw, workspace, N, C, H, W, stride, stream);
}
// Inference: y = act(s[c] * DW3x3(x)[c] + o[c]), relu != 0: ReLU (eval-mode BatchNorm folded to a table); shapes as
// ppea_dwconv3x3_fwd_*; N * C > 65535 or stride not in {1, 2}: PPEA_ERR_UNSUPPORTED.
int ppea_dwconv3x3_fwd_affine_f32(const void* x, const float* w, const float* s, const float* o, int relu, void* y, int N, int C,
                                  int H, int W, int stride, void* stream) {
    return run_affine<float>(x, w, s, o, relu, y, N, C, H, W, stride, stream);
}
int ppea_dwconv3x3_fwd_affine_bf16(const void* x, const float* w, const float* s, const float* o, int relu, void* y, int N, int C,
                                   int H, int W, int stride, void* stream) {
    return run_affine<uint16_t>(x, w, s, o, relu, y, N, C, H, W, stride, stream);
}
// The kernel the entry points below and the affine ones above launch (host only): elem_bytes 4 (f32) | 2 (bf16); mode 0 forward,
// 1 data gradient, 2 affine forward -> 0 generic, 1 dw3v_s1, 2 dw3v_s2_fwd, 3 dw3v_s2_bwd; PPEA_ERR_UNSUPPORTED exactly where
// they return it.
int ppea_dwconv3x3_plan(int elem_bytes, int mode, int N, int C, int H, int W, int stride) {
    return dw3_plan(elem_bytes, mode, N, C, H, W, stride);
}
// x [N,C,H,W] -> y [N,C,Ho,Wo], Ho = (H-1)/stride + 1; w [C,1,3,3] fp32
int ppea_dwconv3x3_fwd_f32(const void* x, const float* w, void* y, int N, int C, int H, int W, int stride, void* stream) {
    return run<float>(false, x, w, y, N, C, H, W, stride, stream);
}
int ppea_dwconv3x3_fwd_bf16(const void* x, const float* w, void* y, int N, int C, int H, int W, int stride, void* stream) {
    return run<uint16_t>(false, x, w, y, N, C, H, W, stride, stream);
}
// dy [N,C,Ho,Wo] -> dx [N,C,H,W]   (H, W are the INPUT sizes of the forward conv)
int ppea_dwconv3x3_bwd_data_f32(const void* dy, const float* w, void* dx, int N, int C, int H, int W, int stride, void* stream) {
    return run<float>(true, dy, w, dx, N, C, H, W, stride, stream);
}
int ppea_dwconv3x3_bwd_data_bf16(const void* dy, const float* w, void* dx, int N, int C, int H, int W, int stride, void* stream) {
    return run<uint16_t>(true, dy, w, dx, N, C, H, W, stride, stream);
}
}
