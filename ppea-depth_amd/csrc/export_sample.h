// The resize and the depth rule of the prediction export, shared by depth_export.hip and point_cloud.hip: eval_gather's
// statement of cv2.resize(INTER_LINEAR) (csrc/eval_metrics.hip) -- half-pixel centres, the source coordinate clamped at 0
// (here taken in fp64), the horizontal pair first, then the vertical -- and the one IEEE division behind it.  A target of
// the source's own size reads the pixel itself (no zero-weight neighbour takes part, so a NaN stays where it is).
#pragma once
#include "common.h"

namespace export_sample {

struct Target {
    long off;              // first pixel of the image in the flat output
    int H, W;
    long size;             // H * W, 0 for a row that does not fit
};

__device__ __forceinline__ Target target_of(const int64_t* __restrict__ table, int b, long out_len) {
    Target t;
    t.off = table[b * 3];
    const long H = table[b * 3 + 1], W = table[b * 3 + 2];
    t.H = (int)H, t.W = (int)W;
    t.size = H * W;
    if (H <= 0 || W <= 0 || H > 0x7fffffffL / W || t.off < 0 || t.off > out_len || t.size > out_len - t.off) t.size = 0;
    return t;
}

// Source index and weights for one axis, eval_metrics.hip's `source` with the coordinate s = max((o + 0.5) n_in / n_out -
// 0.5, 0) taken in fp64 and the weight s - i0 rounded once to fp32: an fp32 coordinate near column 640 is 4e-5 off, which
// at a noisy pixel is more than the 1e-5 the exported depth is held to; the interpolation itself stays fp32.
__device__ __forceinline__ void source(double scale, int dst, int in, int& i0, int& step, float& l0, float& l1) {
    double s = ((double)dst + 0.5) * scale - 0.5;
    s = s < 0.0 ? 0.0 : s;
    i0 = min((int)s, in - 1);
    step = i0 < in - 1 ? 1 : 0;
    l1 = fminf(fmaxf((float)(s - (double)i0), 0.f), 1.f);
    l0 = 1.f - l1;
}

// The resized value of plane p [h][w] at pixel (y, x) of a [H][W] target.  RECIP: the reciprocals of the four sources are
// interpolated (val_ddad resizes the depth).
template <bool RECIP>
__device__ __forceinline__ float sample_yx(const float* __restrict__ p, int h, int w, const Target& t, double sy, double sx,
                                           int y, int x) {
    if (t.H == h && t.W == w) {
        const float v = p[(long)y * w + x];
        return RECIP ? 1.f / v : v;
    }
    int yi, yp, xi, xp;
    float ly0, ly1, lx0, lx1;
    source(sy, y, h, yi, yp, ly0, ly1);
    source(sx, x, w, xi, xp, lx0, lx1);
    const float* row0 = p + (long)yi * w;
    const float* row1 = row0 + (long)yp * w;
    float a = row0[xi], c = row0[xi + xp], e = row1[xi], f = row1[xi + xp];
    if (RECIP) a = 1.f / a, c = 1.f / c, e = 1.f / e, f = 1.f / f;
    return ly0 * (lx0 * a + lx1 * c) + ly1 * (lx0 * e + lx1 * f);
}

// ... at pixel i = y * W + x
template <bool RECIP>
__device__ __forceinline__ float sample(const float* __restrict__ p, int h, int w, const Target& t, double sy, double sx,
                                        int i) {
    if (t.H == h && t.W == w) return RECIP ? 1.f / p[i] : p[i];
    const int y = i / t.W;
    return sample_yx<RECIP>(p, h, w, t, sy, sx, y, i - y * t.W);
}

// Metric depth before the clamp: scale / resize(pred), or scale * resize(1 / pred)
template <bool RECIP>
__device__ __forceinline__ float depth_of(float sc, float r) { return RECIP ? sc * r : sc / r; }

}  // namespace export_sample
