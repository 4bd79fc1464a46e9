// Prediction export, gfx950: what a user does with a predicted plane after the network -- metric depth at the frame's own
// size (fp32, or the KITTI benchmark's 16-bit depth * 256, eval_depth_ori.py:325-328), the value range of a plane (minimum,
// maximum or an exact percentile) and a colour-mapped uint8 picture of it (vis.colorize, matplotlib's Colormap.__call__).
//
// Every kernel that resizes uses eval_gather's statement of cv2.resize(INTER_LINEAR) (csrc/eval_metrics.hip): half-pixel
// centres, the source coordinate clamped at 0 (here taken in fp64), the horizontal pair first, then the vertical.  A target
// of the source's own size reads the pixel itself (no zero-weight neighbour takes part, so a NaN stays where it is).
// Targets are the project's ragged table, [B][3] int64 rows of (offset, H, W): images on grid axis y, fixed chunks of an
// image's pixels on axis x, one launch whatever the sizes.  A row that does not fit the output buffer writes nothing.
//   disp_export  resize + reciprocal + per-image scale + clamp (+ truncation to uint16): 1 launch
//   plane_range  one workgroup per image; radix select on the order-mapped fp32 bit pattern, 8 bits per pass, 3 selections
//                (rank 0 and the percentile's two neighbours) over LDS histograms, integer atomics only; the interpolation
//                between the neighbours in fp64, rounded once: 1 launch, bitwise reproducible
//   colorize     resize + normalise + LUT (in LDS) + pack: 1 launch; a lane owns four pixels whose 12 bytes start on a
//                dword of the output and writes them as three dwords, the pixels of a quad that belong to no image or to a
//                neighbouring one are left alone (the first and last quad of an image are written byte by byte)
#include "common.h"
#include "export_sample.h"

namespace {

constexpr int THREADS = 256;
constexpr int CHUNK = 2048;                 // pixels of one image per workgroup
constexpr int SEL_THREADS = 1024;
constexpr int NSEL = 3;                     // rank 0, the percentile's lower and upper neighbour
constexpr int BINS = 256;

using export_sample::Target;
using export_sample::target_of;
using export_sample::sample;
using export_sample::depth_of;

__device__ __forceinline__ void put_depth(float* p, float d) { *p = d; }
// np.uint16(depth * 256): truncation of the fp32 product (depth <= hi, hi * 256 <= 65535 checked by the launcher)
__device__ __forceinline__ void put_depth(uint16_t* p, float d) { *p = (uint16_t)(uint32_t)(d * 256.0f); }

template <typename OutT, bool RECIP>
__global__ __launch_bounds__(THREADS) void disp_export(const float* __restrict__ pred, const float* __restrict__ scale,
                                                       const int64_t* __restrict__ table, OutT* __restrict__ out,
                                                       long out_len, int h, int w, float lo, float hi) {
    const int b = blockIdx.y;
    const Target t = target_of(table, b, out_len);
    const long base = (long)blockIdx.x * CHUNK;
    if (base >= t.size) return;
    const float* p = pred + (long)b * h * w;
    const double sy = (double)h / (double)t.H, sx = (double)w / (double)t.W;
    const float sc = scale[b];
#pragma unroll
    for (int it = 0; it < CHUNK / THREADS; ++it) {
        const long i = base + it * THREADS + threadIdx.x;
        if (i >= t.size) break;
        const float r = sample<RECIP>(p, h, w, t, sy, sx, (int)i);
        float d = depth_of<RECIP>(sc, r);
        d = d < lo ? lo : d;                  // np.clip: a NaN stays a NaN
        d = d > hi ? hi : d;
        put_depth(out + t.off + i, d);
    }
}

// fp32 bit pattern -> unsigned key of the same order (negative values reversed below the positive ones), and back
__device__ __forceinline__ uint32_t order_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// Wave s < NSEL follows selection s through the LDS histogram of this pass: the digit that holds rank[s], and the rank
// inside that digit's bin.
__device__ void resolve_pass(const int (*hist)[BINS], const int* alias, int* rank, uint32_t* prefix) {
    const int s = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    if (s >= NSEL) return;
    const int* hp = hist[alias[s]] + lane * 4;
    const int c0 = hp[0], c1 = hp[1], c2 = hp[2], c3 = hp[3];
    const int local = c0 + c1 + c2 + c3;
    int incl = local;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int u = __shfl_up(incl, o, WAVE);
        if (lane >= o) incl += u;
    }
    const int excl = incl - local;
    const int k = rank[s];
    const bool mine = k >= excl && k < incl;
    int digit = 0, rest = 0;
    if (mine) {
        const int q = k - excl;
        if (q < c0) digit = 0, rest = q;
        else if (q < c0 + c1) digit = 1, rest = q - c0;
        else if (q < c0 + c1 + c2) digit = 2, rest = q - c0 - c1;
        else digit = 3, rest = q - c0 - c1 - c2;
        digit += lane * 4;
    }
    const unsigned long long who = __ballot(mine);
    const int from = who ? __ffsll((long long)who) - 1 : 0;
    digit = __shfl(digit, from, WAVE);
    rest = __shfl(rest, from, WAVE);
    if (lane == 0) {
        prefix[s] = (prefix[s] << 8) | (uint32_t)digit;
        rank[s] = rest;
    }
}

__global__ __launch_bounds__(SEL_THREADS) void plane_range(const float* __restrict__ x, float* __restrict__ range, long n,
                                                           double quantile) {
    const int b = blockIdx.x;
    const float* p = x + (long)b * n;
    const int lane = threadIdx.x & (WAVE - 1);
    __shared__ int hist[NSEL][BINS];
    __shared__ int alias[NSEL];           // selections with equal leading digits share the histogram of the first of them
    __shared__ int rank[NSEL];
    __shared__ uint32_t prefix[NSEL];
    __shared__ int valid;
    __shared__ double gamma;
    const long rounded = (n + SEL_THREADS - 1) / SEL_THREADS * SEL_THREADS;      // whole waves stay together
    for (int pass = 0; pass < 4; ++pass) {
        for (int i = threadIdx.x; i < NSEL * BINS; i += SEL_THREADS) (&hist[0][0])[i] = 0;
        if (threadIdx.x == 0) {
            if (pass == 0) prefix[0] = prefix[1] = prefix[2] = 0;
            alias[0] = 0;
            alias[1] = prefix[1] == prefix[0] ? 0 : 1;
            alias[2] = prefix[2] == prefix[0] ? 0 : prefix[2] == prefix[1] ? 1 : 2;
        }
        __syncthreads();
        const int shift = 24 - 8 * pass;
        const int a1 = alias[1], a2 = alias[2];
        const uint32_t p0 = prefix[0], p1 = prefix[1], p2 = prefix[2];
        for (long i = threadIdx.x; i < rounded; i += SEL_THREADS) {
            const float v = i < n ? p[i] : __uint_as_float(0x7fc00000u);
            const bool ok = v == v;                                               // NaNs take no part
            const uint32_t key = order_key(v);
            const uint32_t high = pass ? (key >> shift) >> 8 : 0;
            const int d = (key >> shift) & 255;
#pragma unroll
            for (int s = 0; s < NSEL; ++s) {
                if (s == 1 && a1 != 1) continue;
                if (s == 2 && a2 != 2) continue;
                const bool m = ok && high == (s == 0 ? p0 : s == 1 ? p1 : p2);
                const unsigned long long who = __ballot(m);
                if (!who) continue;
                // a smooth plane puts a whole wave into one bin of the leading passes: one add of the count then
                const int first = __ffsll((long long)who) - 1;
                const int d0 = __shfl(d, first, WAVE);
                if (__ballot(m && d == d0) == who) {
                    if (lane == first) atomicAdd(&hist[s][d0], __popcll(who));
                } else if (m) {
                    atomicAdd(&hist[s][d], 1);
                }
            }
        }
        __syncthreads();
        if (pass == 0) {
            if (threadIdx.x < WAVE) {
                const int* hp = hist[0] + lane * 4;
                int c = hp[0] + hp[1] + hp[2] + hp[3];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, WAVE);
                if (lane == 0) {
                    valid = c;
                    // np.percentile's default (linear) rule: virtual index n q + (1 - q) - 1 in fp64, its neighbours
                    const double vi = (double)c * quantile + (1.0 + quantile * -1.0) - 1.0;
                    double fl = floor(vi);
                    long lo = (long)fl, hi = lo + 1;
                    lo = lo < 0 ? 0 : lo > c - 1 ? c - 1 : lo;
                    hi = hi < 0 ? 0 : hi > c - 1 ? c - 1 : hi;
                    rank[0] = 0, rank[1] = (int)lo, rank[2] = (int)hi;
                    gamma = vi - fl;
                }
            }
            __syncthreads();
            if (valid == 0) {                                                      // uniform: nothing to select
                if (threadIdx.x < 2) range[b * 2 + threadIdx.x] = __uint_as_float(0x7fc00000u);
                return;
            }
        }
        resolve_pass(hist, alias, rank, prefix);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double lo = (double)key_value(prefix[1]), hi = (double)key_value(prefix[2]), t = gamma;
        const double diff = hi - lo;
        const double v = t >= 0.5 ? hi - diff * (1.0 - t) : lo + diff * t;         // numpy's _lerp
        range[b * 2] = key_value(prefix[0]);
        range[b * 2 + 1] = prefix[1] == prefix[2] ? key_value(prefix[1]) : (float)v;
    }
}

// matplotlib's Colormap.__call__(bytes=True), N = 256, for x = (v - vmin) / (vmax - vmin): the LUT row, packed in 24 bits
__device__ __forceinline__ uint32_t colour_of(float v, float vmin, float vmax, const uint8_t* lut) {
    const float x = vmin != vmax ? (v - vmin) / (vmax - vmin) : v * 0.f;
    if (!(x == x)) return 0u;                                   // bad: (0, 0, 0)
    const float t = x * 256.0f;
    const int idx = t < 0.f ? 0 : t >= 256.0f ? 255 : (int)t;   // under: row 0, over (and x == 1): row 255
    const uint8_t* c = lut + idx * 3;
    return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16);
}

constexpr int QUAD_CHUNK = CHUNK / 4;       // quads per workgroup

__global__ __launch_bounds__(THREADS) void colorize(const float* __restrict__ x, const float* __restrict__ range,
                                                    const uint8_t* __restrict__ lut_g, const int64_t* __restrict__ table,
                                                    uint8_t* __restrict__ out, long out_len, int h, int w) {
    const int b = blockIdx.y;
    const Target t = target_of(table, b, out_len);
    // quads are counted in the flat buffer from the multiple of 4 at or below the image's first pixel: pixel 4 q sits at
    // byte 12 q of an output whose base is dword-aligned
    const long first_quad = t.off >> 2;
    const long lead = t.off & 3;                                 // pixels of the first quad that precede the image
    const long quads = (lead + t.size + 3) >> 2;
    const long qbase = (long)blockIdx.x * QUAD_CHUNK;
    if (t.size == 0 || qbase >= quads) return;
    __shared__ uint32_t lut_w[192];
    if (threadIdx.x < 192) lut_w[threadIdx.x] = ((const uint32_t*)lut_g)[threadIdx.x];
    __syncthreads();
    const uint8_t* lut = (const uint8_t*)lut_w;
    const float* p = x + (long)b * h * w;
    const double sy = (double)h / (double)t.H, sx = (double)w / (double)t.W;
    const float vmin = range[b * 2], vmax = range[b * 2 + 1];
#pragma unroll
    for (int it = 0; it < QUAD_CHUNK / THREADS; ++it) {
        const long q = qbase + it * THREADS + threadIdx.x;
        if (q >= quads) break;
        const long i0 = q * 4 - lead;                            // image pixel of the quad's first slot (may be < 0)
        uint32_t c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long i = i0 + k;
            c[k] = (i >= 0 && i < t.size) ? colour_of(sample<false>(p, h, w, t, sy, sx, (int)i), vmin, vmax, lut) : 0u;
        }
        uint8_t* dst = out + (first_quad + q) * 12;
        if (i0 >= 0 && i0 + 4 <= t.size) {
            uint32_t* d = (uint32_t*)dst;
            d[0] = c[0] | (c[1] << 24);
            d[1] = (c[1] >> 8) | (c[2] << 16);
            d[2] = (c[2] >> 16) | (c[3] << 8);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long i = i0 + k;
                if (i >= 0 && i < t.size) {
                    dst[k * 3] = (uint8_t)c[k];
                    dst[k * 3 + 1] = (uint8_t)(c[k] >> 8);
                    dst[k * 3 + 2] = (uint8_t)(c[k] >> 16);
                }
            }
        }
    }
}

inline bool bad_batch(int B, int h, int w, long out_len, long max_pixels) {
    return B <= 0 || B > 65535 || h <= 0 || w <= 0 || h > 0x7fffffff / w || out_len <= 0 || max_pixels <= 0;
}

template <typename OutT>
int launch_export(const float* pred, const float* scale, const int64_t* table, OutT* out, long out_len, int B, int h, int w,
                  long max_pixels, float lo, float hi, int mode, void* stream) {
    if (!pred || !scale || !table || !out || bad_batch(B, h, w, out_len, max_pixels)) return PPEA_ERR_ARG;
    if (!(lo <= hi)) return PPEA_ERR_ARG;
    if (mode != 0 && mode != 1) return PPEA_ERR_UNSUPPORTED;
    if (max_pixels > 0x7fffffffL) return PPEA_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((max_pixels + CHUNK - 1) / CHUNK), B);
    hipStream_t st = (hipStream_t)stream;
    if (mode == 1)
        disp_export<OutT, true><<<grid, THREADS, 0, st>>>(pred, scale, table, out, out_len, h, w, lo, hi);
    else
        disp_export<OutT, false><<<grid, THREADS, 0, st>>>(pred, scale, table, out, out_len, h, w, lo, hi);
    return launch_status();
}

}  // namespace

extern "C" int ppea_disp_export_f32(const float* pred, const float* scale, const int64_t* table, float* out, long out_len,
                                    int B, int h, int w, long max_pixels, float lo, float hi, int mode, void* stream) {
    return launch_export(pred, scale, table, out, out_len, B, h, w, max_pixels, lo, hi, mode, stream);
}

extern "C" int ppea_disp_export_u16(const float* pred, const float* scale, const int64_t* table, uint16_t* out,
                                    long out_len, int B, int h, int w, long max_pixels, float lo, float hi, int mode,
                                    void* stream) {
    if (!(lo >= 0.f) || !(hi * 256.0f <= 65535.0f)) return PPEA_ERR_ARG;      // the truncation must fit 16 bits
    return launch_export(pred, scale, table, out, out_len, B, h, w, max_pixels, lo, hi, mode, stream);
}

extern "C" int ppea_plane_range_f32(const float* x, float* range, int B, long n, double percentile, void* stream) {
    if (!x || !range || B <= 0 || n <= 0) return PPEA_ERR_ARG;
    if (!(percentile >= 0.0 && percentile <= 100.0)) return PPEA_ERR_ARG;
    if (n > 0x7fffffffL - SEL_THREADS) return PPEA_ERR_UNSUPPORTED;
    plane_range<<<B, SEL_THREADS, 0, (hipStream_t)stream>>>(x, range, n, percentile / 100.0);
    return launch_status();
}

extern "C" int ppea_colorize_u8(const float* x, const float* range, const uint8_t* lut, const int64_t* table, uint8_t* out,
                                long out_len, int B, int h, int w, long max_pixels, void* stream) {
    if (!x || !range || !lut || !table || !out || bad_batch(B, h, w, out_len, max_pixels)) return PPEA_ERR_ARG;
    if (((uintptr_t)out & 3) || ((uintptr_t)lut & 3)) return PPEA_ERR_ARG;    // dword stores, dword loads of the LUT
    if (max_pixels > 0x7fffffffL) return PPEA_ERR_UNSUPPORTED;
    // an image that does not start on a multiple of 4 pixels spreads over one quad more
    const dim3 grid((unsigned)((max_pixels + 6 + CHUNK - 1) / CHUNK), B);
    colorize<<<grid, THREADS, 0, (hipStream_t)stream>>>(x, range, lut, table, out, out_len, h, w);
    return launch_status();
}
