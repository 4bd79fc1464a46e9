// Input pipeline on uint8 frames, gfx950: Pillow's LANCZOS resize (Resample.c, 8-bit images) and torchvision's PIL-path
// ColorJitter (ImageEnhance blends, Convert.c RGB <-> HSV), bit for bit (ppeadepth/input_pipeline.py is the readable
// restatement; tests/test_input_pipeline_gpu.py compares every byte).
//
//   lanczos_h_view   the horizontal pass; every source is a window of a larger image given by byte strides (dense planar
//               frames are the strides pixel 1, row Win, channel H * Win, image C * H * Win).  One workgroup stages `rpb`
//               whole input rows in LDS (mirrored when the item is flipped, so a flipped frame is never materialised),
//               then one thread per output pixel: int32 accumulator from 1 << 21 over the row's (xmin, n, coeffs[n])
//               entry of the tap table, >> 22, clip.  Every input byte is read exactly once, so the same pass marks the
//               images that hold a non-zero byte (a missing neighbour frame is all zeros).  Planar output.
//   lanczos_h_view3   its specialisation for interleaved RGB (a JPEG decoder's HWC): a row's window staged once in 16-byte
//               chunks and written as three channel rows.  One host function launches either for both entry points.
//   lanczos_h_ragged3   the same staging and accumulation (one copy of each: stage_chunk3, resample_pixel3) for frames of
//               DIFFERENT sizes packed into one buffer: what is uniform there (width, tap table, output row) is per row here.
//   lanczos_v   the same arithmetic down the columns of the 8-bit intermediate, 4 columns per thread through 32-bit words
//               when the row length allows.  lanczos_v_ragged: per image its own height and its class's table.
//   jitter_sum  the item's pointwise operations that precede contrast, then Pillow's RGB -> L; an exact integer sum per
//               2048- or 4096-pixel chunk (no atomics: the partial sums are added again, in order, by every workgroup of
//               the second launch).
//   jitter_out  reads the resized uint8 image once, recomputes the chain with int(mean(L) + 0.5) known and writes `color`
//               and `color_aug` as fp32 x / 255 (one IEEE division, as ToTensor).
// Arithmetic rules: integer where Pillow is integer; fp32 / fp64 operations one at a time in Pillow's order (the file is
// built with -ffp-contract=off), true divisions, no fast-math intrinsic.  All operations of an item are uniform over a
// workgroup (one image per blockIdx.y), so the order switch does not diverge.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int PRECISION_BITS = 32 - 8 - 2;      // Pillow Resample.c
constexpr int MAX_SRCS = 8;
constexpr int MAX_RPB = 32;                     // rows per workgroup of the horizontal pass
constexpr int LDS_LIMIT = 60 * 1024;
constexpr int PARAM_WORDS = 10;                 // order[4], brightness, contrast, saturation (fp32 bits), hue shift, apply, pad
constexpr int JITTER_ITERS = 4;                 // pixel groups per thread and chunk

struct Srcs {
    const uint8_t* p[MAX_SRCS];
};

__host__ __device__ __forceinline__ int clip8(int acc) {
    acc >>= PRECISION_BITS;                     // arithmetic shift, as Pillow's
    return acc < 0 ? 0 : (acc > 255 ? 255 : acc);
}

// One tap-table row, clamped to the input so that a malformed table cannot index outside it.
struct Taps {
    const int* c;
    int lo, n;
};
__device__ __forceinline__ Taps taps_of(const int* __restrict__ table, int kmax, int i, int insize) {
    const int* t = table + (long)i * (2 + kmax);
    Taps r;
    r.lo = min(max(t[0], 0), insize);
    r.n = min(min(max(t[1], 0), kmax), insize - r.lo);
    r.c = t + 2;
    return r;
}

// ---- horizontal pass: every source is a window of a larger image, described by byte strides ------------------------
// Rows of all images are numbered through; a workgroup's per-row bookkeeping lies behind the staged rows in the dynamic
// LDS region (no static LDS: the region's base stays 16-byte aligned for the 128-bit writes).
constexpr int VIEW_CHUNK = 16;                  // bytes per wide load
constexpr int VIEW_META = MAX_RPB * (int)(sizeof(const uint8_t*) + 2 * sizeof(int));

struct ViewRows {
    const uint8_t** src;
    int *flip, *nz;
};
__device__ __forceinline__ ViewRows view_rows(uint8_t* smem, size_t line_bytes) {
    ViewRows v;
    v.src = (const uint8_t**)(smem + line_bytes);           // line_bytes % 16 == 0
    v.flip = (int*)(v.src + MAX_RPB);
    v.nz = v.flip + MAX_RPB;
    return v;
}
__device__ __forceinline__ const uint8_t* view_base(const Srcs& srcs, int s) {
    const uint8_t* base = nullptr;
#pragma unroll
    for (int k = 0; k < MAX_SRCS; ++k) base = k == s ? srcs.p[k] : base;
    return base;
}

// Interleaved pixels (pixel stride 3, channel stride 1).  A row's window, L = Win * 3 bytes at p, is staged ONCE, as it
// lies in memory: 16-byte chunks at the alignment the source has (a window that starts at x0 * 3 is in general not
// aligned), the partial chunk at either end byte by byte, so no byte outside the window is read.  stage_chunk3 is chunk j
// of that: -> whether it held a non-zero byte.
__device__ __forceinline__ bool stage_chunk3(const uint8_t* p, int L, int j, uint8_t* row) {
    const int b0 = j * VIEW_CHUNK - (int)((uintptr_t)p % VIEW_CHUNK);      // the chunk's first byte, window-relative
    uint8_t* out = row + j * VIEW_CHUNK;
    bool nz = false;
    if (b0 >= 0 && b0 + VIEW_CHUNK <= L) {
        const uint4 v = *(const uint4*)(p + b0);
        *(uint4*)out = v;
        nz = (v.x | v.y | v.z | v.w) != 0;
    } else {
        for (int q = 0; q < VIEW_CHUNK; ++q) {
            const int b = b0 + q;
            if (b >= 0 && b < L) {
                const uint8_t v = p[b];
                out[q] = v;
                nz |= v != 0;
            }
        }
    }
    return nz;
}

// One output pixel of a staged row (`row`: where stage_chunk3 put the bytes of p): the three channels written `plane`
// apart; a flipped image is read mirrored.
__device__ __forceinline__ void resample_pixel3(const uint8_t* row, const uint8_t* p, const Taps t, int Win, bool flip,
                                                uint8_t* o, long plane) {
    const uint8_t* in = row + (int)((uintptr_t)p % VIEW_CHUNK);
    const int first = flip ? Win - 1 - t.lo : t.lo, step = flip ? -3 : 3;
    in += first * 3;
    int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
    for (int k = 0; k < t.n; ++k, in += step) {
        const int c = t.c[k];
        a0 += (int)in[0] * c, a1 += (int)in[1] * c, a2 += (int)in[2] * c;
    }
    o[0] = (uint8_t)clip8(a0), o[plane] = (uint8_t)clip8(a1), o[2 * plane] = (uint8_t)clip8(a2);
}

// Frames of one size: rows g = image * H + y.  One thread per chunk stages, then one thread per output pixel.
__global__ __launch_bounds__(THREADS) void lanczos_h_view3(Srcs srcs, int items_per_src, long row_stride, long item_stride,
                                                           const int* __restrict__ table, int kmax,
                                                           const int* __restrict__ flip, int* __restrict__ nonzero,
                                                           uint8_t* __restrict__ dst, long rows, int H, int Win, int Wout,
                                                           int rpb, int pitch) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];      // [rpb][pitch], then the rows' bookkeeping
    const ViewRows vr = view_rows(smem, (size_t)rpb * pitch);
    const long row0 = (long)blockIdx.x * rpb;
    const int nr = (int)min((long)rpb, rows - row0);
    if (threadIdx.x < nr) {
        const long g = row0 + threadIdx.x;
        const long n = g / H;
        const int s = (int)(n / items_per_src);
        vr.src[threadIdx.x] = view_base(srcs, s) + (n - (long)s * items_per_src) * item_stride + (g - n * H) * row_stride;
        vr.flip[threadIdx.x] = flip && flip[n] != 0;
        vr.nz[threadIdx.x] = 0;
    }
    __syncthreads();
    const int L = Win * 3, chunks = pitch / VIEW_CHUNK;
    for (int i = threadIdx.x; i < nr * chunks; i += THREADS) {
        const int r = i / chunks, j = i - r * chunks;
        if (stage_chunk3(vr.src[r], L, j, smem + (size_t)r * pitch)) vr.nz[r] = 1;      // every writer stores the same value
    }
    __syncthreads();
    if (nonzero && threadIdx.x < nr && vr.nz[threadIdx.x]) {
        int* flag = nonzero + (row0 + threadIdx.x) / H;
        if (__atomic_load_n(flag, __ATOMIC_RELAXED) == 0) atomicOr(flag, 1);
    }
    const long plane = (long)H * Wout;
    for (int i = threadIdx.x; i < nr * Wout; i += THREADS) {
        const int r = i / Wout, x = i - r * Wout;
        const long g = row0 + r, n = g / H;
        resample_pixel3(smem + (size_t)r * pitch, vr.src[r], taps_of(table, kmax, x, Win), Win, vr.flip[r] != 0,
                        dst + (n * 3 * H + (g - n * H)) * Wout + x, plane);
    }
}

// Frames of different sizes, packed back to back in ONE buffer (a real KITTI batch mixes the recording days' sizes):
// desc [N] = (byte offset, H, W, size class), H = W = 0 an absent frame; prefix [N + 1] numbers the rows of all images
// through, so a workgroup's `rpb` rows may belong to images of different widths and classes.  A row's bookkeeping thread
// finds its image by binary search in `prefix` (N is a few dozen) and notes, per row, what lanczos_h_view3 has uniform:
// the width, the offset of the class's table in tables [K][Wout][2 + kmax] and the output row in dst [N][3][Hcap][Wout]
// (rows >= H are not written).  A row whose descriptor does not lie inside the buffer, the staged pitch or Hcap gets
// width 0: nothing of it is read or written (the entry point refuses such descriptors before the launch).
constexpr int RAGGED_META = MAX_RPB * (int)(2 * sizeof(void*) + 6 * sizeof(int));

// desc [n] = (byte offset, H, W, size class); the table need not be 16-byte aligned
__device__ __forceinline__ int4 desc_of(const int* __restrict__ desc, int n) {
    const int* d = desc + 4L * n;
    return make_int4(d[0], d[1], d[2], d[3]);
}

struct RaggedRows {
    ViewRows v;
    long* out;
    int *win, *tab, *img;
};
__device__ __forceinline__ RaggedRows ragged_rows(uint8_t* smem, size_t line_bytes) {
    RaggedRows r;
    r.v.src = (const uint8_t**)(smem + line_bytes);         // line_bytes % 16 == 0
    r.out = (long*)(r.v.src + MAX_RPB);
    r.v.flip = (int*)(r.out + MAX_RPB);
    r.v.nz = r.v.flip + MAX_RPB;
    r.win = r.v.nz + MAX_RPB;
    r.tab = r.win + MAX_RPB;
    r.img = r.tab + MAX_RPB;
    return r;
}

__global__ __launch_bounds__(THREADS) void lanczos_h_ragged3(const uint8_t* __restrict__ buf, long buf_bytes,
                                                             const int* __restrict__ desc, const int* __restrict__ prefix,
                                                             int N, const int* __restrict__ tables, int K, int kmax,
                                                             const int* __restrict__ flip, int* __restrict__ nonzero,
                                                             uint8_t* __restrict__ dst, int rows, int Hcap, int Wout,
                                                             int rpb, int pitch) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];      // [rpb][pitch], then the rows' bookkeeping
    const RaggedRows rr = ragged_rows(smem, (size_t)rpb * pitch);
    const int row0 = blockIdx.x * rpb;
    const int nr = min(rpb, rows - row0);
    if (threadIdx.x < nr) {
        const int g = row0 + threadIdx.x;
        int n = 0, hi = N - 1;                  // the last image that starts at or before row g: an absent one has no rows
        while (n < hi) {
            const int mid = (n + hi + 1) >> 1;
            if (prefix[mid] <= g) n = mid;
            else hi = mid - 1;
        }
        const int4 d = desc_of(desc, n);
        const int y = g - prefix[n], W = d.z;
        const bool ok = d.x >= 0 && y >= 0 && y < d.y && d.y <= Hcap && W > 0 && (long)W * 3 + (VIEW_CHUNK - 1) <= pitch &&
                        d.x + (long)d.y * W * 3 <= buf_bytes;
        rr.v.src[threadIdx.x] = ok ? buf + d.x + (long)y * W * 3 : buf;
        rr.out[threadIdx.x] = ((long)n * 3 * Hcap + y) * Wout;
        rr.v.flip[threadIdx.x] = flip && flip[n] != 0;
        rr.v.nz[threadIdx.x] = 0;
        rr.win[threadIdx.x] = ok ? W : 0;
        rr.tab[threadIdx.x] = min(max(d.w, 0), K - 1) * Wout * (2 + kmax);
        rr.img[threadIdx.x] = n;
    }
    __syncthreads();
    const int chunks = pitch / VIEW_CHUNK;
    for (int i = threadIdx.x; i < nr * chunks; i += THREADS) {
        const int r = i / chunks, j = i - r * chunks;
        const int L = rr.win[r] * 3;
        if (j * VIEW_CHUNK >= L + VIEW_CHUNK - 1) continue;             // behind a row narrower than the widest class
        if (stage_chunk3(rr.v.src[r], L, j, smem + (size_t)r * pitch)) rr.v.nz[r] = 1;
    }
    __syncthreads();
    if (nonzero && threadIdx.x < nr && rr.v.nz[threadIdx.x]) {
        int* flag = nonzero + rr.img[threadIdx.x];
        if (__atomic_load_n(flag, __ATOMIC_RELAXED) == 0) atomicOr(flag, 1);
    }
    const long plane = (long)Hcap * Wout;
    for (int i = threadIdx.x; i < nr * Wout; i += THREADS) {
        const int r = i / Wout, x = i - r * Wout;
        const int Win = rr.win[r];
        if (Win == 0) continue;
        resample_pixel3(smem + (size_t)r * pitch, rr.v.src[r], taps_of(tables + rr.tab[r], kmax, x, Win), Win,
                        rr.v.flip[r] != 0, dst + rr.out[r] + x, plane);
    }
}

// Any other strides, dense planar frames among them (pixel stride 1, row stride Win, channel stride H * Win): rows
// g = (image * C + c) * H + y, as the planar output numbers them.  One workgroup stages `rpb` whole rows, fetched byte by
// byte through the pixel stride and written mirrored when the image is flipped, then one thread per output pixel.
__global__ __launch_bounds__(THREADS) void lanczos_h_view(Srcs srcs, int items_per_src, int C, long pixel_stride,
                                                          long row_stride, long channel_stride, long item_stride,
                                                          const int* __restrict__ table, int kmax,
                                                          const int* __restrict__ flip, int* __restrict__ nonzero,
                                                          uint8_t* __restrict__ dst, long rows, int H, int Win, int Wout,
                                                          int rpb, int pitch) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];      // [rpb][pitch], then the rows' bookkeeping
    const ViewRows vr = view_rows(smem, (size_t)rpb * pitch);
    const long row0 = (long)blockIdx.x * rpb;
    const int nr = (int)min((long)rpb, rows - row0);
    const long rows_per_item = (long)C * H;
    if (threadIdx.x < nr) {
        const long g = row0 + threadIdx.x;
        const long n = g / rows_per_item, pl = g / H;
        const int s = (int)(n / items_per_src);
        vr.src[threadIdx.x] = view_base(srcs, s) + (n - (long)s * items_per_src) * item_stride +
                              (pl - n * C) * channel_stride + (g - pl * H) * row_stride;
        vr.flip[threadIdx.x] = flip && flip[n] != 0;
        vr.nz[threadIdx.x] = 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nr * Win; i += THREADS) {
        const int r = i / Win, x = i - r * Win;
        const uint8_t v = vr.src[r][x * pixel_stride];
        smem[(size_t)r * pitch + (vr.flip[r] ? Win - 1 - x : x)] = v;
        if (v) vr.nz[r] = 1;                    // every writer stores the same value
    }
    __syncthreads();
    if (nonzero && threadIdx.x < nr && vr.nz[threadIdx.x]) {
        int* flag = nonzero + (row0 + threadIdx.x) / rows_per_item;
        if (__atomic_load_n(flag, __ATOMIC_RELAXED) == 0) atomicOr(flag, 1);
    }
    for (int i = threadIdx.x; i < nr * Wout; i += THREADS) {
        const int r = i / Wout, x = i - r * Wout;
        const Taps t = taps_of(table, kmax, x, Win);
        const uint8_t* in = smem + (size_t)r * pitch + t.lo;
        int acc = 1 << (PRECISION_BITS - 1);
        for (int k = 0; k < t.n; ++k) acc += (int)in[k] * t.c[k];
        dst[(row0 + r) * Wout + x] = (uint8_t)clip8(acc);
    }
}

// VEC output bytes of one row: `in` is the first tap's row at the thread's column, rows W apart
template <int VEC>
__device__ __forceinline__ void resample_column(const uint8_t* in, const Taps t, int W, uint8_t* out) {
    int acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 1 << (PRECISION_BITS - 1);
    for (int k = 0; k < t.n; ++k) {
        const int c = t.c[k];
        if (VEC == 4) {
            const uint32_t w = *(const uint32_t*)(in + (long)k * W);
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] += (int)((w >> (8 * v)) & 255u) * c;
        } else {
            acc[0] += (int)in[(long)k * W] * c;
        }
    }
    if (VEC == 4) {
        uint32_t w = 0;
#pragma unroll
        for (int v = 0; v < VEC; ++v) w |= (uint32_t)clip8(acc[v]) << (8 * v);
        *(uint32_t*)out = w;
    } else {
        out[0] = (uint8_t)clip8(acc[0]);
    }
}

// grid (ceil(Hout * W / VEC / THREADS), planes); VEC = 4 needs W % 4 == 0 (then every row starts on a 32-bit word)
template <int VEC>
__global__ __launch_bounds__(THREADS) void lanczos_v(const uint8_t* __restrict__ src, const int* __restrict__ table, int kmax,
                                                     uint8_t* __restrict__ dst, int Hin, int Hout, int W) {
    const int Wv = W / VEC;
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= Hout * Wv) return;
    const int y = i / Wv, x = (i - y * Wv) * VEC;
    const Taps t = taps_of(table, kmax, y, Hin);
    resample_column<VEC>(src + ((long)blockIdx.y * Hin + t.lo) * W + x, t, W, dst + ((long)blockIdx.y * Hout + y) * W + x);
}

// The ragged intermediate [N][3][Hcap][W] -> the dense [N][3][Hout][W]; grid (.., N * 3).  Image n has Hin = H_n rows
// (the clamp of taps_of keeps every read below H_n: rows at or beyond it were never written) and the vertical table of its
// class out of tables [K][Hout][2 + kmax]; both are uniform over the workgroup.  An absent image (H_n = 0) has no taps:
// the accumulator's 1 << 21 clips to the zeros it is written as.
template <int VEC>
__global__ __launch_bounds__(THREADS) void lanczos_v_ragged(const uint8_t* __restrict__ src, const int* __restrict__ desc,
                                                            const int* __restrict__ tables, int K, int kmax,
                                                            uint8_t* __restrict__ dst, int Hcap, int Hout, int W) {
    const int Wv = W / VEC;
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= Hout * Wv) return;
    const int y = i / Wv, x = (i - y * Wv) * VEC;
    const int4 d = desc_of(desc, blockIdx.y / 3);
    const Taps t = taps_of(tables + (long)min(max(d.w, 0), K - 1) * Hout * (2 + kmax), kmax, y, min(max(d.y, 0), Hcap));
    resample_column<VEC>(src + ((long)blockIdx.y * Hcap + t.lo) * W + x, t, W, dst + ((long)blockIdx.y * Hout + y) * W + x);
}

// ---- ColorJitter ---------------------------------------------------------------------------------------------------
struct Jitter {
    int order[4];
    float factor[3];        // brightness, contrast, saturation
    int hue;                // trunc(h * 255) & 255
    bool apply;
};
__device__ __forceinline__ Jitter jitter_of(const int* __restrict__ params, const int* __restrict__ nonzero, int n) {
    const int* p = params + (long)n * PARAM_WORDS;
    Jitter j;
#pragma unroll
    for (int k = 0; k < 4; ++k) j.order[k] = p[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) j.factor[k] = __int_as_float(p[4 + k]);
    j.hue = p[7] & 255;
    j.apply = p[8] != 0 && (!nonzero || nonzero[n] != 0);
    return j;
}

// Pillow RGB -> L
__host__ __device__ __forceinline__ int gray_u8(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// PIL.Image.blend(degenerate, image, f): fp32, one rounding per operation, truncated, clipped
__host__ __device__ __forceinline__ int blend_u8(int deg, int x, float f) {
    const float d = (float)deg;
    const float diff = (float)x - d;
    const float prod = f * diff;
    const float t = truncf(d + prod);
    return (int)fminf(fmaxf(t, 0.f), 255.f);
}

// C round() of a non-negative value, clipped to 8 bits
__host__ __device__ __forceinline__ int round_u8(double x) { return (int)fmin(fmax(floor(x + 0.5), 0.0), 255.0); }

// Convert.c rgb2hsv, the 8-bit hue shift, hsv2rgb
__host__ __device__ __forceinline__ void hue_u8(int& r, int& g, int& b, int shift) {
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    int uh = 0, us = 0;
    if (maxc != minc) {
        const float cr = (float)(maxc - minc);
        const float s = cr / (float)maxc;
        const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
        float h;
        if (r == maxc) h = bc - gc;
        else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
        else h = (float)(4.0 + (double)gc - (double)rc);
        const double t = (double)h / 6.0 + 1.0;             // in [5/6, 11/6]: fmod(t, 1) = t - floor(t), exactly
        h = (float)(t - floor(t));
        uh = min(max((int)((double)h * 255.0), 0), 255);
        us = min(max((int)((double)s * 255.0), 0), 255);
    }
    const int v = maxc;
    uh = (uh + shift) & 255;
    if (us == 0) {
        r = g = b = v;
        return;
    }
    const double hf = (double)(float)uh * 6.0 / 255.0;
    const double fl = floor(hf);
    const double f = (double)(float)(hf - fl);
    const double fs = (double)(float)((double)(float)us / 255.0);
    const double vv = (double)v;
    const int p = round_u8(vv * (1.0 - fs));
    const int q = round_u8(vv * (1.0 - fs * f));
    const int t = round_u8(vv * (1.0 - fs * (1.0 - f)));
    switch ((int)fl % 6) {
    case 0: r = v, g = t, b = p; break;
    case 1: r = q, g = v, b = p; break;
    case 2: r = p, g = v, b = t; break;
    case 3: r = p, g = q, b = v; break;
    case 4: r = t, g = p, b = v; break;
    default: r = v, g = p, b = q; break;
    }
}

// operation 0 brightness, 1 contrast (needs the image's gray mean), 2 saturation, 3 hue
__host__ __device__ __forceinline__ void jitter_op(int op, const Jitter& j, int mean, int& r, int& g, int& b) {
    if (op == 0) {
        r = blend_u8(0, r, j.factor[0]), g = blend_u8(0, g, j.factor[0]), b = blend_u8(0, b, j.factor[0]);
    } else if (op == 1) {
        r = blend_u8(mean, r, j.factor[1]), g = blend_u8(mean, g, j.factor[1]), b = blend_u8(mean, b, j.factor[1]);
    } else if (op == 2) {
        const int l = gray_u8(r, g, b);
        r = blend_u8(l, r, j.factor[2]), g = blend_u8(l, g, j.factor[2]), b = blend_u8(l, b, j.factor[2]);
    } else if (op == 3) {
        hue_u8(r, g, b, j.hue);
    }
}

template <int VEC> struct Pixels {
    int r[VEC], g[VEC], b[VEC];
};
template <int VEC> __device__ __forceinline__ Pixels<VEC> load_pixels(const uint8_t* __restrict__ img, long HW, long i) {
    Pixels<VEC> p;
    if (VEC == 4) {
        const uint32_t wr = *(const uint32_t*)(img + i), wg = *(const uint32_t*)(img + HW + i),
                       wb = *(const uint32_t*)(img + 2 * HW + i);
#pragma unroll
        for (int v = 0; v < VEC; ++v)
            p.r[v] = (wr >> (8 * v)) & 255u, p.g[v] = (wg >> (8 * v)) & 255u, p.b[v] = (wb >> (8 * v)) & 255u;
    } else {
        p.r[0] = img[i], p.g[0] = img[HW + i], p.b[0] = img[2 * HW + i];
    }
    return p;
}
template <int VEC> __device__ __forceinline__ void store_unit(float* __restrict__ out, const int* c) {
    if (VEC == 4) {
        float4 f;
        f.x = (float)c[0] / 255.0f, f.y = (float)c[1] / 255.0f, f.z = (float)c[2] / 255.0f, f.w = (float)c[3] / 255.0f;
        *(float4*)out = f;
    } else {
        out[0] = (float)c[0] / 255.0f;
    }
}

__device__ __forceinline__ uint32_t wave_sum_u(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// grid (chunks, N); HW % VEC == 0.  partial [N][chunks]: sum of L over the chunk after the operations preceding contrast
template <int VEC>
__global__ __launch_bounds__(THREADS) void jitter_sum(const uint8_t* __restrict__ img, const int* __restrict__ params,
                                                      const int* __restrict__ nonzero, uint32_t* __restrict__ partial,
                                                      long HW) {
    const int n = blockIdx.y;
    const Jitter j = jitter_of(params, nonzero, n);
    if (!j.apply) return;                       // its partial sums are never read
    const uint8_t* im = img + (long)n * 3 * HW;
    const long base = (long)blockIdx.x * (THREADS * VEC * JITTER_ITERS);
    uint32_t sum = 0;
#pragma unroll
    for (int it = 0; it < JITTER_ITERS; ++it) {
        const long i = base + ((long)it * THREADS + threadIdx.x) * VEC;
        if (i >= HW) break;
        Pixels<VEC> p = load_pixels<VEC>(im, HW, i);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            for (int k = 0; k < 4 && j.order[k] != 1; ++k) jitter_op(j.order[k], j, 0, p.r[v], p.g[v], p.b[v]);
            sum += (uint32_t)gray_u8(p.r[v], p.g[v], p.b[v]);
        }
    }
    __shared__ uint32_t part[THREADS / WAVE];
    sum = wave_sum_u(sum);
    if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x / WAVE] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int k = 0; k < THREADS / WAVE; ++k) s += part[k];
        partial[(long)n * gridDim.x + blockIdx.x] = s;
    }
}

template <int VEC>
__global__ __launch_bounds__(THREADS) void jitter_out(const uint8_t* __restrict__ img, const int* __restrict__ params,
                                                      const int* __restrict__ nonzero, const uint32_t* __restrict__ partial,
                                                      float* __restrict__ color, float* __restrict__ color_aug, long HW) {
    const int n = blockIdx.y;
    const Jitter j = jitter_of(params, nonzero, n);
    __shared__ int mean_s;
    int mean = 0;
    if (j.apply) {                              // uniform over the workgroup
        if (threadIdx.x < WAVE) {
            uint32_t s = 0;
            for (int c = threadIdx.x; c < (int)gridDim.x; c += WAVE) s += partial[(long)n * gridDim.x + c];
            s = wave_sum_u(s);
            if (threadIdx.x == 0) mean_s = (int)floor((double)s / (double)HW + 0.5);      // int(mean(L) + 0.5)
        }
        __syncthreads();
        mean = mean_s;
    }
    const uint8_t* im = img + (long)n * 3 * HW;
    float* oc = color + (long)n * 3 * HW;
    float* oa = color_aug + (long)n * 3 * HW;
    const long base = (long)blockIdx.x * (THREADS * VEC * JITTER_ITERS);
#pragma unroll
    for (int it = 0; it < JITTER_ITERS; ++it) {
        const long i = base + ((long)it * THREADS + threadIdx.x) * VEC;
        if (i >= HW) break;
        Pixels<VEC> p = load_pixels<VEC>(im, HW, i);
        store_unit<VEC>(oc + i, p.r);
        store_unit<VEC>(oc + HW + i, p.g);
        store_unit<VEC>(oc + 2 * HW + i, p.b);
        if (j.apply) {
#pragma unroll
            for (int v = 0; v < VEC; ++v)
                for (int k = 0; k < 4; ++k) jitter_op(j.order[k], j, mean, p.r[v], p.g[v], p.b[v]);
        }
        store_unit<VEC>(oa + i, p.r);
        store_unit<VEC>(oa + HW + i, p.g);
        store_unit<VEC>(oa + 2 * HW + i, p.b);
    }
}

__global__ __launch_bounds__(THREADS) void repeat_rows(const float* __restrict__ src, float* __restrict__ dst, int reps,
                                                       int len, long total) {
    const long i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= total) return;
    const long row = i / ((long)reps * len);
    dst[i] = src[row * len + i % len];
}

inline long jitter_chunks(long HW, int vec) {
    const long chunk = (long)THREADS * vec * JITTER_ITERS;
    return (HW + chunk - 1) / chunk;
}
inline int jitter_vec(long HW) { return HW % 4 == 0 ? 4 : 1; }

// The horizontal pass of both entry points, their arguments checked: the pointer table, the memset of the marks, the
// staged row's pitch, the rows a workgroup takes, and the launch.
int launch_lanczos_h(const void* const* srcs, int nsrc, int items_per_src, int C, long pixel_stride, long row_stride,
                     long channel_stride, long item_stride, const int32_t* taps, int kmax, const int32_t* flip,
                     int32_t* nonzero, uint8_t* dst, int H, int Win, int Wout, void* stream) {
    if (nsrc > MAX_SRCS) return PPEA_ERR_UNSUPPORTED;
    const long images = (long)nsrc * items_per_src;
    if (images > 0x7fffffffL / C || images * C > 0x7fffffffL / H) return PPEA_ERR_ARG;
    Srcs s;
    for (int i = 0; i < MAX_SRCS; ++i) {
        s.p[i] = i < nsrc ? (const uint8_t*)srcs[i] : nullptr;
        if (i < nsrc && !s.p[i]) return PPEA_ERR_ARG;
    }
    const bool rgb = C == 3 && pixel_stride == 3 && channel_stride == 1;
    // a staged row: the window's bytes behind up to 15 bytes of misalignment, in whole chunks / Win bytes
    const long pitch = rgb ? ((long)Win * 3 + 2 * (VIEW_CHUNK - 1)) / VIEW_CHUNK * VIEW_CHUNK
                           : ((long)Win + VIEW_CHUNK - 1) / VIEW_CHUNK * VIEW_CHUNK;
    if (pitch > LDS_LIMIT - VIEW_META) return PPEA_ERR_UNSUPPORTED;      // not even one row can be staged
    hipStream_t st = (hipStream_t)stream;
    if (nonzero) {
        hipError_t e = hipMemsetAsync(nonzero, 0, (size_t)images * sizeof(int32_t), st);
        if (e != hipSuccess) return (int)e;
    }
    const long rows = images * H * (rgb ? 1 : C);
    int rpb = THREADS / Wout;
    rpb = rpb < 1 ? 1 : (rpb > MAX_RPB ? MAX_RPB : rpb);
    if (rpb > (LDS_LIMIT - VIEW_META) / pitch) rpb = (int)((LDS_LIMIT - VIEW_META) / pitch);
    const long blocks = (rows + rpb - 1) / rpb;
    if (blocks > 0x7fffffffL) return PPEA_ERR_UNSUPPORTED;
    const size_t lds = (size_t)rpb * pitch + VIEW_META;
    if (rgb)
        lanczos_h_view3<<<(unsigned)blocks, THREADS, lds, st>>>(s, items_per_src, row_stride, item_stride, taps, kmax, flip,
                                                               nonzero, dst, rows, H, Win, Wout, rpb, (int)pitch);
    else
        lanczos_h_view<<<(unsigned)blocks, THREADS, lds, st>>>(s, items_per_src, C, pixel_stride, row_stride, channel_stride,
                                                              item_stride, taps, kmax, flip, nonzero, dst, rows, H, Win,
                                                              Wout, rpb, (int)pitch);
    return launch_status();
}

}  // namespace

// srcs: HOST array of nsrc device pointers, each `planes_per_src` planes of [H][Win]; the planes of all sources are
// numbered through, `planes_per_item` consecutive planes form an image (flip / nonzero index) and every source holds
// whole images: the views of pixel stride 1, row stride Win, channel stride H * Win.
extern "C" int ppea_lanczos_h_u8(const void* const* srcs, int nsrc, long planes_per_src, const int32_t* taps, int kmax,
                                 const int32_t* flip, int planes_per_item, int32_t* nonzero, uint8_t* dst, int H, int Win,
                                 int Wout, void* stream) {
    if (!srcs || !taps || !dst) return PPEA_ERR_ARG;
    if (nsrc <= 0 || planes_per_src <= 0 || planes_per_item <= 0 || kmax <= 0 || H <= 0 || Win <= 0 || Wout <= 0)
        return PPEA_ERR_ARG;
    if (planes_per_src % planes_per_item != 0 || planes_per_src > 0x7fffffffL) return PPEA_ERR_ARG;
    const long plane = (long)H * Win;
    return launch_lanczos_h(srcs, nsrc, (int)(planes_per_src / planes_per_item), planes_per_item, 1, Win, plane,
                            planes_per_item * plane, taps, kmax, flip, nonzero, dst, H, Win, Wout, stream);
}

// The horizontal pass over views: image i of source k is C channels of [H][Win] pixels at
// srcs[k] + i * item_stride + c * channel_stride + y * row_stride + x * pixel_stride (bytes; the window's x offset is
// folded into srcs[k]).  The images of all sources are numbered through (flip / nonzero index); dst [images][C][H][Wout].
extern "C" int ppea_lanczos_h_view_u8(const void* const* srcs, int nsrc, int items_per_src, int C, long pixel_stride,
                                      long row_stride, long channel_stride, long item_stride, const int32_t* taps, int kmax,
                                      const int32_t* flip, int32_t* nonzero, uint8_t* dst, int H, int Win, int Wout,
                                      void* stream) {
    if (!srcs || !taps || !dst) return PPEA_ERR_ARG;
    if (nsrc <= 0 || items_per_src <= 0 || C <= 0 || kmax <= 0 || H <= 0 || Win <= 0 || Wout <= 0) return PPEA_ERR_ARG;
    if (pixel_stride <= 0 || row_stride <= 0 || channel_stride <= 0 || item_stride <= 0) return PPEA_ERR_ARG;
    const bool interleaved = channel_stride < pixel_stride;
    if (interleaved && (long)C * channel_stride > pixel_stride) return PPEA_ERR_ARG;        // channels run into the next pixel
    // bytes from a row's first to its last: the window must end before the next row begins
    const long row_bytes = (long)(Win - 1) * pixel_stride + (interleaved ? (long)(C - 1) * channel_stride : 0) + 1;
    if (row_bytes > row_stride) return PPEA_ERR_ARG;
    return launch_lanczos_h(srcs, nsrc, items_per_src, C, pixel_stride, row_stride, channel_stride, item_stride, taps, kmax,
                            flip, nonzero, dst, H, Win, Wout, stream);
}

extern "C" int ppea_lanczos_v_u8(const uint8_t* src, const int32_t* taps, int kmax, uint8_t* dst, long planes, int Hin,
                                 int Hout, int W, void* stream) {
    if (!src || !taps || !dst || planes <= 0 || kmax <= 0 || Hin <= 0 || Hout <= 0 || W <= 0) return PPEA_ERR_ARG;
    if (planes > 65535 || (long)Hout * W > 0x7fffffffL || (long)Hin * W > 0x7fffffffL) return PPEA_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = W % 4 == 0 && ((uintptr_t)src | (uintptr_t)dst) % 4 == 0;
    const long work = (long)Hout * (vec ? W / 4 : W);
    const dim3 grid((unsigned)((work + THREADS - 1) / THREADS), (unsigned)planes);
    if (vec) lanczos_v<4><<<grid, THREADS, 0, st>>>(src, taps, kmax, dst, Hin, Hout, W);
    else lanczos_v<1><<<grid, THREADS, 0, st>>>(src, taps, kmax, dst, Hin, Hout, W);
    return launch_status();
}

// ---- frames of different sizes (KITTI's recording days) through one launch pair --------------------------------------
// The descriptor as the host holds it, checked before anything is launched: every extent inside the buffer, every class
// below K, H and W both zero (absent) or both positive.  -> 0, with the row count and the widest image.
static int check_ragged(const int32_t* desc_host, int N, long buf_bytes, int K, int Hcap, long* rows, int* Wmax) {
    *rows = 0, *Wmax = 0;
    for (int n = 0; n < N; ++n) {
        const int32_t *d = desc_host + 4L * n, off = d[0], H = d[1], W = d[2], k = d[3];
        if (off < 0 || H < 0 || W < 0 || (H == 0) != (W == 0) || H > Hcap || k < 0 || k >= K) return PPEA_ERR_ARG;
        if ((long)off + (long)H * W * 3 > buf_bytes) return PPEA_ERR_ARG;
        *rows += H;
        *Wmax = W > *Wmax ? W : *Wmax;
    }
    return *rows > 0x7fffffffL ? PPEA_ERR_UNSUPPORTED : 0;
}

// buf: interleaved-RGB (HWC) frames back to back, buf_bytes < 2^31 long; desc_host / desc: the same int32 [N][4] = (byte
// offset, H, W, size class) on the host (checked here) and on the device (read by the kernel); prefix: device int32
// [N + 1], prefix[n] = rows of the images before n; taps: device int32 [K][Wout][2 + kmax]; dst [N][3][Hcap][Wout], rows
// at or beyond H_n not written.  flip / nonzero [N] as ppea_lanczos_h_view_u8's.  One memset and one launch.
extern "C" int ppea_lanczos_h_ragged_u8(const uint8_t* buf, long buf_bytes, const int32_t* desc_host, const int32_t* desc,
                                        const int32_t* prefix, int N, const int32_t* taps, int K, int kmax,
                                        const int32_t* flip, int32_t* nonzero, uint8_t* dst, int Hcap, int Wout,
                                        void* stream) {
    if (!buf || !desc_host || !desc || !prefix || !taps || !dst) return PPEA_ERR_ARG;
    if (buf_bytes <= 0 || N <= 0 || K <= 0 || kmax <= 0 || Hcap <= 0 || Wout <= 0) return PPEA_ERR_ARG;
    if (buf_bytes > 0x7fffffffL || (long)K * Wout * (2 + kmax) > 0x7fffffffL || (long)N * 3 * Hcap > 0x7fffffffL)
        return PPEA_ERR_UNSUPPORTED;
    long rows;
    int Wmax;
    const int err = check_ragged(desc_host, N, buf_bytes, K, Hcap, &rows, &Wmax);
    if (err != 0) return err;
    // a staged row, as launch_lanczos_h's, sized by the widest image
    const long pitch = ((long)Wmax * 3 + 2 * (VIEW_CHUNK - 1)) / VIEW_CHUNK * VIEW_CHUNK;
    if (pitch > LDS_LIMIT - RAGGED_META) return PPEA_ERR_UNSUPPORTED;       // not even one row can be staged
    hipStream_t st = (hipStream_t)stream;
    if (nonzero) {
        hipError_t e = hipMemsetAsync(nonzero, 0, (size_t)N * sizeof(int32_t), st);
        if (e != hipSuccess) return (int)e;
    }
    if (rows == 0) return 0;                    // every frame absent: the vertical pass writes the zeros
    int rpb = THREADS / Wout;
    rpb = rpb < 1 ? 1 : (rpb > MAX_RPB ? MAX_RPB : rpb);
    if (rpb > (LDS_LIMIT - RAGGED_META) / pitch) rpb = (int)((LDS_LIMIT - RAGGED_META) / pitch);
    const long blocks = (rows + rpb - 1) / rpb;
    const size_t lds = (size_t)rpb * pitch + RAGGED_META;
    lanczos_h_ragged3<<<(unsigned)blocks, THREADS, lds, st>>>(buf, buf_bytes, desc, prefix, N, taps, K, kmax, flip,
                                                             nonzero, dst, (int)rows, Hcap, Wout, rpb, (int)pitch);
    return launch_status();
}

// src: the intermediate [N][3][Hcap][W] of ppea_lanczos_h_ragged_u8; taps: device int32 [K][Hout][2 + kmax]; dst: the
// dense [N][3][Hout][W], an absent image written as zeros.  One launch.
extern "C" int ppea_lanczos_v_ragged_u8(const uint8_t* src, const int32_t* desc_host, const int32_t* desc, int N,
                                        const int32_t* taps, int K, int kmax, uint8_t* dst, int Hcap, int Hout, int W,
                                        void* stream) {
    if (!src || !desc_host || !desc || !taps || !dst) return PPEA_ERR_ARG;
    if (N <= 0 || K <= 0 || kmax <= 0 || Hcap <= 0 || Hout <= 0 || W <= 0) return PPEA_ERR_ARG;
    if ((long)N * 3 > 65535 || (long)Hout * W > 0x7fffffffL || (long)Hcap * W > 0x7fffffffL ||
        (long)K * Hout * (2 + kmax) > 0x7fffffffL)
        return PPEA_ERR_UNSUPPORTED;
    for (int n = 0; n < N; ++n) {
        const int32_t* d = desc_host + 4L * n;
        if (d[1] < 0 || d[1] > Hcap || d[3] < 0 || d[3] >= K) return PPEA_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const bool vec = W % 4 == 0 && ((uintptr_t)src | (uintptr_t)dst) % 4 == 0;
    const long work = (long)Hout * (vec ? W / 4 : W);
    const dim3 grid((unsigned)((work + THREADS - 1) / THREADS), (unsigned)(N * 3));
    if (vec) lanczos_v_ragged<4><<<grid, THREADS, 0, st>>>(src, desc, taps, K, kmax, dst, Hcap, Hout, W);
    else lanczos_v_ragged<1><<<grid, THREADS, 0, st>>>(src, desc, taps, K, kmax, dst, Hcap, Hout, W);
    return launch_status();
}

extern "C" long ppea_color_jitter_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return PPEA_ERR_ARG;
    return (long)N * jitter_chunks((long)H * W, 1) * (long)sizeof(uint32_t);      // the scalar path's chunk count: the larger
}

// img [N][3][H][W] uint8; params [N][10] int32; nonzero [N] int32 or NULL (0: the image is never jittered);
// color, color_aug [N][3][H][W] fp32.  Two launches for any N.
extern "C" int ppea_color_jitter_u8(const uint8_t* img, const int32_t* params, const int32_t* nonzero, void* workspace,
                                    float* color, float* color_aug, int N, int H, int W, void* stream) {
    if (!img || !params || !workspace || !color || !color_aug || N <= 0 || H <= 0 || W <= 0) return PPEA_ERR_ARG;
    const long HW = (long)H * W;
    if (N > 65535 || HW > 0xffffffffL / 255) return PPEA_ERR_UNSUPPORTED;      // the gray sum of an image fits 32 bits
    hipStream_t st = (hipStream_t)stream;
    const bool vec = jitter_vec(HW) == 4 && ((uintptr_t)img | (uintptr_t)color | (uintptr_t)color_aug) % 16 == 0;
    const dim3 grid((unsigned)jitter_chunks(HW, vec ? 4 : 1), (unsigned)N);
    uint32_t* partial = (uint32_t*)workspace;
    if (vec) {
        jitter_sum<4><<<grid, THREADS, 0, st>>>(img, params, nonzero, partial, HW);
        jitter_out<4><<<grid, THREADS, 0, st>>>(img, params, nonzero, partial, color, color_aug, HW);
    } else {
        jitter_sum<1><<<grid, THREADS, 0, st>>>(img, params, nonzero, partial, HW);
        jitter_out<1><<<grid, THREADS, 0, st>>>(img, params, nonzero, partial, color, color_aug, HW);
    }
    return launch_status();
}

// dst [rows][reps][len] = src [rows][len] repeated: the per-scale K / inv_K of a batch in one launch
extern "C" int ppea_repeat_rows_f32(const float* src, float* dst, int rows, int reps, int len, void* stream) {
    if (!src || !dst || rows <= 0 || reps <= 0 || len <= 0) return PPEA_ERR_ARG;
    const long total = (long)rows * reps * len;
    repeat_rows<<<(unsigned)((total + THREADS - 1) / THREADS), THREADS, 0, (hipStream_t)stream>>>(src, dst, reps, len, total);
    return launch_status();
}
