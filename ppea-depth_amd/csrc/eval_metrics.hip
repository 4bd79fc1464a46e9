// Depth-error protocol of Trainer.val on the device, gfx950 (trainer.py:780-843, evaluate_depth.py:35-54), and of
// Trainer.val_ddad (trainer.py:583-623) as MODE_DDAD: the depth 1 / disparity is what is resized (the reciprocals of the four
// source disparities are interpolated), the range test and the clamp end at 200 m, the whole map is scored.
//
// One scored batch = one memset + 7 launches, whatever B is; images sit on grid axis y, fixed 2048-pixel chunks of an image's
// crop rectangle ("region") on axis x:
//   gather      bilinear resize of the predicted disparity at every region pixel of the ragged ground truth, 1 / x, scale
//               factor, validity mask -> dense per-image workspaces (gt = 0 marks a masked-out pixel) + valid count
//   select x 4  exact order statistics by radix select on the fp32 bit pattern (positive floats order as unsigned integers),
//               8 bits per pass from the top; 4 selections per image (pred / gt x lower / upper middle element), histograms
//               in LDS with integer atomics, merged into global histograms with integer atomics.  No pass writes a
//               "state": every later kernel re-derives the chosen digits from the stored histograms (4 wave scans).
//   partial     medians -> ratio; per-pixel error terms in fp32 in numpy's operation order; 7 fp64 sums per chunk
//   final       fp64 sum over chunks, the 7 errors, ratio, count
// Every floating-point sum has a fixed association (thread-serial, xor butterfly, serial over waves / chunks) and the only
// atomics are integer adds, so two calls agree bit for bit, and an image's result does not depend on its batch.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int ITEMS = 8;
constexpr int CHUNK = THREADS * ITEMS;      // region pixels per workgroup
constexpr int NSEL = 4;                     // selection s: array (s >> 1: 0 pred, 1 gt), rank (s & 1: (n-1)/2, n/2)
constexpr int PASSES = 4;
constexpr int BINS = 256;
constexpr float MIN_DEPTH = 1e-3f;

enum { MODE_RANGE = 0, MODE_EIGEN = 1, MODE_CITYSCAPES = 2, MODE_DDAD = 3 };

// The range constants are a property of the mode, fixed at compile time: the kernels that read them are instantiated once
// for val's protocol and once for val_ddad's.
template <bool DDAD> struct Protocol { static constexpr float MAX_DEPTH = DDAD ? 200.f : 80.f; };

struct Region {
    long off;              // first ground-truth value of the image in the flat buffer
    int W;                 // ground-truth row length
    int Hr;                // height the prediction is resized to
    int y0, x0, rh, rw;    // scored rectangle in ground-truth coordinates
    long size;             // rh * rw, clamped to the workspace stride
};

// evaluate.evaluate_image's cropping: the same fp64 products and int32 truncation as numpy's.
__device__ Region region_of(const int64_t* __restrict__ table, int b, int mode, long gt_len, long stride) {
    Region r;
    r.off = table[b * 3];
    const long H = table[b * 3 + 1], W = table[b * 3 + 2];
    r.W = (int)W;
    r.Hr = (int)H;
    int y0 = 0, y1 = (int)H, x0 = 0, x1 = (int)W;
    if (mode == MODE_EIGEN) {
        y0 = (int)(0.40810811 * (double)H);
        y1 = (int)(0.99189189 * (double)H);
        x0 = (int)(0.03594771 * (double)W);
        x1 = (int)(0.96405229 * (double)W);
    } else if (mode == MODE_CITYSCAPES) {
        r.Hr = (int)rint((double)H * 0.75);          // Python's round(): half to even
        y0 = 256, y1 = r.Hr, x0 = 192, x1 = min(1856, (int)W);
    }
    r.y0 = y0, r.x0 = x0;
    r.rh = max(y1 - y0, 0), r.rw = max(x1 - x0, 0);
    r.size = (long)r.rh * r.rw;
    // a table row that does not fit the buffers it indexes scores nothing instead of reading or writing outside them
    if (H <= 0 || W <= 0 || H > 0x7fffffffL / W || r.off < 0 || r.off + H * W > gt_len || r.size > stride) r.size = 0;
    return r;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// F.interpolate(mode="bilinear", align_corners=False) source index and weights for one axis
__device__ __forceinline__ void source(float scale, int dst, int in, int& i0, int& step, float& l0, float& l1) {
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = min((int)s, in - 1);
    step = i0 < in - 1 ? 1 : 0;
    l1 = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
    l0 = 1.f - l1;
}

template <bool DDAD>
__global__ __launch_bounds__(THREADS) void eval_gather(const float* __restrict__ pred, const float* __restrict__ gt,
                                                       long gt_len, const int64_t* __restrict__ table,
                                                       float* __restrict__ pred_ws, float* __restrict__ gt_ws,
                                                       int* __restrict__ count, int h, int w, long stride, int mode,
                                                       float factor) {
    const int b = blockIdx.y;
    const Region r = region_of(table, b, mode, gt_len, stride);
    const long base = (long)blockIdx.x * CHUNK;
    if (base >= r.size) return;
    const float* p = pred + (long)b * h * w;
    const float sy = (float)h / (float)r.Hr, sx = (float)w / (float)r.W;
    int valid = 0;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long i = base + it * THREADS + threadIdx.x;
        if (i >= r.size) break;
        const int ry = (int)(i / r.rw), rx = (int)(i - (long)ry * r.rw);
        const int y = r.y0 + ry, x = r.x0 + rx;
        const float g = gt[r.off + (long)y * r.W + x];
        float d = 0.f, gv = 0.f;
        if (g > MIN_DEPTH && g < Protocol<DDAD>::MAX_DEPTH) {
            int yi, yp, xi, xp;
            float ly0, ly1, lx0, lx1;
            source(sy, y, h, yi, yp, ly0, ly1);
            source(sx, x, w, xi, xp, lx0, lx1);
            const float* row0 = p + (long)yi * w;
            const float* row1 = row0 + (long)yp * w;
            float a = row0[xi], c = row0[xi + xp], e = row1[xi], f = row1[xi + xp];
            if (DDAD) a = 1.f / a, c = 1.f / c, e = 1.f / e, f = 1.f / f;      // val_ddad resizes the depth
            const float v = ly0 * (lx0 * a + lx1 * c) + ly1 * (lx0 * e + lx1 * f);
            d = (DDAD ? v : 1.f / v) * factor;
            gv = g;
            ++valid;
        }
        pred_ws[(long)b * stride + i] = d;
        gt_ws[(long)b * stride + i] = gv;
    }
    __shared__ int part[THREADS / WAVE];
    valid = wave_sum_i(valid);
    if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x / WAVE] = valid;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int k = 0; k < THREADS / WAVE; ++k) s += part[k];
        if (s) atomicAdd(count + b, s);
    }
}

// Wave s of the workgroup follows selection s through the first `npass` stored histograms of image b:
// prefix[s] = the npass * 8 leading bits of the s-th order statistic.  Needs THREADS == NSEL * WAVE.
__device__ void resolve(const int* __restrict__ hist, int B, int b, int n, int npass, uint32_t* prefix) {
    const int s = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    // an odd count has one middle element: only the even selections were histogrammed
    const int src = (n & 1) ? (s & ~1) : s;
    int k = (s & 1) ? n / 2 : (n - 1) / 2;
    uint32_t pre = 0;
    for (int p = 0; p < npass; ++p) {
        const int* hp = hist + (((long)p * B + b) * NSEL + src) * BINS + lane * 4;
        const int c0 = hp[0], c1 = hp[1], c2 = hp[2], c3 = hp[3];
        const int local = c0 + c1 + c2 + c3;
        int incl = local;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const int t = __shfl_up(incl, o, WAVE);
            if (lane >= o) incl += t;
        }
        const int excl = incl - local;
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
        const int from = who ? __ffsll((long long)who) - 1 : 0;      // no owner (empty image): digit 0, nothing selected
        digit = __shfl(digit, from, WAVE);
        k = __shfl(rest, from, WAVE);
        pre = (pre << 8) | (uint32_t)digit;
    }
    if (lane == 0) prefix[s] = pre;
}

__global__ __launch_bounds__(THREADS) void eval_select_pass(const float* __restrict__ pred_ws,
                                                            const float* __restrict__ gt_ws,
                                                            const int64_t* __restrict__ table,
                                                            const int* __restrict__ count, int* __restrict__ hist,
                                                            long gt_len, long stride, int mode, int B, int pass) {
    const int b = blockIdx.y;
    const Region r = region_of(table, b, mode, gt_len, stride);
    const long base = (long)blockIdx.x * CHUNK;
    const int n = count[b];
    if (base >= r.size || n == 0) return;
    __shared__ uint32_t prefix[NSEL];
    __shared__ int lh[NSEL][BINS];
    for (int i = threadIdx.x; i < NSEL * BINS; i += THREADS) (&lh[0][0])[i] = 0;
    resolve(hist, B, b, n, pass, prefix);
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const bool both = (n & 1) == 0;
    const uint32_t p0 = prefix[0], p1 = prefix[1], p2 = prefix[2], p3 = prefix[3];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long i = base + it * THREADS + threadIdx.x;
        if (i >= r.size) break;
        const uint32_t g = __float_as_uint(gt_ws[(long)b * stride + i]);
        if (g == 0) continue;
        const uint32_t d = __float_as_uint(pred_ws[(long)b * stride + i]);
        // the leading bits already fixed (none in pass 0); a shift by 32 is not defined, so it is two shifts
        const uint32_t dh = pass ? (d >> shift) >> 8 : 0, gh = pass ? (g >> shift) >> 8 : 0;
        const int dd = (d >> shift) & 255, gd = (g >> shift) & 255;
        if (dh == p0) atomicAdd(&lh[0][dd], 1);
        if (both && dh == p1) atomicAdd(&lh[1][dd], 1);
        if (gh == p2) atomicAdd(&lh[2][gd], 1);
        if (both && gh == p3) atomicAdd(&lh[3][gd], 1);
    }
    __syncthreads();
    int* out = hist + ((long)pass * B + b) * NSEL * BINS;
    for (int i = threadIdx.x; i < NSEL * BINS; i += THREADS) {
        const int c = (&lh[0][0])[i];
        if (c) atomicAdd(out + i, c);
    }
}

// np.median of the valid values: the middle element, or (a + b) / 2 in fp32
__device__ __forceinline__ float median_of(uint32_t lo, uint32_t hi) {
    return (__uint_as_float(lo) + __uint_as_float(hi)) / 2.f;
}

// fp32 logarithm as numpy's: the fp64 logarithm rounded once
__device__ __forceinline__ float log_f32(float x) { return (float)log((double)x); }

constexpr int NSUM = 7;      // abs_rel, sq_rel, squared error, squared log error, thresh < 1.25, < 1.25^2, < 1.25^3

template <bool DDAD>
__global__ __launch_bounds__(THREADS) void eval_errors_partial(const float* __restrict__ pred_ws,
                                                               const float* __restrict__ gt_ws,
                                                               const int64_t* __restrict__ table,
                                                               const int* __restrict__ count,
                                                               const int* __restrict__ hist, double* __restrict__ partial,
                                                               long gt_len, long stride, int mode, int B,
                                                               int median_scaling) {
    const int b = blockIdx.y;
    const Region r = region_of(table, b, mode, gt_len, stride);
    const long base = (long)blockIdx.x * CHUNK;
    const int n = count[b];
    double* out = partial + ((long)b * gridDim.x + blockIdx.x) * NSUM;
    __shared__ uint32_t prefix[NSEL];
    __shared__ double ws[THREADS / WAVE][NSUM];
    double acc[NSUM];
#pragma unroll
    for (int k = 0; k < NSUM; ++k) acc[k] = 0.0;
    if (base < r.size && n > 0) {                   // uniform over the workgroup
        resolve(hist, B, b, n, PASSES, prefix);
        __syncthreads();
        const float ratio = median_of(prefix[2], prefix[3]) / median_of(prefix[0], prefix[1]);
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            const long i = base + it * THREADS + threadIdx.x;
            if (i >= r.size) break;
            const float g = gt_ws[(long)b * stride + i];
            if (g == 0.f) continue;
            float p = pred_ws[(long)b * stride + i];
            if (median_scaling) p = p * ratio;
            p = p < MIN_DEPTH ? MIN_DEPTH : p;
            p = p > Protocol<DDAD>::MAX_DEPTH ? Protocol<DDAD>::MAX_DEPTH : p;
            const float th = fmaxf(g / p, p / g);
            const float d = g - p, sq = d * d;
            const float l = log_f32(g) - log_f32(p);
            acc[0] += (double)(fabsf(d) / g);
            acc[1] += (double)(sq / g);
            acc[2] += (double)sq;
            acc[3] += (double)(l * l);
            acc[4] += th < 1.25f ? 1.0 : 0.0;
            acc[5] += th < 1.5625f ? 1.0 : 0.0;
            acc[6] += th < 1.953125f ? 1.0 : 0.0;
        }
    }
#pragma unroll
    for (int k = 0; k < NSUM; ++k) acc[k] = wave_sum_d(acc[k]);
    if ((threadIdx.x & (WAVE - 1)) == 0)
        for (int k = 0; k < NSUM; ++k) ws[threadIdx.x / WAVE][k] = acc[k];
    __syncthreads();
    if (threadIdx.x < NSUM) {
        double s = 0.0;
        for (int v = 0; v < THREADS / WAVE; ++v) s += ws[v][threadIdx.x];
        out[threadIdx.x] = s;
    }
}

__global__ __launch_bounds__(THREADS) void eval_errors_final(const double* __restrict__ partial,
                                                             const int* __restrict__ count, const int* __restrict__ hist,
                                                             double* __restrict__ errors, float* __restrict__ ratio,
                                                             int32_t* __restrict__ count_out, int chunks, int B) {
    const int b = blockIdx.x;
    const int n = count[b];
    __shared__ uint32_t prefix[NSEL];
    __shared__ double ws[THREADS / WAVE][NSUM];
    resolve(hist, B, b, n, PASSES, prefix);
    double acc[NSUM];
#pragma unroll
    for (int k = 0; k < NSUM; ++k) acc[k] = 0.0;
    for (int c = threadIdx.x; c < chunks; c += THREADS) {
        const double* p = partial + ((long)b * chunks + c) * NSUM;
#pragma unroll
        for (int k = 0; k < NSUM; ++k) acc[k] += p[k];
    }
#pragma unroll
    for (int k = 0; k < NSUM; ++k) acc[k] = wave_sum_d(acc[k]);
    if ((threadIdx.x & (WAVE - 1)) == 0)
        for (int k = 0; k < NSUM; ++k) ws[threadIdx.x / WAVE][k] = acc[k];
    __syncthreads();
    if (threadIdx.x < NSUM) {
        double s = 0.0;
        for (int v = 0; v < THREADS / WAVE; ++v) s += ws[v][threadIdx.x];
        s = s / (double)n;                           // n = 0: 0 / 0 = NaN, as the host path's empty means
        const int k = threadIdx.x;
        errors[(long)b * NSUM + k] = (k == 2 || k == 3) ? sqrt(s) : s;
    }
    if (threadIdx.x == 0) {
        ratio[b] = n > 0 ? median_of(prefix[2], prefix[3]) / median_of(prefix[0], prefix[1]) : __uint_as_float(0x7fc00000u);
        count_out[b] = n;
    }
}

// mean of the per-image errors over the split: one lane per error, serial over the images
__global__ void eval_errors_mean(const double* __restrict__ errors, double* __restrict__ mean, int n) {
    const int k = threadIdx.x;
    if (k >= NSUM) return;
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += errors[(long)i * NSUM + k];
    mean[k] = s / (double)n;
}

inline long align_up(long v, long a) { return (v + a - 1) / a * a; }
inline long chunks_of(long stride) { return (stride + CHUNK - 1) / CHUNK; }

struct Workspace {
    long partial, pred, gt, ints, bytes;     // byte offsets; ints = [PASSES][B][NSEL][BINS] histograms, then [B] counts
    long int_bytes;
};
inline Workspace layout(int B, long stride) {
    Workspace w;
    w.partial = 0;
    w.pred = align_up((long)B * chunks_of(stride) * NSUM * 8, 256);
    w.gt = w.pred + align_up((long)B * stride * 4, 256);
    w.ints = w.gt + align_up((long)B * stride * 4, 256);
    w.int_bytes = ((long)PASSES * B * NSEL * BINS + B) * 4;
    w.bytes = w.ints + align_up(w.int_bytes, 256);
    return w;
}

}  // namespace

static_assert(THREADS == NSEL * WAVE, "one wave per selection");

extern "C" long ppea_depth_errors_workspace_bytes(int B, long max_region) {
    if (B <= 0 || max_region < 0) return PPEA_ERR_ARG;
    return layout(B, max_region > 0 ? max_region : 1).bytes;
}

extern "C" int ppea_depth_errors_f32(const float* pred_disp, const float* gt, long gt_len, const int64_t* table,
                                     void* workspace, double* errors, float* ratio, int32_t* count, int B, int h, int w,
                                     long max_region, int mode, int median_scaling, float scale, void* stream) {
    if (!pred_disp || !gt || !table || !workspace || !errors || !ratio || !count) return PPEA_ERR_ARG;
    if (B <= 0 || B > 65535 || h <= 0 || w <= 0 || gt_len <= 0 || max_region < 0) return PPEA_ERR_ARG;
    if (mode < MODE_RANGE || mode > MODE_DDAD) return PPEA_ERR_UNSUPPORTED;
    const long stride = max_region > 0 ? max_region : 1;
    if (chunks_of(stride) > 0x7fffffffL) return PPEA_ERR_UNSUPPORTED;
    const Workspace L = layout(B, stride);
    char* base = (char*)workspace;
    double* partial = (double*)(base + L.partial);
    float* pred_ws = (float*)(base + L.pred);
    float* gt_ws = (float*)(base + L.gt);
    int* hist = (int*)(base + L.ints);
    int* cnt = hist + (long)PASSES * B * NSEL * BINS;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(hist, 0, L.int_bytes, st);
    if (e != hipSuccess) return (int)e;
    const int chunks = (int)chunks_of(stride);
    const dim3 grid(chunks, B);
    const bool ddad = mode == MODE_DDAD;
    if (ddad)
        eval_gather<true><<<grid, THREADS, 0, st>>>(pred_disp, gt, gt_len, table, pred_ws, gt_ws, cnt, h, w, stride, mode,
                                                    scale);
    else
        eval_gather<false><<<grid, THREADS, 0, st>>>(pred_disp, gt, gt_len, table, pred_ws, gt_ws, cnt, h, w, stride, mode,
                                                     scale);
    for (int pass = 0; pass < PASSES; ++pass)
        eval_select_pass<<<grid, THREADS, 0, st>>>(pred_ws, gt_ws, table, cnt, hist, gt_len, stride, mode, B, pass);
    if (ddad)
        eval_errors_partial<true><<<grid, THREADS, 0, st>>>(pred_ws, gt_ws, table, cnt, hist, partial, gt_len, stride, mode, B,
                                                            median_scaling);
    else
        eval_errors_partial<false><<<grid, THREADS, 0, st>>>(pred_ws, gt_ws, table, cnt, hist, partial, gt_len, stride, mode, B,
                                                             median_scaling);
    eval_errors_final<<<B, THREADS, 0, st>>>(partial, cnt, hist, errors, ratio, count, chunks, B);
    return launch_status();
}

extern "C" int ppea_depth_errors_mean_f64(const double* errors, double* mean, int n, void* stream) {
    if (!errors || !mean || n <= 0) return PPEA_ERR_ARG;
    eval_errors_mean<<<1, WAVE, 0, (hipStream_t)stream>>>(errors, mean, n);
    return launch_status();
}
