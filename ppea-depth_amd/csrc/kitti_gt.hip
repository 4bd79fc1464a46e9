// KITTI ground truth from raw LiDAR on the device, gfx950: kitti_utils.generate_depth_map (kitti_utils.py:50-102) for a ragged
// batch of velodyne scans, written straight into the flat fp32 layout DeviceGroundTruth / ppea_depth_errors_f32 read.
//
// What the reference does per scan, and what is kept of it (README, "KITTI ground truth"):
//   q = P . (x, y, z, 1) in fp64, u = rint(q0 / q2) - 1, v = rint(q1 / q2) - 1 (half to even), depth = q2 or the point's own
//   fp32 x (vel_depth); points with x < 0 are dropped, q2 < 0 is NOT; a point is valid when 0 <= u < W and 0 <= v < H (NaN
//   fails every comparison);
//   (a) depth[v,u] = z by fancy assignment: the LAST valid point in scan order on a pixel wins;
//   (b) per key = v * (W - 1) + u - 1 (sub2ind; not a bijection: (v, W-1) and (v+1, 0) share a key; key -1 is pixel (0,0)) held
//       by more than one valid point, the pixel of the FIRST such point gets the MINIMUM z over all points of the key;
//   (c) depth < 0 -> 0.
// A pixel's points all carry the pixel's own key, so (b) reaches a pixel only through that one key: the resolve pass needs one
// key lookup per pixel.
//
// One call = one memset + 2 launches per group of GROUP scans.  Nothing depends on the order in which atomics land: every
// atomic is an integer max over a word whose order is the wanted order (scan order in the high bits, complemented where the
// minimum is wanted, so that the cleared word 0 means "no point"), and the resolve pass is a pure function of those words.
//   scatter   one point per lane: projection in fp64, then four no-return integer atomics (per pixel: last; per key: first,
//             highest order, minimum z)
//   resolve   one pixel per lane: (a)-(c) from the words, one plain fp32 store per pixel (every pixel is written)
// The fp32 cast is monotone, so the minimum over cast values is the cast of the reference's fp64 minimum.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int GROUP = 32;          // scans per launch: their descriptors travel as kernel arguments (GROUP * 40 B)

struct Scan {
    long pt0;      // first point of the scan in `points`
    long ws0;      // first pixel of the image in the workspace arrays
    long out0;     // first pixel of the image in out_flat (the table's offset)
    int n;         // points in the scan
    int H, W;
    int b;         // index of the scan in the batch (its P)
};
struct Scans { Scan s[GROUP]; };

// fp32 bits -> unsigned word with the same order as the floats (-inf lowest); NaN never arrives here
__device__ __forceinline__ uint32_t ordered_bits(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float from_ordered_bits(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

__global__ __launch_bounds__(THREADS) void velodyne_scatter(const float4* __restrict__ points, const double* __restrict__ P,
                                                            Scans scans, int vel_depth,
                                                            unsigned long long* __restrict__ last,
                                                            unsigned long long* __restrict__ first_c,
                                                            uint32_t* __restrict__ top_order, uint32_t* __restrict__ min_c) {
    const Scan sc = scans.s[blockIdx.y];
    const long i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= sc.n) return;
    const float4 p = points[sc.pt0 + i];
    if (!(p.x >= 0.f)) return;                                   // velo[:, 0] >= 0: -0.0 passes, NaN does not
    const double* m = P + (long)sc.b * 12;
    const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
    double q[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) q[r] = fma(m[r * 4 + 2], z, fma(m[r * 4 + 1], y, m[r * 4] * x)) + m[r * 4 + 3];
    const double u = rint(q[0] / q[2]) - 1.0, v = rint(q[1] / q[2]) - 1.0;
    if (!(u >= 0.0 && v >= 0.0 && u < (double)sc.W && v < (double)sc.H)) return;
    const int ui = (int)u, vi = (int)v;
    const float depth = vel_depth ? p.x : (float)q[2];
    const uint32_t order = (uint32_t)i;                          // n <= 2^31 - 2: order + 1 fits
    const uint32_t pix = (uint32_t)vi * (uint32_t)sc.W + (uint32_t)ui;
    const long key = (long)vi * (sc.W - 1) + ui;                 // sub2ind + 1: 0 .. H * (W - 1) <= H * W - 1
    atomicMax(last + sc.ws0 + pix, ((unsigned long long)(order + 1u) << 32) | __float_as_uint(depth));
    atomicMax(first_c + sc.ws0 + key, ~(((unsigned long long)order << 32) | pix));
    atomicMax(top_order + sc.ws0 + key, order + 1u);
    atomicMax(min_c + sc.ws0 + key, ~ordered_bits(depth));
}

__global__ __launch_bounds__(THREADS) void velodyne_resolve(Scans scans, const unsigned long long* __restrict__ last,
                                                            const unsigned long long* __restrict__ first_c,
                                                            const uint32_t* __restrict__ top_order,
                                                            const uint32_t* __restrict__ min_c, float* __restrict__ out) {
    const Scan sc = scans.s[blockIdx.y];
    const long pix = (long)blockIdx.x * THREADS + threadIdx.x;
    if (pix >= (long)sc.H * sc.W) return;
    float depth = 0.f;
    const unsigned long long l = last[sc.ws0 + pix];
    if (l) {                                                     // the pixel was hit: its key holds at least its own points
        depth = __uint_as_float((uint32_t)l);
        const int vi = (int)(pix / sc.W), ui = (int)(pix - (long)vi * sc.W);
        const long key = (long)vi * (sc.W - 1) + ui;
        const unsigned long long f = ~first_c[sc.ws0 + key];
        const bool mine = (uint32_t)f == (uint32_t)pix;          // the key's first point landed here
        const bool dup = top_order[sc.ws0 + key] != (uint32_t)(f >> 32) + 1u;      // first != last: more than one point
        if (mine && dup) depth = from_ordered_bits(~min_c[sc.ws0 + key]);
        if (depth < 0.f) depth = 0.f;
    }
    out[sc.out0 + pix] = depth;
}

inline long align_up(long v, long a) { return (v + a - 1) / a * a; }

struct Workspace { long last, first, top, min, bytes; };        // byte offsets
inline Workspace layout(long pixels) {
    Workspace w;
    w.last = 0;
    w.first = w.last + align_up(pixels * 8, 256);
    w.top = w.first + align_up(pixels * 8, 256);
    w.min = w.top + align_up(pixels * 4, 256);
    w.bytes = w.min + align_up(pixels * 4, 256);
    return w;
}

}  // namespace

extern "C" long ppea_velodyne_depth_workspace_bytes(long total_pixels) {
    if (total_pixels < 0 || total_pixels > 0x7fffffffffffL) return PPEA_ERR_ARG;
    return layout(total_pixels).bytes;
}

extern "C" int ppea_velodyne_depth_f32(const float* points, const int64_t* point_offsets, int B, const double* P,
                                       const int64_t* table, int vel_depth, float* out_flat, void* workspace, void* stream) {
    if (!point_offsets || !P || !table || B <= 0) return PPEA_ERR_ARG;
    if (point_offsets[0] < 0) return PPEA_ERR_ARG;
    long pixels = 0;
    for (int b = 0; b < B; ++b) {
        const long n = point_offsets[b + 1] - point_offsets[b];
        const long off = table[b * 3], H = table[b * 3 + 1], W = table[b * 3 + 2];
        if (n < 0 || off < 0 || H < 0 || W < 0) return PPEA_ERR_ARG;
        if (n > 0x7ffffffeL || (W > 0 && H > 0x7fffffffL / W)) return PPEA_ERR_UNSUPPORTED;
        pixels += H * W;
    }
    if (pixels == 0) return 0;                                   // nothing to write
    if (!out_flat || !workspace || (point_offsets[B] > 0 && !points)) return PPEA_ERR_ARG;
    const Workspace L = layout(pixels);
    char* base = (char*)workspace;
    unsigned long long* last = (unsigned long long*)(base + L.last);
    unsigned long long* first_c = (unsigned long long*)(base + L.first);
    uint32_t* top_order = (uint32_t*)(base + L.top);
    uint32_t* min_c = (uint32_t*)(base + L.min);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(workspace, 0, L.bytes, st);
    if (e != hipSuccess) return (int)e;
    long ws0 = 0;
    for (int b0 = 0; b0 < B; b0 += GROUP) {
        Scans scans = {};
        int g = 0;
        long max_n = 0, max_pix = 0;
        for (int b = b0; b < B && b < b0 + GROUP; ++b) {
            const long H = table[b * 3 + 1], W = table[b * 3 + 2];
            if (H * W == 0) continue;                            // no pixel: the scan has nowhere to land
            Scan& s = scans.s[g++];
            s.pt0 = point_offsets[b];
            s.n = (int)(point_offsets[b + 1] - point_offsets[b]);
            s.ws0 = ws0;
            s.out0 = table[b * 3];
            s.H = (int)H, s.W = (int)W, s.b = b;
            ws0 += H * W;
            max_n = s.n > max_n ? s.n : max_n;
            max_pix = H * W > max_pix ? H * W : max_pix;
        }
        if (g == 0) continue;
        if (max_n > 0)
            velodyne_scatter<<<dim3((unsigned)((max_n + THREADS - 1) / THREADS), g), THREADS, 0, st>>>(
                (const float4*)points, P, scans, vel_depth, last, first_c, top_order, min_c);
        velodyne_resolve<<<dim3((unsigned)((max_pix + THREADS - 1) / THREADS), g), THREADS, 0, st>>>(scans, last, first_c,
                                                                                                    top_order, min_c, out_flat);
    }
    return launch_status();
}
