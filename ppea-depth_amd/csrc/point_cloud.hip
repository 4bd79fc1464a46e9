// Point clouds, gfx950: 3D points from a predicted plane -- the export's depth at the frame's own size, back-projected
// through the frame's inverse intrinsics (layers.BackprojectDepth: integer pixel coordinates), moved by a camera-to-world
// matrix, with the frame's colour -- and the pose chain that supplies that matrix to a stream.
//
// The number of points depends on the data (range test, depth-edge test), the order does not: image order, raster order of
// (v, u) inside an image.  Three launches on the caller's stream, none of which waits for another workgroup:
//   mark     grid (chunks, B): a workgroup decides PC_CHUNK candidates (pixels with u % stride == v % stride == 0, in raster
//            order), a wave's 64 decisions are one __ballot word; the words and the chunk's count go to the workspace
//   scan     ONE workgroup: exclusive scan of the B * chunks counts (int64), the per-image counts, the cursor
//   scatter  grid (chunks, B): a kept candidate's rank = chunk offset + prefix of its chunk's words (LDS) + popcount of the
//            lower lanes of its word; the depth is computed again (same code, same bits) and the point is written if it fits
// A single-pass scan (decoupled look-back) would save two launches and make workgroups wait on flags of others; three
// launches cost microseconds and cannot hang.  No float atomics, no integer atomics either.
//   pose_accumulate  world = world @ pose[:, 0] where present, identity elsewhere: 1 launch
#include "common.h"
#include "export_sample.h"

namespace {

using export_sample::Target;
using export_sample::target_of;
using export_sample::sample_yx;
using export_sample::depth_of;

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / WAVE;
constexpr int PC_CHUNK = 2048;                   // candidates of one image per workgroup
constexpr int ITERS = PC_CHUNK / THREADS;
constexpr int WORDS = PC_CHUNK / WAVE;           // ballot words per chunk; word = it * WAVES + wave
constexpr int SCAN_THREADS = 1024;
constexpr long NO_LIMIT = 0x7fffffffffffffffL;

// Upper bound of the candidates of an image of at most P pixels: ceil(H / s) ceil(W / s) <= P / s^2 + (H + W) / s + 1 with
// H + W <= P + 1, and never more than P.
inline long max_candidates(long P, long s) {
    const long bound = P / (s * s) + (P + 1) / s + 2;
    return bound < P ? bound : P;
}
inline long chunks_of(long max_pixels, int stride) {
    return (max_candidates(max_pixels, stride) + PC_CHUNK - 1) / PC_CHUNK;
}

// Workspace: start (the cursor at entry, clamped), offs [n + 1] int64 (exclusive scan of the chunk counts, the total last),
// bits [n][WORDS] uint64, count [n] int32; n = B * chunks, chunk c of image b at b * chunks + c.
struct Workspace {
    int64_t* start;
    int64_t* offs;
    unsigned long long* bits;
    int32_t* count;
};
inline Workspace carve(void* ws, long n) {
    Workspace k;
    k.start = (int64_t*)ws;
    k.offs = k.start + 1;
    k.bits = (unsigned long long*)(k.offs + n + 1);
    k.count = (int32_t*)(k.bits + n * WORDS);
    return k;
}
inline long workspace_bytes(long n) { return 8 + 8 * (n + 1) + 8 * n * WORDS + 4 * n; }

// Candidates of a target: every stride-th row and column
struct Lattice {
    int Wc;                // candidate columns
    long n;                // candidates
};
__device__ __forceinline__ Lattice lattice_of(const Target& t, int stride) {
    Lattice l;
    if (t.size == 0) {
        l.Wc = 1, l.n = 0;
        return l;
    }
    l.Wc = (t.W - 1) / stride + 1;
    l.n = (long)((t.H - 1) / stride + 1) * l.Wc;
    return l;
}

template <bool RECIP>
struct Plane {
    const float* p;
    int h, w;
    double sy, sx;
    float sc;
    __device__ __forceinline__ float depth(const Target& t, int v, int u) const {
        return depth_of<RECIP>(sc, sample_yx<RECIP>(p, h, w, t, sy, sx, v, u));
    }
};
template <bool RECIP>
__device__ __forceinline__ Plane<RECIP> plane_of(const float* pred, const float* scale, int b, int h, int w,
                                                 const Target& t) {
    Plane<RECIP> pl;
    pl.p = pred + (long)b * h * w;
    pl.h = h, pl.w = w;
    pl.sy = (double)h / (double)t.H, pl.sx = (double)w / (double)t.W;
    pl.sc = scale[b];
    return pl;
}

template <bool RECIP>
__global__ __launch_bounds__(THREADS) void mark(const float* __restrict__ pred, const float* __restrict__ scale,
                                                const int64_t* __restrict__ table, int h, int w, float lo, float hi,
                                                int stride, float edge, unsigned long long* __restrict__ bits,
                                                int32_t* __restrict__ count) {
    const int b = blockIdx.y;
    const long slot = (long)b * gridDim.x + blockIdx.x;
    const Target t = target_of(table, b, NO_LIMIT);
    const Lattice lat = lattice_of(t, stride);
    const long base = (long)blockIdx.x * PC_CHUNK;
    if (base >= lat.n) {                                         // uniform
        if (threadIdx.x == 0) count[slot] = 0;
        return;
    }
    const Plane<RECIP> pl = plane_of<RECIP>(pred, scale, b, h, w, t);
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    __shared__ int wave_count[WAVES];
    int kept = 0;                                                // of this wave (the same in all its lanes)
#pragma unroll 1
    for (int it = 0; it < ITERS; ++it) {
        const long j = base + it * THREADS + threadIdx.x;
        bool keep = false;
        if (j < lat.n) {
            const int vq = (int)(j / lat.Wc), uq = (int)(j - (long)vq * lat.Wc);
            const int v = vq * stride, u = uq * stride;
            const float d = pl.depth(t, v, u);
            keep = d > lo && d < hi;                             // a NaN fails
            if (keep && edge > 0.f) {
                const float tol = edge * d;
                // a NaN neighbour compares false and does not drop the pixel
                if (u > 0 && fabsf(pl.depth(t, v, u - 1) - d) > tol) keep = false;
                if (u < t.W - 1 && fabsf(pl.depth(t, v, u + 1) - d) > tol) keep = false;
                if (v > 0 && fabsf(pl.depth(t, v - 1, u) - d) > tol) keep = false;
                if (v < t.H - 1 && fabsf(pl.depth(t, v + 1, u) - d) > tol) keep = false;
            }
        }
        const unsigned long long word = __ballot(keep);
        if (lane == 0) bits[slot * WORDS + it * WAVES + wave] = word;
        kept += __popcll(word);
    }
    if (lane == 0) wave_count[wave] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
#pragma unroll
        for (int k = 0; k < WAVES; ++k) c += wave_count[k];
        count[slot] = c;
    }
}

// One workgroup: offs = exclusive scan of count [n], offs[n] = total; counts[b] = the image's kept pixels; the cursor.
__global__ __launch_bounds__(SCAN_THREADS) void scan(const int32_t* __restrict__ count, int64_t* __restrict__ offs,
                                                     int64_t* __restrict__ start_out, long n, int B, long chunks,
                                                     long capacity, int64_t* __restrict__ cursor,
                                                     int64_t* __restrict__ counts) {
    constexpr int NW = SCAN_THREADS / WAVE;
    __shared__ long wave_total[NW];
    __shared__ long carry;
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (long tile = 0; tile < n; tile += SCAN_THREADS) {
        const long i = tile + threadIdx.x;
        const long mine = i < n ? (long)count[i] : 0;
        long incl = mine;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const long up = __shfl_up(incl, o, WAVE);
            if (lane >= o) incl += up;
        }
        if (lane == WAVE - 1) wave_total[wave] = incl;
        __syncthreads();
        long before = carry;
        for (int k = 0; k < wave; ++k) before += wave_total[k];
        if (i < n) offs[i] = before + incl - mine;
        __syncthreads();
        if (threadIdx.x == SCAN_THREADS - 1) carry = before + incl;
        __syncthreads();
    }
    const long total = carry;
    if (threadIdx.x == 0) offs[n] = total;
    __syncthreads();                                             // offs: written and read by this workgroup only
    for (int b = threadIdx.x; b < B; b += SCAN_THREADS) counts[b] = offs[(long)(b + 1) * chunks] - offs[(long)b * chunks];
    if (threadIdx.x == 0) {
        long start = cursor[0];
        start = start < 0 ? 0 : start > capacity ? capacity : start;
        const long room = capacity - start;
        const long fit = total < room ? total : room;
        start_out[0] = start;
        cursor[0] = start + fit;
        cursor[1] += total - fit;
    }
}

__device__ __forceinline__ uint8_t unit_byte(float c) {          // the inverse of ToTensor, valstore's rule
    const float r = rintf(c * 255.0f);
    return (uint8_t)(!(r >= 0.f) ? 0.f : r > 255.f ? 255.f : r);  // a NaN gives 0
}

template <bool RECIP>
__global__ __launch_bounds__(THREADS) void scatter(const float* __restrict__ pred, const float* __restrict__ scale,
                                                   const int64_t* __restrict__ table, int h, int w, int stride,
                                                   const float* __restrict__ inv_K, const float* __restrict__ cam_to_world,
                                                   const void* __restrict__ colour, const int64_t* __restrict__ colour_off,
                                                   int colour_mode, float* __restrict__ xyz, uint8_t* __restrict__ rgb,
                                                   int64_t* __restrict__ index, long capacity,
                                                   const unsigned long long* __restrict__ bits,
                                                   const int64_t* __restrict__ offs, const int64_t* __restrict__ start_in) {
    const int b = blockIdx.y;
    const long slot = (long)b * gridDim.x + blockIdx.x;
    const Target t = target_of(table, b, NO_LIMIT);
    const Lattice lat = lattice_of(t, stride);
    const long base = (long)blockIdx.x * PC_CHUNK;
    if (base >= lat.n) return;                                   // uniform; its words were not written
    const long first = start_in[0] + offs[slot];                 // where this chunk's points begin
    if (first >= capacity || offs[slot + 1] == offs[slot]) return;
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    __shared__ unsigned long long word_s[WORDS];
    __shared__ int prefix_s[WORDS];                              // kept candidates of the chunk before each word
    if (threadIdx.x < WAVE) {
        const unsigned long long wd = lane < WORDS ? bits[slot * WORDS + lane] : 0ull;
        const int c = __popcll(wd);
        int incl = c;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const int up = __shfl_up(incl, o, WAVE);
            if (lane >= o) incl += up;
        }
        if (lane < WORDS) word_s[lane] = wd, prefix_s[lane] = incl - c;
    }
    __syncthreads();
    const Plane<RECIP> pl = plane_of<RECIP>(pred, scale, b, h, w, t);
    const float* K = inv_K + (long)b * 16;
    const float k00 = K[0], k01 = K[1], k02 = K[2], k10 = K[4], k11 = K[5], k12 = K[6], k20 = K[8], k21 = K[9], k22 = K[10];
    const float* M = cam_to_world ? cam_to_world + (long)b * 16 : nullptr;
#pragma unroll 1
    for (int it = 0; it < ITERS; ++it) {
        const unsigned long long wd = word_s[it * WAVES + wave];
        if (!((wd >> lane) & 1ull)) continue;
        const long k = first + prefix_s[it * WAVES + wave] + __popcll(wd & ((1ull << lane) - 1ull));
        if (k >= capacity) continue;
        const long j = base + it * THREADS + threadIdx.x;
        const int vq = (int)(j / lat.Wc), uq = (int)(j - (long)vq * lat.Wc);
        const int v = vq * stride, u = uq * stride;
        const float d = pl.depth(t, v, u);
        const float fu = (float)u, fv = (float)v;
        const float c0 = ((k00 * fu + k01 * fv) + k02) * d;
        const float c1 = ((k10 * fu + k11 * fv) + k12) * d;
        const float c2 = ((k20 * fu + k21 * fv) + k22) * d;
        float x = c0, y = c1, z = c2;
        if (M) {
            x = ((M[0] * c0 + M[1] * c1) + M[2] * c2) + M[3];
            y = ((M[4] * c0 + M[5] * c1) + M[6] * c2) + M[7];
            z = ((M[8] * c0 + M[9] * c1) + M[10] * c2) + M[11];
        }
        xyz[k * 3] = x, xyz[k * 3 + 1] = y, xyz[k * 3 + 2] = z;
        const long pix = (long)v * t.W + u;
        index[k] = t.off + pix;
        if (colour_mode == 1) {
            const uint8_t* c = (const uint8_t*)colour + colour_off[b] + pix * 3;
            rgb[k * 3] = c[0], rgb[k * 3 + 1] = c[1], rgb[k * 3 + 2] = c[2];
        } else if (colour_mode == 2) {
            const float* c = (const float*)colour + (long)b * 3 * t.size + pix;
            rgb[k * 3] = unit_byte(c[0]), rgb[k * 3 + 1] = unit_byte(c[t.size]), rgb[k * 3 + 2] = unit_byte(c[2 * t.size]);
        }
    }
}

// 4 matrices per workgroup, a thread per element: all of a matrix is read before any of it is written
__global__ __launch_bounds__(WAVE) void pose_accumulate(float* __restrict__ world, const float* __restrict__ pose,
                                                        const uint8_t* __restrict__ present, int B, int F) {
    const int b = blockIdx.x * 4 + threadIdx.x / 16, e = threadIdx.x & 15, i = e >> 2, j = e & 3;
    float v = i == j ? 1.f : 0.f;
    if (b < B && present[(long)b * F] != 0) {
        const float* W = world + (long)b * 16 + i * 4;
        const float* P = pose + (long)b * F * 16 + j;
        v = ((W[0] * P[0] + W[1] * P[4]) + W[2] * P[8]) + W[3] * P[12];
    }
    __syncthreads();
    if (b < B) world[(long)b * 16 + e] = v;
}

}  // namespace

extern "C" long ppea_point_cloud_workspace_bytes(int B, long max_pixels, int stride) {
    if (B <= 0 || B > 65535 || max_pixels <= 0 || max_pixels > 0x7fffffffL || stride < 1) return PPEA_ERR_ARG;
    return workspace_bytes((long)B * chunks_of(max_pixels, stride));
}

extern "C" int ppea_point_cloud_f32(const float* pred, const float* scale, const int64_t* table, int B, int h, int w,
                                    long max_pixels, float lo, float hi, int mode, int stride, float edge,
                                    const float* inv_K, const float* cam_to_world, const void* colour,
                                    const int64_t* colour_off, int colour_mode, float* xyz, uint8_t* rgb, int64_t* index,
                                    long capacity, int64_t* cursor, int64_t* counts, void* workspace, void* stream) {
    if (!pred || !scale || !table || !inv_K || !cursor || !counts || !workspace) return PPEA_ERR_ARG;
    if (capacity > 0 && (!xyz || !index || (colour_mode != 0 && !rgb))) return PPEA_ERR_ARG;   // capacity 0: nothing is written
    if (B <= 0 || B > 65535 || h <= 0 || w <= 0 || h > 0x7fffffff / w || max_pixels <= 0) return PPEA_ERR_ARG;
    if (stride < 1 || capacity < 0 || colour_mode < 0 || colour_mode > 2) return PPEA_ERR_ARG;
    if (colour_mode != 0 && !colour) return PPEA_ERR_ARG;
    if (colour_mode == 1 && !colour_off) return PPEA_ERR_ARG;
    if (((uintptr_t)workspace & 7)) return PPEA_ERR_ARG;
    if (mode != 0 && mode != 1) return PPEA_ERR_UNSUPPORTED;
    if (max_pixels > 0x7fffffffL) return PPEA_ERR_UNSUPPORTED;
    const long chunks = chunks_of(max_pixels, stride), n = (long)B * chunks;
    const Workspace k = carve(workspace, n);
    const dim3 grid((unsigned)chunks, B);
    hipStream_t st = (hipStream_t)stream;
    if (mode == 1)
        mark<true><<<grid, THREADS, 0, st>>>(pred, scale, table, h, w, lo, hi, stride, edge, k.bits, k.count);
    else
        mark<false><<<grid, THREADS, 0, st>>>(pred, scale, table, h, w, lo, hi, stride, edge, k.bits, k.count);
    scan<<<1, SCAN_THREADS, 0, st>>>(k.count, k.offs, k.start, n, B, chunks, capacity, cursor, counts);
    if (mode == 1)
        scatter<true><<<grid, THREADS, 0, st>>>(pred, scale, table, h, w, stride, inv_K, cam_to_world, colour, colour_off,
                                                colour_mode, xyz, rgb, index, capacity, k.bits, k.offs, k.start);
    else
        scatter<false><<<grid, THREADS, 0, st>>>(pred, scale, table, h, w, stride, inv_K, cam_to_world, colour, colour_off,
                                                 colour_mode, xyz, rgb, index, capacity, k.bits, k.offs, k.start);
    return launch_status();
}

extern "C" int ppea_pose_accumulate_f32(float* world, const float* pose, const uint8_t* present, int B, int F,
                                        void* stream) {
    if (!world || !pose || !present || B <= 0 || F <= 0) return PPEA_ERR_ARG;
    pose_accumulate<<<(B + 3) / 4, WAVE, 0, (hipStream_t)stream>>>(world, pose, present, B, F);
    return launch_status();
}
