// Geometry of the photometric warp, gfx950:
//   A18+A19  BackprojectDepth -> Project3D fused        (layers.py:138-199)
//   A18, A19 the same two modules as one launch each, for callers that keep them apart or need the points
//   A20      F.grid_sample bilinear, align_corners=True  (trainer.py:911-914, rkm.py:299)
//   A15      axis-angle + translation -> 4x4, and the relative-pose chains built from it
// All HBM-bound streaming kernels: one thread per output pixel, coalesced NCHW rows,
// no intermediate [B,4,HW] point cloud (the reference writes ~5 MB/img for 1.5 MB
// of algorithmic traffic; here depth is read once and the grid written once).
//
// The projection arithmetic is written ONCE, in four device functions (load_rows, backproject_pixel, project_point,
// project_point_bwd); the six kernels of the fused and the split form are loads, one or two calls and stores.  The fused
// kernels pass the literal Xh[3] = 1.f: p * 1.f and dc * 1.f are exact and fold away, so where row 3 of the points is 1
// the split form carries the fused form's bits.  That, and the recorded bits of tests/golden/geometry_bits.npz, hold only
// while the expression trees below stay as written: the parentheses, the order of the k sums, division in the forward
// and reciprocal-multiply in the backward, -ffp-contract=off.  One silent change of association moves the pose gradient
// and, a few optimizer steps later, the whole pose branch.
#include <type_traits>

#include "common.h"

namespace {

// Rows 0-2, columns 0 .. COLS-1 of item b of a batch of row-major matrices with 4 columns, `stride` floats per item: 16 for
// [B,4,4] (inv_K; K @ T, whose `[:, :3, :]` is read in place without a copy), 12 for P [B,3,4].  Broadcast through SGPRs.
template <int COLS>
__device__ __forceinline__ void load_rows(const float* __restrict__ m, int stride, int b, float (&o)[3 * COLS]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < COLS; ++j) o[i * COLS + j] = m[b * stride + i * 4 + j];
}

// ray = inv_K[:3,:3] @ (x, y, 1) with the reference's matmul association (k = 0,1,2).
__device__ __forceinline__ void pixel_ray(const float (&ik)[9], float x, float y, float (&r)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) r[i] = (ik[i * 3] * x + ik[i * 3 + 1] * y) + ik[i * 3 + 2];
}

// BackprojectDepth at pixel (px, py): its ray r and the homogeneous point Xh = (depth * r, 1)
__device__ __forceinline__ void backproject_pixel(const float (&ik)[9], int px, int py, float d, float (&r)[3], float (&Xh)[4]) {
    pixel_ray(ik, (float)px, (float)py, r);
#pragma unroll
    for (int k = 0; k < 3; ++k) Xh[k] = d * r[k];
    Xh[3] = 1.f;
}

__device__ __forceinline__ float dot3(const float* a, const float (&r)[3]) { return a[0] * r[0] + a[1] * r[1] + a[2] * r[2]; }

// cam = P @ Xh in the reference's matmul association (k = 0,1,2,3)
__device__ __forceinline__ void camera_point(const float (&p)[12], const float (&Xh)[4], float (&cam)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
        cam[k] = ((p[k * 4] * Xh[0] + p[k * 4 + 1] * Xh[1]) + p[k * 4 + 2] * Xh[2]) + p[k * 4 + 3] * Xh[3];
}

// Project3D at one point -> (grid.x, grid.y, cam z); the pixel by DIVISION, as the reference forms it
__device__ __forceinline__ float3 project_point(const float (&p)[12], const float (&Xh)[4], int H, int W, float eps) {
    float cam[3];
    camera_point(p, Xh, cam);
    const float iz = cam[2] + eps;
    float u = cam[0] / iz, v = cam[1] / iz;
    u = u / (float)(W - 1);
    v = v / (float)(H - 1);
    return make_float3((u - 0.5f) * 2.f, (v - 0.5f) * 2.f, cam[2]);
}

// The gradient of project_point at one point, from d grid `dg` and d cam z `*dz` (NULL: none): dc = d cam, dX = P^T dc and
// the 12 terms g[k * 4 + j] = dc[k] * Xh[j] of dP.  The pixel by RECIPROCAL-MULTIPLY here.
__device__ __forceinline__ void project_point_bwd(const float (&p)[12], const float (&Xh)[4], float2 dg, const float* __restrict__ dz,
                                                  int H, int W, float eps, float (&dc)[3], float (&dX)[4], float (&g)[12]) {
    float cam[3];
    camera_point(p, Xh, cam);
    const float iz = 1.f / (cam[2] + eps);
    const float u = cam[0] * iz, v = cam[1] * iz;
    const float du = dg.x * 2.f / (float)(W - 1), dv = dg.y * 2.f / (float)(H - 1);
    dc[0] = du * iz;
    dc[1] = dv * iz;
    dc[2] = -(du * u + dv * v) * iz;
    if (dz != nullptr) dc[2] = dc[2] + *dz;
#pragma unroll
    for (int j = 0; j < 4; ++j) dX[j] = p[j] * dc[0] + p[4 + j] * dc[1] + p[8 + j] * dc[2];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) g[k * 4 + j] = dc[k] * Xh[j];
}

// N per-thread terms -> one partial per block and entry in partial [B][blocks][N] (wave shuffle -> LDS -> fixed tree);
// bp_reduce_4x4 adds them in a fixed order.  Round 1 added the block sums with float atomics: the pose gradient -- and, after a
// few optimizer steps, the whole pose branch -- then depended on the order in which the 480 blocks of an image happened to
// finish.
template <int N>
__device__ __forceinline__ void block_partials(const float (&g)[N], float (&red)[4][N], float* __restrict__ partial, int b) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const float s = wave_sum(g[k]);
        if (lane == 0) red[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const float s = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        partial[((long)b * gridDim.x + blockIdx.x) * N + threadIdx.x] = s;
    }
}

// out [B][ROWS][4] (ROWS = 4: a 4x4; 3: the fused form's [B,3,4]): the R x C sums over the image's blocks in the upper-left
// corner, zeros elsewhere; always in the same order (one wave per batch item: lane-strided over the blocks, then wave_sum,
// entry by entry).  <3,4,3>: dP [B,3,4]; <3,4,4>: dP [B,4,4]; <3,3,4>: d_inv_K [B,4,4].
template <int R, int C, int ROWS>
__global__ __launch_bounds__(64) void bp_reduce_4x4(const float* __restrict__ partial, float* __restrict__ out, int blocks) {
    const int b = blockIdx.x, lane = threadIdx.x;
    float acc[R * C];
#pragma unroll
    for (int k = 0; k < R * C; ++k) acc[k] = 0.f;
    for (int i = lane; i < blocks; i += 64) {
        const float* p = partial + ((long)b * blocks + i) * (R * C);
#pragma unroll
        for (int k = 0; k < R * C; ++k) acc[k] += p[k];
    }
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < R * C; ++k) {
        const float s = wave_sum(acc[k]);
        if (lane == (k / C) * 4 + k % C) v = s;
    }
    if (lane < ROWS * 4) out[b * (ROWS * 4) + lane] = v;
}

// ---- A18+A19 fused: depth -> grid, P [B,3,4] ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void backproject_project_fwd(const float* __restrict__ depth,
                                                               const float* __restrict__ inv_K,
                                                               const float* __restrict__ P,
                                                               float* __restrict__ grid, int H, int W,
                                                               float eps) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const long HW = (long)H * W;
    if (i >= HW) return;
    float ik[9], p[12];
    load_rows<3>(inv_K, 16, b, ik);
    load_rows<4>(P, 12, b, p);
    const int py = i / W, px = i - py * W;
    float r[3], Xh[4];
    backproject_pixel(ik, px, py, depth[b * HW + i], r, Xh);
    const float3 o = project_point(p, Xh, H, W, eps);
    reinterpret_cast<float2*>(grid)[b * HW + i] = make_float2(o.x, o.y);
}

// d_depth (per pixel) and the 12 per-block sums of dP in `partial` [B][blocks][12]
__global__ __launch_bounds__(256) void backproject_project_bwd(const float* __restrict__ depth,
                                                               const float* __restrict__ inv_K,
                                                               const float* __restrict__ P,
                                                               const float* __restrict__ d_grid,
                                                               float* __restrict__ d_depth,
                                                               float* __restrict__ partial, int H, int W,
                                                               float eps) {
    __shared__ float red[4][12];
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const long HW = (long)H * W;
    float ik[9], p[12];
    load_rows<3>(inv_K, 16, b, ik);
    load_rows<4>(P, 12, b, p);
    float g[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) g[k] = 0.f;
    if (i < HW) {
        const int py = i / W, px = i - py * W;
        float r[3], Xh[4], dc[3], dX[4];
        backproject_pixel(ik, px, py, depth[b * HW + i], r, Xh);
        project_point_bwd(p, Xh, reinterpret_cast<const float2*>(d_grid)[b * HW + i], nullptr, H, W, eps, dc, dX, g);
        d_depth[b * HW + i] = dot3(dX, r);
    }
    block_partials<12>(g, red, partial, b);
}

// ---- the same geometry split at the point cloud (layers.py:138-199 as two modules) ---------------------------------------
// BackprojectDepth and Project3D for callers that keep the reference's two-module form or need the [B,4,HW] points / the
// projected depth themselves.  P is the [B,4,4] product K @ T.
__global__ __launch_bounds__(256) void backproject_fwd(const float* __restrict__ depth, const float* __restrict__ inv_K,
                                                       float* __restrict__ points, int H, int W) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const long HW = (long)H * W;
    if (i >= HW) return;
    float ik[9];
    load_rows<3>(inv_K, 16, b, ik);
    const int py = i / W, px = i - py * W;
    float r[3], Xh[4];
    backproject_pixel(ik, px, py, depth[b * HW + i], r, Xh);
    float* o = points + (long)b * 4 * HW + i;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j * HW] = Xh[j];
}

// d_depth (NULL: not wanted) = d_points[:3] . ray; partial != NULL: the 9 sums of d inv_K[:3,:3], entry (i, j) = d_points[i] * depth * (x, y, 1)[j]
__global__ __launch_bounds__(256) void backproject_bwd(const float* __restrict__ depth, const float* __restrict__ inv_K,
                                                       const float* __restrict__ d_points, float* __restrict__ d_depth,
                                                       float* __restrict__ partial, int H, int W) {
    __shared__ float red[4][9];
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const long HW = (long)H * W;
    float ik[9];
    load_rows<3>(inv_K, 16, b, ik);
    float g[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) g[k] = 0.f;
    if (i < HW) {
        const int py = i / W, px = i - py * W;
        const float xy[3] = {(float)px, (float)py, 1.f};
        float r[3];
        pixel_ray(ik, xy[0], xy[1], r);
        const float* dp = d_points + (long)b * 4 * HW + i;
        const float dX[3] = {dp[0], dp[HW], dp[2 * HW]};
        if (d_depth != nullptr) d_depth[b * HW + i] = dot3(dX, r);
        if (partial != nullptr) {
            const float d = depth[b * HW + i];
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int j = 0; j < 3; ++j) g[k * 3 + j] = (dX[k] * d) * xy[j];
        }
    }
    if (partial != nullptr) block_partials<9>(g, red, partial, b);      // uniform over the launch
}

__global__ __launch_bounds__(256) void project3d_fwd(const float* __restrict__ points, const float* __restrict__ P,
                                                     float* __restrict__ grid, float* __restrict__ z, int H, int W, float eps) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const long HW = (long)H * W;
    if (i >= HW) return;
    float p[12];
    load_rows<4>(P, 16, b, p);
    const float* x = points + (long)b * 4 * HW + i;
    const float Xh[4] = {x[0], x[HW], x[2 * HW], x[3 * HW]};
    const float3 o = project_point(p, Xh, H, W, eps);
    reinterpret_cast<float2*>(grid)[b * HW + i] = make_float2(o.x, o.y);
    if (z != nullptr) z[b * HW + i] = o.z;
}

// d_points [B,4,HW] (NULL: not wanted) and, with partial != NULL, the 12 per-block sums of dP; d_z (NULL: none) is the
// gradient of the projected depth cam[2]
__global__ __launch_bounds__(256) void project3d_bwd(const float* __restrict__ points, const float* __restrict__ P,
                                                     const float* __restrict__ d_grid, const float* __restrict__ d_z,
                                                     float* __restrict__ d_points, float* __restrict__ partial, int H, int W,
                                                     float eps) {
    __shared__ float red[4][12];
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const long HW = (long)H * W;
    float p[12];
    load_rows<4>(P, 16, b, p);
    float g[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) g[k] = 0.f;
    if (i < HW) {
        const float* x = points + (long)b * 4 * HW + i;
        const float Xh[4] = {x[0], x[HW], x[2 * HW], x[3 * HW]};
        float dc[3], dX[4];
        project_point_bwd(p, Xh, reinterpret_cast<const float2*>(d_grid)[b * HW + i], d_z != nullptr ? d_z + b * HW + i : nullptr,
                          H, W, eps, dc, dX, g);
        if (d_points != nullptr) {
            float* o = d_points + (long)b * 4 * HW + i;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j * HW] = dX[j];
        }
    }
    if (partial != nullptr) block_partials<12>(g, red, partial, b);     // uniform over the launch
}

// ---- grid_sample -----------------------------------------------------------------------
struct Tap {
    int x0, y0;
    float tx, ty;       // fractional parts
    float mx, my;       // d(ix)/d(grid.x), d(iy)/d(grid.y) incl. the border clip gate
};

__device__ __forceinline__ Tap make_tap(float gx, float gy, int Wi, int Hi, bool border) {
    // align_corners=True un-normalisation: ix = (x + 1) / 2 * (W - 1)
    float ix = ((gx + 1.f) / 2.f) * (float)(Wi - 1);
    float iy = ((gy + 1.f) / 2.f) * (float)(Hi - 1);
    Tap t;
    t.mx = (float)(Wi - 1) / 2.f;
    t.my = (float)(Hi - 1) / 2.f;
    if (border) {       // clip_coordinates_set_grad: zero gradient at and beyond the rim
        if (!(ix > 0.f)) { ix = 0.f; t.mx = 0.f; } else if (ix >= (float)(Wi - 1)) { ix = (float)(Wi - 1); t.mx = 0.f; }
        if (!(iy > 0.f)) { iy = 0.f; t.my = 0.f; } else if (iy >= (float)(Hi - 1)) { iy = (float)(Hi - 1); t.my = 0.f; }
    }
    const float fx = floorf(ix), fy = floorf(iy);
    t.tx = ix - fx;
    t.ty = iy - fy;
    // far-out-of-range coordinates (zeros mode): keep the int conversion defined; all four
    // corners are then outside the image and contribute 0.
    t.x0 = (int)fminf(fmaxf(fx, -4.f), (float)Wi + 4.f);
    t.y0 = (int)fminf(fmaxf(fy, -4.f), (float)Hi + 4.f);
    return t;
}

__device__ __forceinline__ float fetch(const float* __restrict__ plane, int x, int y, int Wi, int Hi) {
    return (x >= 0 && x < Wi && y >= 0 && y < Hi) ? plane[(long)y * Wi + x] : 0.f;
}

__global__ __launch_bounds__(256) void grid_sample_fwd(const float* __restrict__ src,
                                                       const float* __restrict__ grid,
                                                       float* __restrict__ out, int C, int Hi, int Wi,
                                                       int Ho, int Wo, int border) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Ho * Wo) return;
    const float2 g = reinterpret_cast<const float2*>(grid)[(long)b * Ho * Wo + i];
    const Tap t = make_tap(g.x, g.y, Wi, Hi, border != 0);
    // weights exactly as ATen: nw = (x1 - ix)(y1 - iy) etc.
    const float wx1 = t.tx, wx0 = 1.f - t.tx, wy1 = t.ty, wy0 = 1.f - t.ty;
    for (int c = 0; c < C; ++c) {
        const float* plane = src + ((long)b * C + c) * Hi * Wi;
        const float v00 = fetch(plane, t.x0, t.y0, Wi, Hi), v01 = fetch(plane, t.x0 + 1, t.y0, Wi, Hi);
        const float v10 = fetch(plane, t.x0, t.y0 + 1, Wi, Hi), v11 = fetch(plane, t.x0 + 1, t.y0 + 1, Wi, Hi);
        out[((long)b * C + c) * Ho * Wo + i] = ((v00 * (wx0 * wy0) + v01 * (wx1 * wy0)) + v10 * (wx0 * wy1)) + v11 * (wx1 * wy1);
    }
}

__global__ __launch_bounds__(256) void grid_sample_bwd_grid(const float* __restrict__ src,
                                                            const float* __restrict__ grid,
                                                            const float* __restrict__ d_out,
                                                            float* __restrict__ d_grid, int C, int Hi,
                                                            int Wi, int Ho, int Wo, int border) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Ho * Wo) return;
    const float2 g = reinterpret_cast<const float2*>(grid)[(long)b * Ho * Wo + i];
    const Tap t = make_tap(g.x, g.y, Wi, Hi, border != 0);
    float gx = 0.f, gy = 0.f;
    for (int c = 0; c < C; ++c) {
        const float* plane = src + ((long)b * C + c) * Hi * Wi;
        const float v00 = fetch(plane, t.x0, t.y0, Wi, Hi), v01 = fetch(plane, t.x0 + 1, t.y0, Wi, Hi);
        const float v10 = fetch(plane, t.x0, t.y0 + 1, Wi, Hi), v11 = fetch(plane, t.x0 + 1, t.y0 + 1, Wi, Hi);
        const float go = d_out[((long)b * C + c) * Ho * Wo + i];
        gx += go * ((v01 - v00) * (1.f - t.ty) + (v11 - v10) * t.ty);
        gy += go * ((v10 - v00) * (1.f - t.tx) + (v11 - v01) * t.tx);
    }
    float2 o;
    o.x = gx * t.mx;
    o.y = gy * t.my;
    reinterpret_cast<float2*>(d_grid)[(long)b * Ho * Wo + i] = o;
}


// ---- A15: axis-angle + translation -> 4x4 transformation (layers.py:26-42, 61-100) --------------------------------------
// One thread per sample.  The reference builds the matrix from ~25 tiny element-wise kernels (and autograd adds ~50 more on
// the way back) on the step's critical stream; here the forward is one launch and the backward one launch whose Jacobian
// comes from running the SAME arithmetic on dual numbers (value + 6 partial derivatives): exact, no hand-derived formulas.
struct Dual6 {
    float v, d[6];
};
__device__ __forceinline__ Dual6 dconst(float c) { Dual6 r; r.v = c; for (int i = 0; i < 6; ++i) r.d[i] = 0.f; return r; }
__device__ __forceinline__ Dual6 dvar(float c, int k) { Dual6 r = dconst(c); r.d[k] = 1.f; return r; }
__device__ __forceinline__ Dual6 operator+(const Dual6& a, const Dual6& b) { Dual6 r; r.v = a.v + b.v; for (int i = 0; i < 6; ++i) r.d[i] = a.d[i] + b.d[i]; return r; }
__device__ __forceinline__ Dual6 operator-(const Dual6& a, const Dual6& b) { Dual6 r; r.v = a.v - b.v; for (int i = 0; i < 6; ++i) r.d[i] = a.d[i] - b.d[i]; return r; }
__device__ __forceinline__ Dual6 operator*(const Dual6& a, const Dual6& b) { Dual6 r; r.v = a.v * b.v; for (int i = 0; i < 6; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i]; return r; }
__device__ __forceinline__ Dual6 operator/(const Dual6& a, const Dual6& b) {
    Dual6 r; r.v = a.v / b.v;
    for (int i = 0; i < 6; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) / b.v;
    return r;
}
__device__ __forceinline__ Dual6 dsqrt(const Dual6& a) { Dual6 r; r.v = sqrtf(a.v); for (int i = 0; i < 6; ++i) r.d[i] = a.v > 0.f ? a.d[i] / (2.f * r.v) : 0.f; return r; }
__device__ __forceinline__ Dual6 dsin(const Dual6& a) { Dual6 r; r.v = sinf(a.v); const float c = cosf(a.v); for (int i = 0; i < 6; ++i) r.d[i] = c * a.d[i]; return r; }
__device__ __forceinline__ Dual6 dcos(const Dual6& a) { Dual6 r; r.v = cosf(a.v); const float s = -sinf(a.v); for (int i = 0; i < 6; ++i) r.d[i] = s * a.d[i]; return r; }

// T[16] row-major from (axis-angle vx, vy, vz, translation tx, ty, tz); `N` is float (forward) or Dual6 (backward)
template <typename N>
__device__ __forceinline__ void pose_matrix(const N& vx, const N& vy, const N& vz, const N& tx, const N& ty, const N& tz, int invert,
                                            N (&T)[16], N (*cst)(float), N (*sq)(const N&), N (*sn)(const N&), N (*cs)(const N&)) {
    const N angle = sq(vx * vx + vy * vy + vz * vz);
    const N den = angle + cst(1e-7f);
    const N x = vx / den, y = vy / den, z = vz / den;
    const N ca = cs(angle), sa = sn(angle);
    const N C = cst(1.f) - ca;
    const N xC = x * C, yC = y * C, zC = z * C;
    N R[9] = {x * xC + ca, x * yC - z * sa, z * xC + y * sa,
              x * yC + z * sa, y * yC + ca, y * zC - x * sa,
              z * xC - y * sa, y * zC + x * sa, z * zC + ca};
    const N zero = cst(0.f), one = cst(1.f);
    if (!invert) {                                           // T(t) . R  = [R | t]
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) T[4 * i + j] = R[3 * i + j];
        }
        T[3] = tx; T[7] = ty; T[11] = tz;
    } else {                                                 // R^T . T(-t) = [R^T | -R^T t]
        const N nx = zero - tx, ny = zero - ty, nz = zero - tz;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) T[4 * i + j] = R[3 * j + i];
            T[4 * i + 3] = R[i] * nx + R[3 + i] * ny + R[6 + i] * nz;
        }
    }
    T[12] = zero; T[13] = zero; T[14] = zero; T[15] = one;
}
__device__ __forceinline__ float fconst(float c) { return c; }
__device__ __forceinline__ float fsqrt(const float& a) { return sqrtf(a); }
__device__ __forceinline__ float fsin(const float& a) { return sinf(a); }
__device__ __forceinline__ float fcos(const float& a) { return cosf(a); }

// the fp32 forward of one sample: aa, tr point at its three axis-angle / translation components
__device__ __forceinline__ void pose_matrix_f32(const float* __restrict__ aa, const float* __restrict__ tr, int invert, float (&M)[16]) {
    pose_matrix<float>(aa[0], aa[1], aa[2], tr[0], tr[1], tr[2], invert, M, fconst, fsqrt, fsin, fcos);
}

__global__ void pose_matrix_fwd(const float* __restrict__ aa, const float* __restrict__ tr, float* __restrict__ T, int B, int invert) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float M[16];
    pose_matrix_f32(aa + 3 * b, tr + 3 * b, invert, M);
    for (int i = 0; i < 16; ++i) T[16 * b + i] = M[i];
}

// ---- relative poses of the F lookup frames in one launch (repdepth.py:465-507) -----------------------------------------
// Frame f takes the pose network's output of pair c.pair[f] (sample b at aa[pair] + b * stride), builds its matrix with
// pose_matrix_f32 (c.invert[f]), multiplies it from the left onto the relative pose of its predecessor c.pred[f] (-1: none)
//     T(f)[i][j] = ((A[i][0] P[0][j] + A[i][1] P[1][j]) + A[i][2] P[2][j]) + A[i][3] P[3][j]       (k = 0, 1, 2, 3)
// and is then masked with keep[b][f] (NULL: keep all): a flagged-off entry is exact zeros, and the MASKED matrix is what its successors
// multiply with (the reference masks inputs[("relative_pose", f)] before the next frame reads it).  One thread per batch
// item walks the chain in frame order (pred[f] < f), every matrix in registers.  The chain description travels by value.
#define POSE_CHAIN_MAX 4
struct PoseChain {
    const float* aa[POSE_CHAIN_MAX];
    const float* tr[POSE_CHAIN_MAX];
    int pair[POSE_CHAIN_MAX], invert[POSE_CHAIN_MAX], pred[POSE_CHAIN_MAX];
};

// A <- A @ R (A multiplied from the left onto R), 4x4 row-major, each entry summed as in the formula above; both chain
// kernels multiply through this function
__device__ __forceinline__ void left_multiply(float (&A)[16], const float (&R)[16]) {
    float P[16];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            P[4 * i + j] = ((A[4 * i] * R[j] + A[4 * i + 1] * R[4 + j]) + A[4 * i + 2] * R[8 + j]) + A[4 * i + 3] * R[12 + j];
#pragma unroll
    for (int i = 0; i < 16; ++i) A[i] = P[i];
}

template <int F>
__global__ void pose_chain_fwd(PoseChain c, const float* __restrict__ keep, float* __restrict__ T, int B, int stride) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float R[F][16];
#pragma unroll
    for (int f = 0; f < F; ++f) {
        float A[16];
        pose_matrix_f32(c.aa[c.pair[f]] + (long)b * stride, c.tr[c.pair[f]] + (long)b * stride, c.invert[f], A);
        const bool on = keep == nullptr || keep[b * F + f] != 0.f;
#pragma unroll
        for (int g = 0; g < F; ++g) {
            if (g < f && c.pred[f] == g) left_multiply(A, R[g]);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            R[f][i] = on ? A[i] : 0.f;
            T[((long)b * F + f) * 16 + i] = R[f][i];
        }
    }
}

// ---- the same chain on a video stream: the pairs come from a device ring ------------------------------------------------
// ring [F][B][2][3]: slot s holds the pose decoder's raw (axisangle, translation) of one pair of consecutive frames.  With
// head = state[0] (brought into 0 .. F - 1) the pair (t - j - 1, t - j) is slot (head - j) mod F; `aa_new` / `tr_new`
// (sample b at + b * stride; NULL: the ring already holds it) is the newest pair (t - 1, t) and is written into slot head
// first.  T(0 -> -1) = inv(pair 0), T(0 -> -(j + 1)) = inv(pair j) @ T(0 -> -j), each built by pose_matrix_f32 and
// multiplied by left_multiply.  seen = state[1 + b] frames came before this one: frame j of item b is present iff
// seen > j; an absent frame is exact zeros (so is everything behind it: seen <= j implies seen <= j + 1) and its slot is
// never read.  present [B][F] bytes.  One thread per item; a thread touches only its own item's words of the ring.
template <int F>
__global__ void pose_chain_ring_fwd(const float* __restrict__ aa_new, const float* __restrict__ tr_new, int stride,
                                    float* ring, const int32_t* __restrict__ state, float* __restrict__ T,
                                    uint8_t* __restrict__ present, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int head = state[0] % F;
    if (head < 0) head += F;
    const int seen = state[1 + b];
    float R[16];
#pragma unroll
    for (int j = 0; j < F; ++j) {
        int slot = head - j;
        if (slot < 0) slot += F;
        float* pr = ring + ((long)slot * B + b) * 6;
        float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (j == 0 && aa_new != nullptr) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                v[k] = aa_new[(long)b * stride + k];
                v[3 + k] = tr_new[(long)b * stride + k];
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) pr[k] = v[k];
        }
        const bool on = seen > j;
        float A[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) A[i] = 0.f;
        if (on) {
            if (!(j == 0 && aa_new != nullptr)) {
#pragma unroll
                for (int k = 0; k < 6; ++k) v[k] = pr[k];
            }
            pose_matrix_f32(v, v + 3, 1, A);
            if (j > 0) left_multiply(A, R);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            R[i] = A[i];
            T[((long)b * F + j) * 16 + i] = A[i];
        }
        present[b * F + j] = on ? 1 : 0;
    }
}

__global__ void pose_matrix_bwd(const float* __restrict__ aa, const float* __restrict__ tr, const float* __restrict__ dT,
                                float* __restrict__ daa, float* __restrict__ dtr, int B, int invert) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    Dual6 M[16];
    pose_matrix<Dual6>(dvar(aa[3 * b], 0), dvar(aa[3 * b + 1], 1), dvar(aa[3 * b + 2], 2), dvar(tr[3 * b], 3), dvar(tr[3 * b + 1], 4),
                       dvar(tr[3 * b + 2], 5), invert, M, dconst, dsqrt, dsin, dcos);
    float g[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < 16; ++i) {
        const float w = dT[16 * b + i];
        for (int k = 0; k < 6; ++k) g[k] += w * M[i].d[k];
    }
    for (int k = 0; k < 3; ++k) { daa[3 * b + k] = g[k]; dtr[3 * b + k] = g[3 + k]; }
}


// kernel<F> for F = 1 .. POSE_CHAIN_MAX (checked by the callers): fn receives std::integral_constant<int, F>
template <typename Fn>
void with_frames(int F, Fn fn) {
    switch (F) {
        case 1: fn(std::integral_constant<int, 1>()); break;
        case 2: fn(std::integral_constant<int, 2>()); break;
        case 3: fn(std::integral_constant<int, 3>()); break;
        default: fn(std::integral_constant<int, 4>()); break;
    }
}

// The six projection entry points: B is gridDim.y and a pixel index an int.  min_hw = 2 where the grid is normalised by
// W - 1 and H - 1, 1 for backproject_*.
bool dims_ok(int B, int H, int W, int min_hw) {
    return B >= 0 && B <= 65535 && H >= min_hw && W >= min_hw && (long)H * W <= 0x7fffff00L;
}
dim3 pixel_grid(int B, int H, int W) { return dim3((H * W + 255) / 256, B); }

// bytes of the [B][blocks][n] per-block sums of a backward launch
long partial_bytes(int B, int H, int W, int min_hw, int n) {
    if (B <= 0 || H < min_hw || W < min_hw) return 0;
    return (long)B * (((long)H * W + 255) / 256) * n * (long)sizeof(float);
}

}  // namespace

extern "C" {

int ppea_backproject_project_fwd_f32(const float* depth, const float* inv_K, const float* P, float* grid,
                                     int B, int H, int W, float eps, void* stream) {
    if (!dims_ok(B, H, W, 2)) return PPEA_ERR_UNSUPPORTED;
    if (B == 0) return 0;
    hipLaunchKernelGGL(backproject_project_fwd, pixel_grid(B, H, W), dim3(256), 0, (hipStream_t)stream, depth, inv_K, P, grid,
                       H, W, eps);
    return launch_status();
}

long ppea_backproject_project_bwd_workspace_bytes(int B, int H, int W) { return partial_bytes(B, H, W, 2, 12); }

int ppea_backproject_project_bwd_f32(const float* depth, const float* inv_K, const float* P,
                                     const float* d_grid, float* d_depth, float* dP, void* workspace, int B, int H,
                                     int W, float eps, void* stream) {
    if (!dims_ok(B, H, W, 2)) return PPEA_ERR_UNSUPPORTED;
    if (B == 0) return 0;
    if (workspace == nullptr) return PPEA_ERR_ARG;
    const dim3 g = pixel_grid(B, H, W);
    hipLaunchKernelGGL(backproject_project_bwd, g, dim3(256), 0, (hipStream_t)stream, depth, inv_K, P,
                       d_grid, d_depth, (float*)workspace, H, W, eps);
    hipLaunchKernelGGL((bp_reduce_4x4<3, 4, 3>), dim3(B), dim3(64), 0, (hipStream_t)stream, (const float*)workspace, dP, (int)g.x);
    return launch_status();
}

// BackprojectDepth / Project3D as separate launches (see backproject_fwd ... project3d_bwd above)
int ppea_backproject_fwd_f32(const float* depth, const float* inv_K, float* points, int B, int H, int W, void* stream) {
    if (!dims_ok(B, H, W, 1)) return PPEA_ERR_UNSUPPORTED;
    if (B == 0) return 0;
    if (!depth || !inv_K || !points) return PPEA_ERR_ARG;
    hipLaunchKernelGGL(backproject_fwd, pixel_grid(B, H, W), dim3(256), 0, (hipStream_t)stream, depth, inv_K, points, H, W);
    return launch_status();
}

long ppea_backproject_bwd_workspace_bytes(int B, int H, int W) { return partial_bytes(B, H, W, 1, 9); }

int ppea_backproject_bwd_f32(const float* depth, const float* inv_K, const float* d_points, float* d_depth, float* d_inv_K,
                             void* workspace, int B, int H, int W, void* stream) {
    if (!dims_ok(B, H, W, 1)) return PPEA_ERR_UNSUPPORTED;
    if (B == 0) return 0;
    if (!depth || !inv_K || !d_points || (d_depth == nullptr && d_inv_K == nullptr) || (d_inv_K != nullptr && workspace == nullptr))
        return PPEA_ERR_ARG;
    const dim3 g = pixel_grid(B, H, W);
    float* partial = d_inv_K != nullptr ? (float*)workspace : nullptr;
    hipLaunchKernelGGL(backproject_bwd, g, dim3(256), 0, (hipStream_t)stream, depth, inv_K, d_points, d_depth, partial, H, W);
    if (d_inv_K != nullptr)
        hipLaunchKernelGGL((bp_reduce_4x4<3, 3, 4>), dim3(B), dim3(64), 0, (hipStream_t)stream, (const float*)partial, d_inv_K, (int)g.x);
    return launch_status();
}

int ppea_project3d_fwd_f32(const float* points, const float* P, float* grid, float* z, int B, int H, int W, float eps,
                           void* stream) {
    if (!dims_ok(B, H, W, 2)) return PPEA_ERR_UNSUPPORTED;
    if (B == 0) return 0;
    if (!points || !P || !grid) return PPEA_ERR_ARG;
    hipLaunchKernelGGL(project3d_fwd, pixel_grid(B, H, W), dim3(256), 0, (hipStream_t)stream, points, P, grid, z, H, W, eps);
    return launch_status();
}

long ppea_project3d_bwd_workspace_bytes(int B, int H, int W) { return partial_bytes(B, H, W, 2, 12); }

int ppea_project3d_bwd_f32(const float* points, const float* P, const float* d_grid, const float* d_z, float* d_points,
                           float* dP, void* workspace, int B, int H, int W, float eps, void* stream) {
    if (!dims_ok(B, H, W, 2)) return PPEA_ERR_UNSUPPORTED;
    if (B == 0) return 0;
    if (!points || !P || !d_grid || (d_points == nullptr && dP == nullptr) || (dP != nullptr && workspace == nullptr))
        return PPEA_ERR_ARG;
    const dim3 g = pixel_grid(B, H, W);
    float* partial = dP != nullptr ? (float*)workspace : nullptr;
    hipLaunchKernelGGL(project3d_bwd, g, dim3(256), 0, (hipStream_t)stream, points, P, d_grid, d_z, d_points, partial, H, W, eps);
    if (dP != nullptr)
        hipLaunchKernelGGL((bp_reduce_4x4<3, 4, 4>), dim3(B), dim3(64), 0, (hipStream_t)stream, (const float*)partial, dP, (int)g.x);
    return launch_status();
}

int ppea_grid_sample_fwd_f32(const float* src, const float* grid, float* out, int B, int C, int Hi, int Wi,
                             int Ho, int Wo, int padding, void* stream) {
    if (B < 0 || C <= 0 || Hi <= 0 || Wi <= 0 || Ho <= 0 || Wo <= 0 || (padding != 0 && padding != 1))
        return PPEA_ERR_UNSUPPORTED;
    if (B == 0) return 0;
    dim3 g((Ho * Wo + 255) / 256, B);
    hipLaunchKernelGGL(grid_sample_fwd, g, dim3(256), 0, (hipStream_t)stream, src, grid, out, C, Hi, Wi,
                       Ho, Wo, padding);
    return launch_status();
}

int ppea_grid_sample_bwd_grid_f32(const float* src, const float* grid, const float* d_out, float* d_grid,
                                  int B, int C, int Hi, int Wi, int Ho, int Wo, int padding, void* stream) {
    if (B < 0 || C <= 0 || Hi <= 0 || Wi <= 0 || Ho <= 0 || Wo <= 0 || (padding != 0 && padding != 1))
        return PPEA_ERR_UNSUPPORTED;
    if (B == 0) return 0;
    dim3 g((Ho * Wo + 255) / 256, B);
    hipLaunchKernelGGL(grid_sample_bwd_grid, g, dim3(256), 0, (hipStream_t)stream, src, grid, d_out, d_grid,
                       C, Hi, Wi, Ho, Wo, padding);
    return launch_status();
}


// A15 (layers.py:26-42, 61-100): T [B][4][4] fp32 from axis-angle aa [B][3] and translation tr [B][3] (invert: the inverse
// transformation R^T T(-t)); backward: d aa, d tr from dT (exact Jacobian of the same arithmetic).
int ppea_pose_matrix_fwd_f32(const float* aa, const float* tr, float* T, int B, int invert, void* stream) {
    if (B < 0) return PPEA_ERR_ARG;
    if (B == 0) return 0;
    if (!aa || !tr || !T) return PPEA_ERR_ARG;
    hipLaunchKernelGGL(pose_matrix_fwd, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, aa, tr, T, B, invert);
    return launch_status();
}
// Relative poses of F lookup frames from P pose-network outputs (see pose_chain_fwd).  aa, tr: HOST arrays of P device
// pointers; pair, invert, pred: HOST arrays of F ints -- everything but keep and T is copied into the launch's arguments.
int ppea_pose_chain_fwd_f32(const float* const* aa, const float* const* tr, int P, int stride, const int* pair,
                            const int* invert, const int* pred, const float* keep, float* T, int B, int F, void* stream) {
    if (B < 0 || F < 1 || F > POSE_CHAIN_MAX || P < 1 || P > POSE_CHAIN_MAX) return PPEA_ERR_UNSUPPORTED;
    if (!aa || !tr || !pair || !invert || !pred || stride < 3) return PPEA_ERR_ARG;
    PoseChain c = {};
    for (int p = 0; p < P; ++p) {
        if (!aa[p] || !tr[p]) return PPEA_ERR_ARG;
        c.aa[p] = aa[p];
        c.tr[p] = tr[p];
    }
    for (int f = 0; f < F; ++f) {
        if (pair[f] < 0 || pair[f] >= P || pred[f] < -1 || pred[f] >= f) return PPEA_ERR_ARG;
        c.pair[f] = pair[f];
        c.invert[f] = invert[f] != 0;
        c.pred[f] = pred[f];
    }
    if (B == 0) return 0;
    if (!T) return PPEA_ERR_ARG;
    with_frames(F, [&](auto f) {
        hipLaunchKernelGGL(pose_chain_fwd<decltype(f)::value>, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, c, keep, T,
                           B, stride);
    });
    return launch_status();
}
// The chain of a video stream (see pose_chain_ring_fwd): ring [F][B][2][3] fp32 and state [1 + B] int32 on the device;
// aa_new, tr_new: the newest pair's decoder output, sample b at + b * stride floats (both NULL: slot head already holds it),
// stored into slot head by this launch.  T [B][F][4][4]; present [B][F] bytes, 1 where seen[b] > j.
int ppea_pose_chain_ring_fwd_f32(const float* aa_new, const float* tr_new, int stride, float* ring, const int32_t* state,
                                 float* T, uint8_t* present, int B, int F, void* stream) {
    if (B < 0 || F < 1 || F > POSE_CHAIN_MAX) return PPEA_ERR_UNSUPPORTED;
    if ((aa_new == nullptr) != (tr_new == nullptr) || (aa_new != nullptr && stride < 3)) return PPEA_ERR_ARG;
    if (B == 0) return 0;
    if (!ring || !state || !T || !present) return PPEA_ERR_ARG;
    with_frames(F, [&](auto f) {
        hipLaunchKernelGGL(pose_chain_ring_fwd<decltype(f)::value>, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, aa_new,
                           tr_new, stride, ring, state, T, present, B);
    });
    return launch_status();
}
int ppea_pose_matrix_bwd_f32(const float* aa, const float* tr, const float* dT, float* daa, float* dtr, int B, int invert,
                             void* stream) {
    if (B < 0) return PPEA_ERR_ARG;
    if (B == 0) return 0;
    if (!aa || !tr || !dT || !daa || !dtr) return PPEA_ERR_ARG;
    hipLaunchKernelGGL(pose_matrix_bwd, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, aa, tr, dT, daa, dtr, B, invert);
    return launch_status();
}

}  // extern "C"
