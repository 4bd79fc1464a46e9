// Filter gradient of the large-kernel depthwise convolution (+ its 5x5 branch) on the matrix cores, bf16 activations
// (full fine-tuning, --fullft_reb, and the plug-in's weight.grad):
//     dw[c][u][v] = sum_{n,i,j} dy[n][c][i][j] * x[n][c][i+u-K/2][j+v-K/2]            (zero outside the plane)
// Per channel this is a GEMM once the reduction index runs over the INPUT row: with k = (n, r, j)
//     dw_c[u][v] = sum_k P[u][k] * Q[v][k],   P[u][(n,r,j)] = dy[n][c][r-u+K/2][j],   Q[v][(n,r,j)] = x[n][c][r][j+v-K/2]
// u and v padded to 32: one v_mfma_f32_32x32x16_bf16 tile (16 accumulators per lane) per 16 consecutive j of one input
// row.  The 5x5 branch has the same Q; its P comes from dy_small (rows u < 5, shifted by u - 2) into a second
// accumulator, and its taps are columns K/2-2 .. K/2+2 of that tile -- both gradients leave ONE launch that stages x once.
//   A operand (P): lane (u = l & 31, h = l >> 5) holds 8 consecutive j of one dy row: one 16-byte global load.
//   B operand (Q): the x row sits in LDS behind a zero halo; a lane's 8 values start at element j0 + 8h + v, which is
//                  only 2-byte aligned: five aligned dword reads and a per-lane 0- or 16-bit funnel shift.
// grid (C, S): a workgroup takes a band of (n, r) input rows, one row per wave and round (waves do not wait for each
// other: each stages its row in LDS of its own); its four waves' tiles are
// added in wave order through LDS and stored as part S of the caller's workspace; a second launch adds the parts in
// index order.  No floating-point atomics: the result is a bitwise function of the inputs.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int WAVES = 4;
constexpr int MAX_W = 4096;

inline bool lk_wgrad_served(int N, int C, int H, int W, int K, int KS) {
    return N > 0 && C > 0 && H > 0 && W > 0 && W <= MAX_W && (K == 31 || K == 29 || K == 27 || K == 13) &&
           (KS == 0 || KS == 5) && (long)N * H < (1L << 30);
}
// parts per channel: about 2048 workgroups in all, and at least one round of WAVES rows each
inline int lk_wgrad_parts(int N, int C, int H) {
    const long rows = (long)N * H;
    long s = (2048 + C - 1) / C;
    const long most = (rows + WAVES - 1) / WAVES;
    if (s > most) s = most;
    if (s < 1) s = 1;
    const long rpp = (rows + s - 1) / s;
    return (int)((rows + rpp - 1) / rpp);
}
inline int lk_wgrad_rows_per_part(int N, int C, int H) {
    const long rows = (long)N * H;
    const int s = lk_wgrad_parts(N, C, H);
    return (int)((rows + s - 1) / s);
}
__host__ __device__ inline int lk_row_elems(int W) { return ((W + 15) & ~15) + 40; }          // halo + row + the reach of the last fragment

// The host decisions of a launch (no device call): the launch goes by them and ppea_dwconv_lk_bwd_filter_plan reports them.
struct WgPlan { int parts, rows_per_part, rounds, vec, last_rows; size_t lds; };
inline WgPlan lk_wgrad_plan(int N, int C, int H, int W) {
    WgPlan p;
    p.parts = lk_wgrad_parts(N, C, H);
    p.rows_per_part = lk_wgrad_rows_per_part(N, C, H);
    p.rounds = (p.rows_per_part + WAVES - 1) / WAVES;                        // of a full part (the kernel's `rounds`)
    p.vec = (W & 7) == 0 ? 1 : 0;                                            // the kernel's `vec`
    p.last_rows = (int)((long)N * H - (long)(p.parts - 1) * p.rows_per_part);
    p.lds = (size_t)WAVES * lk_row_elems(W) * sizeof(uint16_t);
    return p;
}

__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// 8 bf16 of one dy row starting at column j (j % 8 == 0), zeros where the row or the columns are outside the plane
__device__ __forceinline__ uint4 load_dy8(const uint16_t* __restrict__ plane, int yr, int j, int H, int W, bool lane_ok,
                                          bool vec) {
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
    if (!lane_ok || yr < 0 || yr >= H || j >= W) return r;
    const uint16_t* p = plane + (long)yr * W + j;
    if (vec) return *reinterpret_cast<const uint4*>(p);                    // W % 8 == 0: all 8 inside, 16-byte aligned
    uint32_t e[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) e[i] = (j + i < W) ? (uint32_t)p[i] : 0u;
    return make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
}

__global__ __launch_bounds__(256) void dwconv_lk_bwd_filter_mfma(const uint16_t* __restrict__ x, const uint16_t* __restrict__ dyb,
                                                     const uint16_t* __restrict__ dys, float* __restrict__ ws, int N, int C,
                                                     int H, int W, int K, int KS, int rows_per_part) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];          // [WAVES][L / 2] x rows, then the reduce tile
    __shared__ float red[WAVES][32 * 32];
    const int c = blockIdx.x, part = blockIdx.y, parts = gridDim.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r32 = lane & 31, h = lane >> 5;
    const int HALF = K >> 1;
    const int L = lk_row_elems(W);
    uint16_t* row16 = reinterpret_cast<uint16_t*>(lds) + wave * L;
    const uint32_t* row32 = lds + wave * (L >> 1);
    const bool vec = (W & 7) == 0;
    const long rows = (long)N * H;
    const long r0 = (long)part * rows_per_part;
    long r1 = r0 + rows_per_part;
    if (r1 > rows) r1 = rows;
    const int rounds = (int)((r1 - r0 + WAVES - 1) / WAVES);
    const int Wp = (W + 15) & ~15;

    f32x16 accb, accs;
#pragma unroll
    for (int i = 0; i < 16; ++i) { accb[i] = 0.f; accs[i] = 0.f; }

    // A wave writes and reads only its own LDS row, and the LDS serves one wave's accesses in issue order: between staging a
    // row and reading it (and before the next row overwrites it) a wave-local fence is enough -- it keeps the compiler from
    // moving the 16-bit stores and the 32-bit loads across each other; the four waves run their rounds independently.
    for (int it = 0; it < rounds; ++it) {
        const long row = r0 + (long)it * WAVES + wave;
        if (row >= r1) break;                                              // (wave-uniform; no block barrier inside the loop)
        const int n = (int)(row / H), r = (int)(row % H);
        const long plane = ((long)n * C + c) * H * W;
        wave_fence();                                                      // the previous row's reads are issued
        const uint16_t* xr = x + plane + (long)r * W;
        for (int i = lane; i < L; i += 64) {
            const int j = i - HALF;
            row16[i] = (j >= 0 && j < W) ? xr[j] : (uint16_t)0;
        }
        wave_fence();
        const uint16_t* pb = dyb + plane;
        const uint16_t* ps = dys ? dys + plane : nullptr;
        const int yb = r - r32 + HALF, ys = r - r32 + 2;
        for (int j0 = 0; j0 < Wp; j0 += 16) {
            const int o = j0 + 8 * h + r32;                                // first element of this lane's Q fragment
            const uint32_t* q = row32 + (o >> 1);
            const uint32_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3], d4 = q[4];
            const uint32_t sh = (uint32_t)(o & 1) << 4;
            const uint4 bq = make_uint4(__builtin_amdgcn_alignbit(d1, d0, sh), __builtin_amdgcn_alignbit(d2, d1, sh),
                                        __builtin_amdgcn_alignbit(d3, d2, sh), __builtin_amdgcn_alignbit(d4, d3, sh));
            const bf16x8 bfrag = __builtin_bit_cast(bf16x8, bq);
            const uint4 ab = load_dy8(pb, yb, j0 + 8 * h, H, W, r32 < K, vec);
            accb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ab), bfrag, accb, 0, 0, 0);
            if (ps) {
                const uint4 as = load_dy8(ps, ys, j0 + 8 * h, H, W, r32 < 5, vec);
                accs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, as), bfrag, accs, 0, 0, 0);
            }
        }
    }

    // the four waves' tiles, added in wave order; C/D map: column v = lane & 31, row u = (reg & 3) + 8 (reg >> 2) + 4 h
    float* out = ws + ((long)c * parts + part) * (K * K + KS * KS);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) red[wave][((i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r32] = accb[i];
    __syncthreads();
    for (int i = threadIdx.x; i < K * K; i += 256) {
        const int t = (i / K) * 32 + (i % K);
        out[i] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    }
    if (KS) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i) red[wave][((i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r32] = accs[i];
        __syncthreads();
        if (threadIdx.x < 25) {
            const int t = (threadIdx.x / 5) * 32 + (threadIdx.x % 5) + HALF - 2;
            out[K * K + threadIdx.x] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
        }
    }
}

__global__ __launch_bounds__(256) void dwconv_lk_bwd_filter_sum(const float* __restrict__ ws, float* __restrict__ dwb,
                                                    float* __restrict__ dws, int C, int parts, int KK, int SS) {
    const int per = KK + SS;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)C * per) return;
    const int c = (int)(i / per), t = (int)(i % per);
    const float* p = ws + (long)c * parts * per + t;
    float s = 0.f;
    for (int k = 0; k < parts; ++k) s += p[(long)k * per];
    if (t < KK) dwb[(long)c * KK + t] = s;
    else dws[(long)c * SS + (t - KK)] = s;
}

}  // namespace

extern "C" {

// Both filter gradients of ReparamLargeKernelConv's depthwise pair from ONE launch over bf16 x / dy (fp32 accumulation on
// the matrix cores): dw_big [C,1,K,K], dw_small [C,1,KS,KS] fp32, overwritten.  K in {31, 29, 27, 13}, KS in {0, 5}
// (dy_small / dw_small NULL iff KS == 0), any N, C, H with N * H < 2^30, W <= 4096; otherwise PPEA_ERR_UNSUPPORTED (the _workspace_bytes
// function returns it too) and the caller keeps ppea_dwconv_lk_bwd_filter_f32.  `workspace`: device scratch of
// ppea_dwconv_lk_bwd_filter_workspace_bytes bytes for the per-part tiles, added in a fixed order by a second launch.
long ppea_dwconv_lk_bwd_filter_workspace_bytes(int N, int C, int H, int W, int K, int KS) {
    if (!lk_wgrad_served(N, C, H, W, K, KS)) return PPEA_ERR_UNSUPPORTED;
    return (long)C * lk_wgrad_parts(N, C, H) * (K * K + KS * KS) * (long)sizeof(float);
}
int ppea_dwconv_lk_bwd_filter_bf16(const uint16_t* x, const uint16_t* dy_big, const uint16_t* dy_small, float* dw_big,
                                   float* dw_small, void* workspace, int N, int C, int H, int W, int K, int KS,
                                   void* stream) {
    if (!lk_wgrad_served(N, C, H, W, K, KS)) return PPEA_ERR_UNSUPPORTED;
    if (x == nullptr || dy_big == nullptr || dw_big == nullptr || workspace == nullptr ||
        (KS != 0) != (dy_small != nullptr) || (KS != 0) != (dw_small != nullptr))
        return PPEA_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const WgPlan pl = lk_wgrad_plan(N, C, H, W);
    const int parts = pl.parts, rpp = pl.rows_per_part;
    const size_t smem = pl.lds;
    hipLaunchKernelGGL(dwconv_lk_bwd_filter_mfma, dim3((unsigned)C, (unsigned)parts), dim3(256), smem, st, x, dy_big, dy_small,
                       (float*)workspace, N, C, H, W, K, KS, rpp);
    const int r = launch_status();
    if (r != 0) return r;
    const long total = (long)C * (K * K + KS * KS);
    hipLaunchKernelGGL(dwconv_lk_bwd_filter_sum, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const float*)workspace,
                       dw_big, dw_small, C, parts, K * K, KS * KS);
    return launch_status();
}

// Host only: plan[0..5] = parts, rows_per_part, rounds (of a full part), vec (W % 8 == 0), dynamic LDS bytes, rows of the
// last part, as ppea_dwconv_lk_bwd_filter_bf16 launches; PPEA_ERR_UNSUPPORTED where that call returns it.
int ppea_dwconv_lk_bwd_filter_plan(int N, int C, int H, int W, int K, int KS, int* plan) {
    if (plan == nullptr) return PPEA_ERR_ARG;
    if (!lk_wgrad_served(N, C, H, W, K, KS)) return PPEA_ERR_UNSUPPORTED;
    const WgPlan pl = lk_wgrad_plan(N, C, H, W);
    plan[0] = pl.parts; plan[1] = pl.rows_per_part; plan[2] = pl.rounds; plan[3] = pl.vec; plan[4] = (int)pl.lds;
    plan[5] = pl.last_rows;
    return 0;
}

}  // extern "C"
