// Pointwise (1x1) convolution on the matrix cores, NCHW bf16 in / fp32 accumulate / bf16 out, gfx950.
// Replaces the 1x1 nn.Conv2d of RepLKBlock / ConvFFN / stem[2] / transitions[.][0]
// (networks/replknet_adapter.py:270-271, 296-297, 415, 452) in forward and, with the transposed
// weight matrix, their data gradients.
//
//     Y[n][m][p] = sum_k A[m][k] * X[n][k][p] (+ bias[m])        A = W [Cout][Cin]  (or W^T for dgrad)
//
// Per image a GEMM with the activation operand in its natural NCHW form: k (channel) is the SLOW axis
// of X, pixels are contiguous.  The tile of X is staged into LDS exactly as it lies in memory
// ([32 channels][128 pixels], coalesced 16-byte reads, no transposition) and the MFMA B fragments
// (8 consecutive k for one pixel) come out of `ds_read_b64_tr_b16`, the CDNA4 transposing LDS read.
//   * block = 4 waves, tile BM x 128 pixels, BK = 32; `v_mfma_f32_16x16x32_bf16`;
//   * A tile [BM][32] with a 96-byte row stride, B tile XOR-swizzled in 8-byte chunks: both fragment
//     reads are bank-conflict free (cdna_hip_programming.md 2, T10);
//   * global -> register prefetch of the next K-tile overlaps the MFMAs of the current one; LDS is
//     double buffered so a K step costs one barrier.
#include "gemm_bf16.h"
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace {

constexpr int BN = 128;
constexpr int B_STRIDE = 256;                   // bytes per B row (128 pixels), swizzled
// K step BK = 32 or 64 channels: the long-K, few-tile shapes of stage 2 are bound by the per-step barrier and
// load latency, not by MFMA issue -- twice the work per step halves that overhead.
constexpr int a_stride(int bk) { return bk == 32 ? 96 : 160; }   // bytes per A row in LDS: data + 32 (32 * odd)

__device__ __forceinline__ int b_swz(int row) { return 4 * (row & 3) + 16 * ((row >> 3) & 1); }

// ---- epilogue values: one accumulator quad (4 consecutive pixels of one channel) -> the packed bf16 pairs both kernels store
// EPI 0: Y = acc + bias.   EPI 1: Y = pre = acc + bias, Y2 = GELU(pre) (pre rounded to bf16 first, like an
// autocast nn.GELU on the stored tensor).   EPI 2: Y = acc * GELU'(aux[n][m][p]) (data gradient through GELU).
// EPI 4: as EPI 0, and per-channel partial sums (sum, sum of squares) of the values AS STORED, per pixel-wave of the
// workgroup, into (float*)Y2 [M][B * pixel tiles * WN][2] -- the BatchNorm that follows needs no statistics pass.
struct PwQuad { uint2 y, y2; };
struct Bf16x4 { uint16_t v[4]; };
__device__ __forceinline__ Bf16x4 unpack4(uint2 a) {
    return {{(uint16_t)(a.x & 0xffffu), (uint16_t)(a.x >> 16), (uint16_t)(a.y & 0xffffu), (uint16_t)(a.y >> 16)}};
}

// `aux`: the quad's four bf16 of aux (EPI 2);  `count`: the quad lies inside the plane and joins the statistics (EPI 4).
// The form is the one hipcc compiles like the code spelled out in each kernel: the quad by value and the dwords packed here (with
// uint16_t[4] results handed back by reference every value is converted alone, twice the v_cvt_pk_bf16_f32); GELU of the stored
// values in a loop of its own (inside the first, the 128-row v1 kernels take 4 more VGPRs).
template <int EPI>
__device__ __forceinline__ PwQuad pw_values(f32x4 acc, float bv, uint2 aux, bool count, float& st_s, float& st_q) {
    uint16_t e[4], f[4] = {0, 0, 0, 0};
    if constexpr (EPI == 2) {
        const Bf16x4 x = unpack4(aux);
#pragma unroll
        for (int r = 0; r < 4; ++r) e[r] = f2bf(acc[r] * dgelu_f(bf2f(x.v[r])));
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            e[r] = f2bf(acc[r] + bv);
            if constexpr (EPI == 4) {
                if (count) { const float t = bf2f(e[r]); st_s += t; st_q += t * t; }
            }
        }
        if constexpr (EPI == 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) f[r] = f2bf(gelu_f(bf2f(e[r])));
        }
    }
    return {make_uint2(e[0] | ((uint32_t)e[1] << 16), e[2] | ((uint32_t)e[3] << 16)),
            make_uint2(f[0] | ((uint32_t)f[1] << 16), f[2] | ((uint32_t)f[3] << 16))};
}

// the bias of channel m (fp32 or bf16; none: 0)
__device__ __forceinline__ float pw_bias(const void* bias, int bias_bf16, int m) {
    if (bias == nullptr) return 0.f;
    return bias_bf16 ? bf2f(reinterpret_cast<const uint16_t*>(bias)[m]) : reinterpret_cast<const float*>(bias)[m];
}

// EPI 4: the four lane groups g hold the other pixels of channel m -- fixed-order butterfly, lane group 0 writes partial
// `part + wn` of P; channel-major [M][P][2]: the finalize kernel reads a channel's P partials as one contiguous run
__device__ __forceinline__ void pw_store_stats(float* stats, float st_s, float st_q, bool writer, int m, long P, long part, int wn) {
    st_s += __shfl_xor(st_s, 16, WAVE); st_q += __shfl_xor(st_q, 16, WAVE);
    st_s += __shfl_xor(st_s, 32, WAVE); st_q += __shfl_xor(st_q, 32, WAVE);
    if (writer) {
        float* sp = stats + ((long)m * P + part + wn) * 2;
        sp[0] = st_s; sp[1] = st_q;
    }
}

// v1: register prefetch into a double-buffered LDS tile.
// TA: the matrix is given transposed, At [K][M] (m contiguous) -- its tile is staged like the X tile and the A
// fragments come out of the transposing LDS read as well, so a data gradient uses the forward weight as is.
template <int BM, int WM, int WN, int EPI, bool TA, int BK>
__global__ __launch_bounds__(256) void pwconv_kernel(const uint16_t* __restrict__ A, const uint16_t* __restrict__ X,
                                                     const void* __restrict__ bias, int bias_bf16,
                                                     const uint16_t* __restrict__ aux, uint16_t* __restrict__ Y,
                                                     uint16_t* __restrict__ Y2, int M, int K, int HW) {
    static_assert(WM * WN == 4, "four waves");
    constexpr int TM = BM / WM, TN = BN / WN, MT = TM / 16, NT = TN / 16;
    constexpr int A_STRIDE = a_stride(BK), KH = BK / 32;
    constexpr int A_BYTES = TA ? BK * B_STRIDE : BM * A_STRIDE, B_BYTES = BK * B_STRIDE;
    constexpr int A_CH = (BM * BK / 8 + 255) / 256;  // 16-byte chunks of the A tile per thread
    constexpr int A_CPR = TA ? BM / 8 : BK / 8;      // chunks per staged row: [BK k][BM m] or [BM m][BK k]
    constexpr int B_CH = BK * 16 / 256;              // 16-byte chunks of the X tile per thread
    constexpr int BUF = A_BYTES + B_BYTES;
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * BUF];      // double buffered: one barrier per K step

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int p0 = blockIdx.x * BN, m0 = blockIdx.y * BM, n = blockIdx.z;
    const uint16_t* Xn = X + (long)n * K * HW;

    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

    // per-thread staging coordinates
    int a_row[A_CH], a_ch[A_CH];
#pragma unroll
    for (int c = 0; c < A_CH; ++c) { const int idx = tid + c * 256; a_row[c] = idx / A_CPR; a_ch[c] = idx % A_CPR; }
    int b_row[B_CH], b_c16[B_CH];
#pragma unroll
    for (int c = 0; c < B_CH; ++c) { const int idx = tid + c * 256; b_row[c] = idx >> 4; b_c16[c] = idx & 15; }

    uint4 a_reg[A_CH], b_reg[B_CH];
    auto load_tiles = [&](int k0) {
#pragma unroll
        for (int c = 0; c < A_CH; ++c) {
            if constexpr (TA) {
                const int m = m0 + a_ch[c] * 8;
                a_reg[c] = (m < M && a_row[c] < BK && k0 + a_row[c] < K)
                               ? *reinterpret_cast<const uint4*>(A + (long)(k0 + a_row[c]) * M + m) : make_uint4(0, 0, 0, 0);
            } else {
                const int m = m0 + a_row[c];
                a_reg[c] = (m < M && a_row[c] < BM && k0 + a_ch[c] * 8 < K)
                               ? *reinterpret_cast<const uint4*>(A + (long)m * K + k0 + a_ch[c] * 8) : make_uint4(0, 0, 0, 0);
            }
        }
#pragma unroll
        for (int c = 0; c < B_CH; ++c) {
            const int p = p0 + b_c16[c] * 8;
            b_reg[c] = (p < HW && k0 + b_row[c] < K) ? *reinterpret_cast<const uint4*>(Xn + (long)(k0 + b_row[c]) * HW + p)
                                                     : make_uint4(0, 0, 0, 0);
        }
    };
    auto store_tiles = [&](uint8_t* As) {
        uint8_t* Bs = As + A_BYTES;
#pragma unroll
        for (int c = 0; c < A_CH; ++c) {
            if constexpr (TA) {
                if (a_row[c] < BK) {
                    const int s = b_swz(a_row[c]);
                    uint8_t* rowp = As + a_row[c] * B_STRIDE;
                    // the swizzle is a multiple of 4 chunks: the two 8-byte halves stay adjacent -> one 16-byte store
                    *reinterpret_cast<uint4*>(rowp + (((2 * a_ch[c]) ^ s) << 3)) = a_reg[c];
                }
            } else {
                if (a_row[c] < BM) *reinterpret_cast<uint4*>(As + a_row[c] * A_STRIDE + a_ch[c] * 16) = a_reg[c];
            }
        }
#pragma unroll
        for (int c = 0; c < B_CH; ++c) {
            const int s = b_swz(b_row[c]);
            uint8_t* rowp = Bs + b_row[c] * B_STRIDE;
            *reinterpret_cast<uint4*>(rowp + (((2 * b_c16[c]) ^ s) << 3)) = b_reg[c];
        }
    };

    // fragment offsets inside a buffer
    const int g = lane >> 4, li = lane & 15, q = li >> 2, pp = li & 3;
    const int b_rowi = 8 * g + q;
    const int a_off = TA ? b_rowi * B_STRIDE : (wm * TM + li) * A_STRIDE + g * 16;
    const int b_off = A_BYTES + b_rowi * B_STRIDE;
    const int b_s = b_swz(b_rowi);

    load_tiles(0);
    store_tiles(lds);
    __syncthreads();
    int cur = 0;
    for (int k0 = 0; k0 < K; k0 += BK) {
        const bool more = k0 + BK < K;
        if (more) load_tiles(k0 + BK);            // in flight while the MFMAs of this step run
        const uint8_t* buf = lds + cur * BUF;
#pragma unroll
        for (int h = 0; h < KH; ++h) {                    // 32-wide halves of the K step
            bf16x8 af[MT], bfr[NT];
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                if constexpr (TA) {
                    const int chunk = (((wm * TM + 16 * i) >> 2) + pp) ^ b_swz(b_rowi);
                    af[i] = tr_frag(buf + a_off + h * 32 * B_STRIDE + (chunk << 3), B_STRIDE);
                } else {
                    af[i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(buf + a_off + i * 16 * A_STRIDE + h * 64));
                }
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int chunk = (((wn * TN + 16 * j) >> 2) + pp) ^ b_s;
                bfr[j] = tr_frag(buf + b_off + h * 32 * B_STRIDE + (chunk << 3), B_STRIDE);
            }
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    // operands swapped (the two fragment layouts are the same registers): the accumulator holds the
                    // TRANSPOSED tile -- a lane owns 4 consecutive pixels of one output channel = one 8-byte store
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
        }
        if (more) store_tiles(lds + (cur ^ 1) * BUF);   // the other buffer was last read one barrier ago
        __syncthreads();
        cur ^= 1;
    }

    // epilogue: transposed C layout -- col = lane & 15 = output channel, row = 4 * (lane >> 4) + r = pixel
    // (HW % 8 == 0 and the four pixels start at a multiple of 4: all inside the plane or all outside)
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int m = m0 + wm * TM + 16 * i + li;
        if (m >= M) continue;
        const float bv = pw_bias(bias, bias_bf16, m);
        float st_s = 0.f, st_q = 0.f;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int p = p0 + wn * TN + 16 * j + 4 * g;
            if (p >= HW) continue;
            const long o = (long)n * M * HW + (long)m * HW + p;
            uint2 a = make_uint2(0, 0);
            if constexpr (EPI == 2) a = *reinterpret_cast<const uint2*>(aux + o);
            const PwQuad v = pw_values<EPI>(acc[i][j], bv, a, true, st_s, st_q);
            if constexpr (EPI == 1) *reinterpret_cast<uint2*>(Y2 + o) = v.y2;
            *reinterpret_cast<uint2*>(Y + o) = v.y;
        }
        if constexpr (EPI == 4)
            pw_store_stats(reinterpret_cast<float*>(Y2), st_s, st_q, g == 0, m, (long)gridDim.z * gridDim.x * WN,
                           ((long)n * gridDim.x + blockIdx.x) * WN, wn);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// v2: the same GEMM on the three-stage LDS-DMA ring of gemm_bf16.h (one raw barrier per K step, two K tiles in flight
// across it), an XCD-aware tile order and 16-byte epilogue stores.
//   * both tiles are dense images with the swizzle on the SOURCE address:
//       X tile [BK k][128 pixels] (256-byte rows): 16-byte slot s of row r holds pixel chunk s ^ (2 (r & 3) + 8 ((r >> 3) & 1))
//         -- the 8-byte swizzle of v1, which is a multiple of two 8-byte chunks; read with `ds_read_b64_tr_b16`;
//       A tile [BM m][BK k] (128- / 64-byte rows): swz16<BK>, read with `ds_read_b128`.
//   * epilogue: `v_permlane16_swap` between the packed results of two neighbouring 16-pixel tiles gives every lane 8
//     consecutive pixels of one channel: one 16-byte store instead of two 8-byte ones (a wave writes 64 contiguous bytes
//     per channel row).
//   * TA (the matrix given transposed, At [K][M]: data gradients use the forward weight as is): with BM = 128 the A tile
//     [BK k][128 m] has the X tile's shape, so it is staged with the X tile's source swizzle and its fragments come out of
//     the same transposing read -- the adapters' data gradients ran 17-22 us on v1's transposed mode against 5-9 us for
//     the same GEMM with a row-major matrix.
// Requirements: K % BK == 0, HW % 8 == 0; TA: BM = 128, M % 8 == 0.

// EPI 5 (inference, eval-mode BatchNorm folded to a per-channel table; ppea_pwconv_infer_bf16):
//     t = act(s[m] * acc + o[m])   Y = t (+ r1) (+ r2_scale * r2)   Y2 = s2[m] * Y + o2[m]  (Y as stored; Y2 optional)
// Its arguments ride in a trailing kernel parameter that is an empty struct for every other epilogue.
struct PwInfer {
    const float* s; const float* o; const uint16_t* r1; const uint16_t* r2; float r2_scale;
    const float* s2; const float* o2; int act;
};
template <int EPI> struct PwExtra {};
template <> struct PwExtra<5> { PwInfer v; };

// this lane's channel of the tables (s, o: 1, 0 where absent; s2, o2 only with a second output), then pw_values' shape
struct PwInferLane { float sc = 1.f, sh = 0.f, sc2 = 0.f, sh2 = 0.f; };
__device__ __forceinline__ PwQuad pw_infer_values(f32x4 acc, const PwInferLane& t, uint2 r1, uint2 r2, const PwInfer& ex) {
    const Bf16x4 x1 = unpack4(r1), x2 = unpack4(r2);
    uint16_t e[4], f[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float v = fmaf(t.sc, acc[r], t.sh);
        if (ex.act == 1) v = fmaxf(v, 0.f);
        else if (ex.act == 2) v = gelu_f(v);
        v += bf2f(x1.v[r]);
        v = fmaf(ex.r2_scale, bf2f(x2.v[r]), v);
        e[r] = f2bf(v);
        f[r] = f2bf(fmaf(t.sc2, bf2f(e[r]), t.sh2));          // the next block's pre-BN of the tensor as stored
    }
    return {make_uint2(e[0] | ((uint32_t)e[1] << 16), e[2] | ((uint32_t)e[3] << 16)),
            make_uint2(f[0] | ((uint32_t)f[1] << 16), f[2] | ((uint32_t)f[3] << 16))};
}

template <int BM, int BK, int EPI, bool TA = false>
__global__ __launch_bounds__(256) void pwconv2_kernel(const uint16_t* __restrict__ A, const uint16_t* __restrict__ X,
                                                      const void* __restrict__ bias, int bias_bf16,
                                                      const uint16_t* __restrict__ aux, uint16_t* __restrict__ Y,
                                                      uint16_t* __restrict__ Y2, int M, int K, int HW, int nb, int mtiles,
                                                      int total, PwExtra<EPI> ex = {}) {
    constexpr int WM = BM >= 64 ? 2 : 1, WN = 4 / WM;
    constexpr int TM = BM / WM, TN = BN / WN, MT = TM / 16, NT = TN / 16;
    static_assert(!TA || BM == 128, "the transposed-A tile reuses the X tile's 256-byte-row layout");
    constexpr int ARB = BK * 2;                          // bytes per A row
    constexpr int A_BYTES = BM * ARB, X_BYTES = BK * B_STRIDE, STAGE = A_BYTES + X_BYTES;
    constexpr int A_INS = A_BYTES / 1024 / 4, X_INS = X_BYTES / 1024 / 4;      // LDS-DMA instructions per wave and stage
    static_assert(A_BYTES % 4096 == 0 && X_BYTES % 4096 == 0, "every wave issues the same number of loads per stage");
    constexpr int LPS = A_INS + X_INS, KH = BK / 32;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];

    // XCD-aware order: consecutive workgroup ids go round-robin over the 8 XCDs (each with its own L2); give every XCD a
    // contiguous run of logical tiles, channel tiles fastest, so the workgroups that share an X tile share an L2
    const int id = blockIdx.x, xcd = id & 7, q8 = total >> 3, r8 = total & 7;
    const int L = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (id >> 3);
    const int mt_i = L % mtiles, pt = L / mtiles;
    const int n = pt / nb, p0 = (pt - n * nb) * BN, m0 = mt_i * BM;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const uint16_t* Xn = X + (long)n * K * HW;

    // ---- LDS-DMA source addresses (per lane; advanced by BK channels per stage) and destinations (wave uniform) ----------
    const uint16_t* a_src[A_INS];
    const uint16_t* x_src[X_INS];
#pragma unroll
    for (int c = 0; c < A_INS; ++c) {
        const int t = c * 4 + wave;                              // 1-KiB piece of the A tile
        if constexpr (TA) {                                      // [BK k][128 m]: the X tile's layout and source swizzle
            const int row = 4 * t + (lane >> 4), slot = lane & 15;
            int m = m0 + 8 * (slot ^ (2 * (row & 3) + 8 * ((row >> 3) & 1)));
            if (m >= M) m = m0;                                  // chunks past M: any valid chunk (not stored; M % 8 == 0)
            a_src[c] = A + (long)row * M + m;
        } else {
            const int row = t * (1024 / ARB) + lane / (ARB / 16), slot = lane % (ARB / 16);
            const int m = min(m0 + row, M - 1);                  // rows past M: any valid row (their outputs are not stored)
            a_src[c] = A + (long)m * K + 8 * (slot ^ swz16<BK>(row));
        }
    }
#pragma unroll
    for (int c = 0; c < X_INS; ++c) {
        const int t = c * 4 + wave;
        const int row = 4 * t + (lane >> 4), slot = lane & 15;
        int p = p0 + 8 * (slot ^ (2 * (row & 3) + 8 * ((row >> 3) & 1)));
        if (p >= HW) p = p0;                                     // chunks past the plane: any valid chunk (not stored)
        x_src[c] = Xn + (long)row * HW + p;
    }
    const unsigned lds_base = lds_address(lds);
    auto issue = [&](int kt, int stage) {
        const unsigned base = __builtin_amdgcn_readfirstlane(lds_base + stage * STAGE + wave * 1024);
        const long ka = TA ? (long)kt * BK * M : (long)kt * BK, kx = (long)kt * BK * HW;
#pragma unroll
        for (int c = 0; c < A_INS; ++c) glds16(a_src[c] + ka, base + c * 4096);
#pragma unroll
        for (int c = 0; c < X_INS; ++c) glds16(x_src[c] + kx, base + A_BYTES + c * 4096);
    };

    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

    // fragment read offsets inside a stage
    const int g = lane >> 4, li = lane & 15, q = li >> 2, pp = li & 3;
    const int b_rowi = 8 * g + q, b_s = b_swz(b_rowi);
    int a_off[MT][KH];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int h = 0; h < KH; ++h) {
            const int row = wm * TM + 16 * i + li;
            a_off[i][h] = row * ARB + 16 * ((4 * h + g) ^ swz16<BK>(row));
        }
    const int x_off = A_BYTES + b_rowi * B_STRIDE;

    const int nk = K / BK;
    issue(0, 0);
    if (nk > 1) issue(1, 1);
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        ring_wait<LPS>(kt + 1 < nk);
        if (kt + 2 < nk) issue(kt + 2, ring_refill(cur));
        const uint8_t* buf = lds + cur * STAGE;
#pragma unroll
        for (int h = 0; h < KH; ++h) {
            bf16x8 af[MT], bfr[NT];
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                if constexpr (TA) {
                    const int chunk = (((wm * TM + 16 * i) >> 2) + pp) ^ b_s;
                    af[i] = tr_frag(buf + b_rowi * B_STRIDE + h * 32 * B_STRIDE + (chunk << 3), B_STRIDE);
                } else {
                    af[i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(buf + a_off[i][h]));
                }
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int chunk = (((wn * TN + 16 * j) >> 2) + pp) ^ b_s;
                bfr[j] = tr_frag(buf + x_off + h * 32 * B_STRIDE + (chunk << 3), B_STRIDE);
            }
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
        }
        cur = ring_next(cur);
    }

    // ---- epilogue: transposed C layout (col = lane & 15 = channel, rows 4 g + r = pixels); pairs of pixel tiles exchange
    // halves so that a lane stores 8 consecutive pixels
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int m = m0 + wm * TM + 16 * i + li;
        const bool m_ok = m < M;
        const float bv = m_ok ? pw_bias(bias, bias_bf16, m) : 0.f;
        float st_s = 0.f, st_q = 0.f;
        uint2 v[NT], w[NT];
        PwInferLane tab;
        if constexpr (EPI == 5) {
            if (m_ok) {
                if (ex.v.s != nullptr) tab.sc = ex.v.s[m];
                if (ex.v.o != nullptr) tab.sh = ex.v.o[m];
                if (Y2 != nullptr) { tab.sc2 = ex.v.s2[m]; tab.sh2 = ex.v.o2[m]; }
            }
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int p = p0 + wn * TN + 16 * j + 4 * g;
            const bool ok = m_ok && p < HW;
            const long o = (long)n * M * HW + (long)m * HW + p;
            uint2 a = make_uint2(0, 0), a2 = make_uint2(0, 0);      // aux (EPI 2) / r1, r2 (EPI 5): absent or outside = 0
            PwQuad r;
            if constexpr (EPI == 5) {
                if (ok && ex.v.r1 != nullptr) a = *reinterpret_cast<const uint2*>(ex.v.r1 + o);
                if (ok && ex.v.r2 != nullptr) a2 = *reinterpret_cast<const uint2*>(ex.v.r2 + o);
                r = pw_infer_values(acc[i][j], tab, a, a2, ex.v);
            } else {
                if constexpr (EPI == 2) {
                    if (ok) a = *reinterpret_cast<const uint2*>(aux + o);
                }
                r = pw_values<EPI>(acc[i][j], bv, a, ok, st_s, st_q);
            }
            v[j] = r.y; w[j] = r.y2;
        }
#pragma unroll
        for (int j = 0; j < NT; j += 2) {
            // rows 1 / 3 of tile j <-> rows 0 / 2 of tile j + 1: lane group g then holds pixels 8 (g >> 1) .. + 7 of tile
            // j + (g & 1), the first four in the tile-j register, the next four in the tile-(j + 1) register
            auto sx = __builtin_amdgcn_permlane16_swap(v[j].x, v[j + 1].x, false, false);
            auto sy = __builtin_amdgcn_permlane16_swap(v[j].y, v[j + 1].y, false, false);
            const int p = p0 + wn * TN + 16 * (j + (g & 1)) + 8 * (g >> 1);
            const long o = (long)n * M * HW + (long)m * HW + p;
            if (m_ok && p < HW) *reinterpret_cast<uint4*>(Y + o) = make_uint4(sx[0], sy[0], sx[1], sy[1]);
            if constexpr (EPI == 1 || EPI == 5) {
                auto tx = __builtin_amdgcn_permlane16_swap(w[j].x, w[j + 1].x, false, false);
                auto ty = __builtin_amdgcn_permlane16_swap(w[j].y, w[j + 1].y, false, false);
                if (m_ok && p < HW && (EPI == 1 || Y2 != nullptr))
                    *reinterpret_cast<uint4*>(Y2 + o) = make_uint4(tx[0], ty[0], tx[1], ty[1]);
            }
        }
        if constexpr (EPI == 4)
            pw_store_stats(reinterpret_cast<float*>(Y2), st_s, st_q, g == 0 && m_ok, m, (long)(total / mtiles) * WN, (long)pt * WN, wn);
    }
}

// ---- dispatch ----------------------------------------------------------------------------------------------------------
// One place decides the kernel and its tile: the statistics epilogue writes one partial per pixel-wave (WN), and
// ppea_pwconv_stats_partials must size that buffer for the kernel that will run.
struct PwCfg { int v2, bm, bk, wn; };

// `force` / `v2env`: the values of PPEA_PW_TILE / PPEA_PW_V2 (pw_choose reads them per call; the plan sweep reads them once).
PwCfg pw_choose_env(int B, int M, int K, int HW, bool ta, const char* force, const char* v2env) {
    const int nb = (HW + BN - 1) / BN;
    const long blocks128 = (long)nb * ((M + 127) / 128) * B, blocks64 = (long)nb * ((M + 63) / 64) * B;
    PwCfg c;
    const bool v2off = v2env != nullptr && v2env[0] == '0' && v2env[1] == 0;
    if (force != nullptr) {
        c.bm = atoi(force) == 128 ? 128 : (atoi(force) == 64 ? 64 : 32);
        c.bk = (c.bm != 128 && strchr(force, 'd') != nullptr) ? 64 : 32;      // v1 has no 128-row tile with 64-channel steps
    } else {
        c.bm = (M >= 128 && blocks128 >= 512) ? 128 : ((M > 32 && blocks64 >= 256) ? 64 : 32);
        // 64 channels per step only where it pays (measured on v1): long contraction AND too few tiles to hide the
        // per-step latency by occupancy
        c.bk = (c.bm != 128 && K >= 512) ? 64 : 32;
    }
    c.v2 = 0;
    if (!ta && !v2off) {
        // measured per trunk shape (tools/bench_pw4.py, profiles/r03_pwconv_shapes.txt): enough 128-row tiles to fill the
        // chip once -> 128 x 128 tiles with 32-channel steps (48 KB of LDS: three workgroups per CU hide each other's
        // barriers); else 64-row tiles (64-channel steps for long contractions); else 32-row tiles with 64-channel steps
        int bm, bk;
        if (M >= 128 && blocks128 >= 256) { bm = 128; bk = 32; }
        else if (M > 32 && blocks64 >= 256) { bm = 64; bk = (K >= 512 && K % 64 == 0) ? 64 : 32; }
        else if (K % 64 == 0) { bm = 32; bk = 64; }
        else { bm = 64; bk = 32; }
        if (v2env != nullptr && strchr(v2env, ',') != nullptr) { bm = atoi(v2env); bk = atoi(strchr(v2env, ',') + 1); }
        if (bm == 32 && bk == 32) bk = 64;                       // a 32 x 32 A tile is half a piece per wave
        if ((bm == 128 || bm == 64 || bm == 32) && (bk == 64 || bk == 32) && K % bk == 0) { c.v2 = 1; c.bm = bm; c.bk = bk; }
    }
    if (ta) {
        // transposed matrix on the LDS-DMA ring: 128-row tiles only (see pwconv2_kernel); PPEA_PW_V2=0 keeps v1
        static const bool ta_v2 = !(getenv("PPEA_PW_TA_V2") != nullptr && getenv("PPEA_PW_TA_V2")[0] == '0');
        // ... where they give at least ~128 workgroups: a 128-channel result on 12 x 40 maps is 48 tiles with a long
        // contraction each, and v1's 32-row tiles (192 workgroups) are faster there (10 against 18 us, tools/bench_pw_ta.py)
        if (ta_v2 && !v2off && M >= 128 && blocks128 >= 128 && (M % 8) == 0 && (K % 32) == 0) { c.v2 = 1; c.bm = 128; c.bk = 32; }
    }
    c.wn = c.bm == 32 ? 4 : 2;
    return c;
}

PwCfg pw_choose(int B, int M, int K, int HW, bool ta) {
    // tuning / test hooks, read per call so that a test can walk the tiles in one process
    return pw_choose_env(B, M, K, HW, ta, getenv("PPEA_PW_TILE"),  // v1 tile: "128", "64", "32" [+ "d" = 64-channel steps]
                         getenv("PPEA_PW_V2"));                    // "0": v1 everywhere; "bm,bk": force a v2 tile
}

// the shape checks of every entry point of this file (and of ppea_pwconv_plan)
bool pw_served(int B, int M, int K, int HW, bool ta) {
    if (B <= 0 || M <= 0 || K <= 0 || HW <= 0 || (K % 32) != 0 || (HW % 8) != 0 || B > 65535) return false;
    return !(ta && (M % 8) != 0);
}

// plan[0..7] of ppea_pwconv_plan for a served shape
void pw_plan_of(const PwCfg& c, int B, int M, int HW, int* plan) {
    const int nb = (HW + BN - 1) / BN, mt = (M + c.bm - 1) / c.bm;
    plan[0] = c.v2 ? 2 : 1; plan[1] = c.bm; plan[2] = c.bk; plan[3] = c.wn;
    if (c.v2) { plan[4] = nb * mt * B; plan[5] = 1; plan[6] = 1; }
    else { plan[4] = nb; plan[5] = mt; plan[6] = B; }
    plan[7] = B * nb * c.wn;
}

template <int BM, int BK, int EPI, bool TA = false>
int launch_pw2_t(const void* A, const void* X, const void* bias, int bias_bf16, const void* aux, void* Y, void* Y2, int B,
                 int M, int K, int HW, hipStream_t st, PwExtra<EPI> ex = {}) {
    constexpr int smem = NSTAGE * (BM * BK * 2 + BK * B_STRIDE);
    static bool ready = false;                                   // per instantiation
    auto kern = pwconv2_kernel<BM, BK, EPI, TA>;
    if (!ready) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
        if (e != hipSuccess) return (int)e;
        ready = true;
    }
    const int nb = (HW + BN - 1) / BN, mtiles = (M + BM - 1) / BM;
    const long total = (long)nb * mtiles * B;
    if (total > 0x7fffffffL) return PPEA_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(kern, dim3((unsigned)total), dim3(256), smem, st, (const uint16_t*)A, (const uint16_t*)X, bias, bias_bf16,
                       (const uint16_t*)aux, (uint16_t*)Y, (uint16_t*)Y2, M, K, HW, nb, mtiles, (int)total, ex);
    return launch_status();
}

// THE tile dispatch: f(BM, BK), as integral constants, for the tile of `c`.  v2 has 128/64, 128/32, 64/64, 64/32 and 32/64;
// v1 has no 128-row tile with 64-channel steps, and has 32/32.
template <bool V2, class F>
int pw_tile(const PwCfg& c, F&& f) {
    typedef std::integral_constant<int, 32> i32;
    typedef std::integral_constant<int, 64> i64;
    typedef std::integral_constant<int, 128> i128;
    if (c.bm == 128) {
        if constexpr (V2) { if (c.bk == 64) return f(i128{}, i64{}); }
        return f(i128{}, i32{});
    }
    if (c.bm == 64) return c.bk == 64 ? f(i64{}, i64{}) : f(i64{}, i32{});
    if constexpr (!V2) { if (c.bk != 64) return f(i32{}, i32{}); }
    return f(i32{}, i64{});
}

template <int EPI, bool TA>
int launch_pw(const void* A, const void* X, const void* bias, int bias_bf16, const void* aux, void* Y, void* Y2, int B,
              int M, int K, int HW, hipStream_t st) {
    const PwCfg c = pw_choose(B, M, K, HW, TA);
    if (c.v2) {
        if constexpr (TA) return launch_pw2_t<128, 32, EPI, true>(A, X, bias, bias_bf16, aux, Y, Y2, B, M, K, HW, st);
        else return pw_tile<true>(c, [&](auto bm, auto bk) {
            return launch_pw2_t<decltype(bm)::value, decltype(bk)::value, EPI>(A, X, bias, bias_bf16, aux, Y, Y2, B, M, K, HW, st);
        });
    }
    return pw_tile<false>(c, [&](auto bm, auto bk) {
        constexpr int BM = decltype(bm)::value, WM = BM >= 64 ? 2 : 1;
        hipLaunchKernelGGL((pwconv_kernel<BM, WM, 4 / WM, EPI, TA, decltype(bk)::value>), dim3((HW + BN - 1) / BN, (M + BM - 1) / BM, B),
                           dim3(256), 0, st, (const uint16_t*)A, (const uint16_t*)X, bias, bias_bf16, (const uint16_t*)aux,
                           (uint16_t*)Y, (uint16_t*)Y2, M, K, HW);
        return launch_status();
    });
}

// ppea_pwconv_bf16 / _stats_bf16 / _ex_bf16: the shape check, then the (epilogue, A mode) instantiation
int pw_run(int epi, bool ta, const void* A, const void* X, const void* bias, int bias_bf16, const void* aux, void* Y, void* Y2,
           int B, int M, int K, int HW, void* stream) {
    if (!pw_served(B, M, K, HW, ta)) return PPEA_ERR_UNSUPPORTED;
    if ((epi == 1 || epi == 4) && !Y2) return PPEA_ERR_ARG;
    if (epi == 2 && !aux) return PPEA_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    auto go = [&](auto e, auto t) {
        constexpr int EPI = decltype(e)::value;
        return launch_pw<EPI, decltype(t)::value>(A, X, EPI == 2 ? nullptr : bias, EPI == 2 ? 0 : bias_bf16, EPI == 2 ? aux : nullptr, Y,
                                                  (EPI == 1 || EPI == 4) ? Y2 : nullptr, B, M, K, HW, st);
    };
    using std::integral_constant;
    switch (ta ? epi + 8 : epi) {
        case 0: return go(integral_constant<int, 0>{}, std::false_type{});
        case 1: return go(integral_constant<int, 1>{}, std::false_type{});
        case 2: return go(integral_constant<int, 2>{}, std::false_type{});
        case 4: return go(integral_constant<int, 4>{}, std::false_type{});
        case 8: return go(integral_constant<int, 0>{}, std::true_type{});
        case 9: return go(integral_constant<int, 1>{}, std::true_type{});
        case 10: return go(integral_constant<int, 2>{}, std::true_type{});
    }
    return PPEA_ERR_ARG;
}

}  // namespace

extern "C" {

// A [M][K] bf16 row-major (k contiguous); X [B][K][HW] bf16; Y [B][M][HW] bf16; bias [M] fp32 or NULL.
// Requirements of the fast path: K % 32 == 0, HW % 8 == 0 (else PPEA_ERR_UNSUPPORTED).
int ppea_pwconv_bf16(const void* A, const void* X, const float* bias, void* Y, int B, int M, int K, int HW,
                     void* stream) {
    return pw_run(0, false, A, X, bias, 0, nullptr, Y, nullptr, B, M, K, HW, stream);
}

// ppea_pwconv_bf16 plus the statistics of the BatchNorm that follows (conv_bn / conv_bn_relu, rka.py:182-197): per output
// channel the sum and the sum of squares of the stored bf16 values, as P = ppea_pwconv_stats_partials(B, M, K, HW) partial
// pairs, stats [M][P][2] fp32 (every entry written; reduce with ppea_bn_finalize_sums_f32).
static int stats_partials_env(int B, int M, int K, int HW, const char* force, const char* v2env) {
    if (B <= 0 || M <= 0 || K <= 0 || HW <= 0) return 0;
    return B * ((HW + BN - 1) / BN) * pw_choose_env(B, M, K, HW, false, force, v2env).wn;
}
int ppea_pwconv_stats_partials(int B, int M, int K, int HW) {
    return stats_partials_env(B, M, K, HW, getenv("PPEA_PW_TILE"), getenv("PPEA_PW_V2"));
}
int ppea_pwconv_stats_bf16(const void* A, const void* X, const float* bias, void* Y, float* stats, int B, int M, int K,
                           int HW, void* stream) {
    return pw_run(4, false, A, X, bias, 0, nullptr, Y, stats, B, M, K, HW, stream);
}

// Host only: what ppea_pwconv_bf16 / _stats_bf16 / _ex_bf16 / _infer_bf16 launch for these arguments, answered by pw_choose
// (the function launch_pw goes by).  plan[0..7] = version (1: pwconv_kernel, 2: pwconv2_kernel), BM, BK, WN, grid x, y, z,
// statistics partials P.  PPEA_ERR_UNSUPPORTED exactly where the entry points return it for their shape arguments.
int ppea_pwconv_plan(int B, int M, int K, int HW, int a_transposed, int* plan) {
    if (plan == nullptr) return PPEA_ERR_ARG;
    if (!pw_served(B, M, K, HW, a_transposed != 0)) return PPEA_ERR_UNSUPPORTED;
    const PwCfg c = pw_choose(B, M, K, HW, a_transposed != 0);
    if (c.v2 && (long)((HW + BN - 1) / BN) * ((M + c.bm - 1) / c.bm) * B > 0x7fffffffL) return PPEA_ERR_UNSUPPORTED;
    pw_plan_of(c, B, M, HW, plan);
    return 0;
}

// Test support, host only: ppea_pwconv_plan for one B and A mode over M = Mstep * (1..nM) x K = 32 * (1..nK) x
// HW = 8 * (1..nHW), one byte per shape in out[nM][nK][nHW]: bit 0 v2, bits 1-2 BM (0: 32, 1: 64, 2: 128), bit 3 BK = 64;
// 0xff: not served.  summary[0] = shapes served, [1] = row-major shapes whose ppea_pwconv_stats_partials differs from
// plan[7].  The hooks are read once for the whole sweep.
int ppea_pwconv_plan_sweep(int B, int a_transposed, int Mstep, int nM, int nK, int nHW, unsigned char* out, long* summary) {
    if (out == nullptr || summary == nullptr || Mstep <= 0) return PPEA_ERR_ARG;
    const char* force = getenv("PPEA_PW_TILE");
    const char* v2env = getenv("PPEA_PW_V2");
    const bool ta = a_transposed != 0;
    summary[0] = summary[1] = 0;
    long i = 0;
    for (int im = 1; im <= nM; ++im)
        for (int ik = 1; ik <= nK; ++ik)
            for (int ip = 1; ip <= nHW; ++ip, ++i) {
                const int M = im * Mstep, K = 32 * ik, HW = 8 * ip;
                if (!pw_served(B, M, K, HW, ta)) { out[i] = 0xff; continue; }
                const PwCfg c = pw_choose_env(B, M, K, HW, ta, force, v2env);
                int plan[8];
                pw_plan_of(c, B, M, HW, plan);
                out[i] = (unsigned char)(c.v2 | ((c.bm == 128 ? 2 : (c.bm == 64 ? 1 : 0)) << 1) | ((c.bk == 64) << 3));
                summary[0]++;
                if (!ta && stats_partials_env(B, M, K, HW, force, v2env) != plan[7]) summary[1]++;
            }
    return 0;
}

// Same GEMM with an epilogue (adapters, replknet_adapter.py:20-109): epi 0 plain; epi 1 writes the
// pre-activation to Y and GELU(pre) to Y2; epi 2 multiplies by GELU'(aux) (aux, Y: [B][M][HW] bf16).
// `bias` is fp32 or, with bias_bf16 != 0, bf16.  a_transposed != 0: A is given as At [K][M] (M % 8 == 0).
int ppea_pwconv_ex_bf16(const void* A, const void* X, const void* bias, int bias_bf16, int epi, const void* aux,
                        void* Y, void* Y2, int B, int M, int K, int HW, int a_transposed, void* stream) {
    return pw_run(epi >= 0 && epi <= 2 ? epi : -1, a_transposed != 0, A, X, bias, bias_bf16, aux, Y, Y2, B, M, K, HW, stream);
}

// Inference form of the 1x1 conv + BatchNorm (+ activation, residual, adapter add, next block's first BatchNorm) of the
// trunk (replknet_adapter.py:270-326 in eval mode): the BatchNorm is a per-channel table (s, o) applied to the fp32
// accumulator, so the weights stay the training model's bf16 matrices.
//   t = act(s[m] * (A X)[m][p] + o[m])   act: 0 none, 1 ReLU, 2 GELU (erf);  s NULL = 1, o NULL = 0
//   Y = t (+ r1[b][m][p]) (+ r2_scale * r2[b][m][p])                          r1 / r2 [B][M][HW] bf16 or NULL
//   Y2 = s2[m] * Y + o2[m]   (of Y as stored in bf16)                         Y2 NULL: not written
// Served by the LDS-DMA kernel only: K % 32 == 0, HW % 8 == 0, else PPEA_ERR_UNSUPPORTED.
int ppea_pwconv_infer_bf16(const void* A, const void* X, const float* s, const float* o, int act, const void* r1,
                           const void* r2, float r2_scale, const float* s2, const float* o2, void* Y, void* Y2, int B, int M,
                           int K, int HW, void* stream) {
    if (!pw_served(B, M, K, HW, false)) return PPEA_ERR_UNSUPPORTED;
    if (A == nullptr || X == nullptr || Y == nullptr || act < 0 || act > 2) return PPEA_ERR_ARG;
    if (Y2 != nullptr && (s2 == nullptr || o2 == nullptr)) return PPEA_ERR_ARG;
    const PwCfg c = pw_choose(B, M, K, HW, false);
    if (!c.v2) return PPEA_ERR_UNSUPPORTED;
    PwExtra<5> ex;
    ex.v = PwInfer{s, o, (const uint16_t*)r1, (const uint16_t*)r2, r2_scale, s2, o2, act};
    hipStream_t st = (hipStream_t)stream;
    return pw_tile<true>(c, [&](auto bm, auto bk) {
        return launch_pw2_t<decltype(bm)::value, decltype(bk)::value, 5>(A, X, nullptr, 0, nullptr, Y, Y2, B, M, K, HW, st, ex);
    });
}

}  // extern "C"
