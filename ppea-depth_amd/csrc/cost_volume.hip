// Plane-sweep matching cost volume, gfx950 (replk_matching_adapter.py:261-340, 372-387, 446-456).
//
// The reference repeats each lookup feature map 96x ([96,128,48,160] = 377 MB per item and frame), warps it with
// grid_sample, subtracts, reduces -- per batch item and lookup frame, in Python loops.  Here ONE kernel, cost_volume_fwd,
// computes, for every (item, depth bin, pixel), the projected sample position in each of the F = 1 .. 4 lookup frames
// analytically and reduces |warp(lookup) - cur| over channels on the fly: nothing but the [B,D,h,w] cost leaves the chip
// (10.8 MB/img algorithmic).  It serves fp32 features and bf16 features packed as channel pairs
// (cv_pack_pairs); one lookup frame is its F = 1 instantiation.  A second kernel, cost_volume_reduce, does the per-pixel
// work over the bin axis (missing -> max, confidence, argmin, lowest-cost depth).
#include "common.h"

namespace {

// cost = (sum over the frames f that contribute of diff_f) / (#{f: diff_f > 0} + 1e-7), diff_f the masked mean
// |warp_f(lookup_f) - cur| of frame f (rkm.py:289-326); for F = 1 that is diff / ((diff > 0) + 1e-7).
//
// One thread = one pixel x DB consecutive depth bins x all F frames, channel loop outermost.  The kernel is bound by
// vector-memory instruction issue (gathers that hit L1 / L2: a lookup map is 3.9 MB per item), not by bytes, so the loads
// are what is economised: the current frame's feature depends on neither the bin nor the frame and is read once per channel
// for all F * DB samples, and two horizontally adjacent corners of a bilinear footprint are one 8-byte load (Pair: the
// address is only 4-byte aligned, x0 being any column, which gfx950 global loads allow) -- (1 + 2 * F * DB) / (F * DB)
// = 2.25 loads per (pixel, bin, frame, channel) at four samples per thread instead of 5.  The F single-frame volumes
// never exist.  The F * DB sums stay apart until the epilogue (the count needs each frame's own diff); they are added in
// frame order in fp32, as the reference's `cost_volume + diffs` does.  Same arithmetic, in the same order, for every DB
// (pinned bit for bit by test_cost_volume_golden's argmin and by tests/golden/cost_volume_f1_bits.npz).
//
// PK: the features are bf16 channel PAIRS (cv_pack_pairs), one dword = channels 2c, 2c + 1 at one position; CE = C / 2
// elements per position.  The bytes that cross the L1 (64 B / clk / CU: 4 bilinear corners per pixel, bin and channel; the
// neighbouring lanes' footprints overlap, the cache lines are fetched once but delivered per lane) are halved: a corner
// load serves two channels.  The arithmetic is the fp32 form's on the widened values, channel by channel in the same
// order: bit-identical to PK = false on `feature.float()`.
__device__ __forceinline__ float lo_f(uint32_t v) { return __uint_as_float(v << 16); }
__device__ __forceinline__ float hi_f(uint32_t v) { return __uint_as_float(v & 0xffff0000u); }
template <bool PK> struct CvFeat { using T = float; };
template <> struct CvFeat<true> { using T = uint32_t; };
template <typename T> struct alignas(4) Pair { T a, b; };

template <bool PK, typename T>
__device__ __forceinline__ void cv_accum(double& acc, T v00, T v01, T v10, T v11, float w00, float w01, float w10,
                                         float w11, T cv) {
    if constexpr (PK) {
        const float wa = ((lo_f(v00) * w00 + lo_f(v01) * w01) + lo_f(v10) * w10) + lo_f(v11) * w11;
        acc += (double)fabsf(wa - lo_f(cv));
        const float wb = ((hi_f(v00) * w00 + hi_f(v01) * w01) + hi_f(v10) * w10) + hi_f(v11) * w11;
        acc += (double)fabsf(wb - hi_f(cv));
    } else {
        const float warped = ((v00 * w00 + v01 * w01) + v10 * w10) + v11 * w11;
        acc += (double)fabsf(warped - cv);
    }
}

// Head slot of a feature / pose ring of F slots from the device-side stream state (state[0]; state[1 + b]: frames item b
// has seen since its reset, clamped at F).  Brought into 0 .. F - 1 whatever the word holds: it becomes an address.
__device__ __forceinline__ int ring_head(const int32_t* __restrict__ state, int F) {
    const int hd = state[0] % F;
    return hd < 0 ? hd + F : hd;
}

// RING: `lookup` is a ring [F][B][CE][hw] of the last F frames' features and frame f of item b is slot (head - 1 - f) mod F
// (video streaming: the newest frame sits just behind the head); the frame is skipped where seen[b] <= f, or-ed with the
// zero-pose flag skip[b][f] (NULL: none).  Otherwise `lookup` is [B][F][CE][hw].  Only where a frame's map starts differs:
// a block-uniform address per frame, found once before the channel loop.
template <int F, int DB, bool PK, bool RING>
__global__ __launch_bounds__(256) void cost_volume_fwd(const typename CvFeat<PK>::T* __restrict__ cur,
                                                       const typename CvFeat<PK>::T* __restrict__ lookup,
                                                       const float* __restrict__ P,       // [B][F][3][4]
                                                       const float* __restrict__ inv_K,
                                                       const float* __restrict__ bins,
                                                       const int32_t* __restrict__ skip,  // [B][F]
                                                       const int32_t* __restrict__ state, // RING: [1 + B]
                                                       float* __restrict__ cost, int C, int h, int w, int D,
                                                       float eps) {
    using T = typename CvFeat<PK>::T;
    const int b = blockIdx.z, d0 = blockIdx.y * DB;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int hw = h * w, CE = PK ? (C >> 1) : C;
    if (i >= hw) return;
    float* outp = cost + ((long)b * D + d0) * hw + i;
    const int nd = min(DB, D - d0);
    const int py = i / w, px = i - py * w;
    const T* fb[F];                                    // frame f's map of item b; same in every lane, like fskip and any
    bool fskip[F];
    bool any = false;
#pragma unroll
    for (int f = 0; f < F; ++f) {
        if constexpr (RING) {
            int slot = ring_head(state, F) - 1 - f;
            if (slot < 0) slot += F;
            fb[f] = lookup + ((long)slot * gridDim.z + b) * CE * hw;
            fskip[f] = state[1 + b] <= f || (skip != nullptr && skip[b * F + f] != 0);
        } else {
            fb[f] = lookup + ((long)b * F + f) * CE * hw;
            fskip[f] = skip[b * F + f] != 0;
        }
        any = any || !fskip[f];
    }
    if (!any || px < 2 || px >= w - 2 || py < 2 || py >= h - 2) {
        for (int k = 0; k < nd; ++k) outp[(long)k * hw] = 0.f;
        return;
    }
    const float* ik = inv_K + b * 16;
    const float fx = (float)px, fy = (float)py;
    float ray[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) ray[k] = (ik[k * 4] * fx + ik[k * 4 + 1] * fy) + ik[k * 4 + 2];
    const T* cu = cur + (long)b * CE * hw + i;
    // off: y0 * w + x0 of the footprint's top-left corner; -1: the sample adds nothing (frame skipped or outside the edge
    // mask); -2: resolved below, its diff is in w00
    int off[F][DB];
    float w00[F][DB], w01[F][DB], w10[F][DB], w11[F][DB];
#pragma unroll
    for (int f = 0; f < F; ++f) {
        const float* pm = P + ((long)b * F + f) * 12;
#pragma unroll
        for (int k = 0; k < DB; ++k) {
            off[f][k] = -1;
            w00[f][k] = w01[f][k] = w10[f][k] = w11[f][k] = 0.f;
            if (fskip[f] || k >= nd) continue;
            const float depth = bins[d0 + k];
            float X[3], cam[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) X[q] = depth * ray[q];
#pragma unroll
            for (int q = 0; q < 3; ++q)
                cam[q] = ((pm[q * 4] * X[0] + pm[q * 4 + 1] * X[1]) + pm[q * 4 + 2] * X[2]) + pm[q * 4 + 3];
            const float iz = cam[2] + eps;
            const float gx = ((cam[0] / iz) / (float)(w - 1) - 0.5f) * 2.f;
            const float gy = ((cam[1] / iz) / (float)(h - 1) - 0.5f) * 2.f;
            const float xv = (gx / 2.f + 0.5f) * (float)(w - 1);
            const float yv = (gy / 2.f + 0.5f) * (float)(h - 1);
            if (!(xv >= 2.0f && xv <= (float)(w - 2) && yv >= 2.0f && yv <= (float)(h - 2))) continue;
            const float ix = ((gx + 1.f) / 2.f) * (float)(w - 1);
            const float iy = ((gy + 1.f) / 2.f) * (float)(h - 1);
            const float flx = floorf(ix), fly = floorf(iy);
            const int x0 = (int)flx, y0 = (int)fly;
            const float tx = ix - flx, ty = iy - fly;
            w00[f][k] = (1.f - tx) * (1.f - ty); w01[f][k] = tx * (1.f - ty); w10[f][k] = (1.f - tx) * ty; w11[f][k] = tx * ty;
            off[f][k] = y0 * w + x0;
            if (!(x0 + 1 < w && y0 + 1 < h)) {
                // The footprint touches the last column / row: corner by corner with zero fill, as grid_sample does.  Not
                // reached by finite inputs: xv <= w - 2 and ix >= w - 1 are two roundings of (gx + 1) / 2 * (w - 1) that
                // differ by a few ulps of w, never by 1 (tests/test_cv_arms_cpu.py counts it over every row and a pose sweep:
                // 0; DESIGN.md, "Several lookup frames").  Kept: it is what makes the 8-byte loads below safe by construction.
                const T* lk = fb[f] + off[f][k];
                double acc = 0.0;
                for (int c = 0; c < CE; ++c) {
                    const T* l = lk + (long)c * hw;
                    const T v01 = (x0 + 1 < w) ? l[1] : (T)0;
                    const T v10 = (y0 + 1 < h) ? l[w] : (T)0;
                    cv_accum<PK, T>(acc, l[0], v01, v10, (T)0, w00[f][k], w01[f][k], w10[f][k], w11[f][k], cu[(long)c * hw]);
                }
                w00[f][k] = (float)(acc / (double)C);
                off[f][k] = -2;
            }
        }
    }
    double acc[F][DB];
#pragma unroll
    for (int f = 0; f < F; ++f)
#pragma unroll
        for (int k = 0; k < DB; ++k) acc[f][k] = 0.0;
    for (int c = 0; c < CE; ++c) {
        const T cv = cu[(long)c * hw];
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const T* lc = fb[f] + (long)c * hw;
#pragma unroll
            for (int k = 0; k < DB; ++k) {
                if (off[f][k] < 0) continue;
                const Pair<T> top = *reinterpret_cast<const Pair<T>*>(lc + off[f][k]);
                const Pair<T> bot = *reinterpret_cast<const Pair<T>*>(lc + off[f][k] + w);
                cv_accum<PK, T>(acc[f][k], top.a, top.b, bot.a, bot.b, w00[f][k], w01[f][k], w10[f][k], w11[f][k], cv);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < DB; ++k) {
        if (k >= nd) continue;
        float sum = 0.f, count = 0.f;
#pragma unroll
        for (int f = 0; f < F; ++f) {
            if (off[f][k] == -1) continue;
            const float diff = off[f][k] == -2 ? w00[f][k] : (float)(acc[f][k] / (double)C);
            sum = sum + diff;
            count += diff > 0.f ? 1.f : 0.f;
        }
        outp[(long)k * hw] = sum / (count + 1e-7f);          // average over the frames that saw the point (:323-326)
    }
}

// (1 + F) maps [n][2 * C2][hw] bf16 -> channel-pair dwords [n][C2][hw]: the current frame's, then the lookups'
__global__ __launch_bounds__(256) void cv_pack_pairs(const uint16_t* __restrict__ cur, const uint16_t* __restrict__ look,
                                                     uint32_t* __restrict__ out, int C2, int hw, long n_cur, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;      // over (B + B * F) * C/2 * hw
    if (i >= total) return;
    const uint16_t* src = i < n_cur ? cur : look;
    const long j = i < n_cur ? i : i - n_cur;
    const long p = j % hw, c2 = (j / hw) % C2, n = j / ((long)hw * C2);
    const long s = (n * 2 * C2 + 2 * c2) * hw + p;
    out[i] = (uint32_t)src[s] | ((uint32_t)src[s + hw] << 16);
}

// One map [B][CE (x2 for PK)][hw] -> slot `head` of a ring [F][B][CE][hw] (state == NULL: slot 0 of a plain buffer); PK:
// bf16 source, written as the channel-pair dwords of cv_pack_pairs.  n = B * CE * hw elements per slot.
template <bool PK>
__global__ __launch_bounds__(256) void cv_ring_store(const void* __restrict__ src, void* __restrict__ dst,
                                                     const int32_t* __restrict__ state, int F, int CE, int hw, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long base = state == nullptr ? 0 : (long)ring_head(state, F) * n;
    if constexpr (PK) {
        const uint16_t* s16 = (const uint16_t*)src;
        const long p = i % hw, c2 = (i / hw) % CE, nb = i / ((long)hw * CE);
        const long s = (nb * 2 * CE + 2 * c2) * hw + p;
        ((uint32_t*)dst)[base + i] = (uint32_t)s16[s] | ((uint32_t)s16[s + hw] << 16);
    } else {
        ((float*)dst)[base + i] = ((const float*)src)[i];
    }
}

// thread 0: the head; thread 1 + b: item b's count of frames seen.  Every thread owns its word.  The count is clamped
// before the increment: a word of INT_MAX must come out as F, not overflow.
__global__ void cv_ring_advance(int32_t* __restrict__ state, int B, int F) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > B) return;
    state[i] = i == 0 ? (ring_head(state, F) + 1) % F : min(max(state[i], 0), F - 1) + 1;
}

// Bins per thread for F lookup frames: the F * DB samples of a thread each hold a double sum, an offset and four weights.
// 3 - 4 samples per thread keep the kernel at 8 waves / SIMD (<= 62 VGPRs), where one frame with DB = 4 was measured best
// ("Several lookup frames": registers and occupancy per F and DB).
template <bool PK, bool RING, typename T>
int cost_volume_launch(const T* cur, const T* lookup, const float* P, const float* inv_K, const float* bins,
                       const int32_t* skip, const int32_t* state, float* cost, int B, int F, int C, int h, int w, int D,
                       float eps, hipStream_t stream) {
#define CV_LAUNCH(F_, DB_)                                                                                           \
    hipLaunchKernelGGL((cost_volume_fwd<F_, DB_, PK, RING>), dim3((h * w + 255) / 256, (D + DB_ - 1) / DB_, B),       \
                       dim3(256), 0, stream, cur, lookup, P, inv_K, bins, skip, state, cost, C, h, w, D, eps)
    if (F == 1) CV_LAUNCH(1, 4); else if (F == 2) CV_LAUNCH(2, 2); else if (F == 3) CV_LAUNCH(3, 1); else CV_LAUNCH(4, 1);
#undef CV_LAUNCH
    return launch_status();
}

__global__ __launch_bounds__(256) void cost_volume_reduce(const float* __restrict__ cost,
                                                          const float* __restrict__ bins,
                                                          float* __restrict__ cost_out,
                                                          float* __restrict__ confidence,
                                                          int64_t* __restrict__ argmin,
                                                          float* __restrict__ lowest, int D, int hw) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hw) return;
    const float* cp = cost + (long)b * D * hw + i;
    float mx = -INFINITY;
    bool all_pos = true;
    for (int d = 0; d < D; ++d) {
        const float v = cp[(long)d * hw];
        mx = fmaxf(mx, v);
        all_pos = all_pos && (v > 0.f);
    }
    const float conf = all_pos ? 1.f : 0.f;
    float best = INFINITY;
    int bi = 0;
    float* op = cost_out + (long)b * D * hw + i;
    for (int d = 0; d < D; ++d) {
        const float v = cp[(long)d * hw];
        const float miss = (v == 0.f) ? 1.f : 0.f;
        const float filled = v * (1.f - miss) + mx * miss;
        const float viz = (filled == 0.f) ? 100.f : filled;
        if (viz < best) { best = viz; bi = d; }
        op[(long)d * hw] = filled * conf;
    }
    confidence[(long)b * hw + i] = conf;
    argmin[(long)b * hw + i] = bi;
    lowest[(long)b * hw + i] = 1.f / bins[bi];
}

}  // namespace

extern "C" {

// F = 1 .. 4 lookup frames in one launch: lookup [B][F][C][h][w], P [B][F][3][4], skip [B][F].
int ppea_cost_volume_multi_fwd_f32(const float* cur, const float* lookup, const float* P, const float* inv_K,
                                   const float* bins, const int32_t* skip, float* cost, int B, int F, int C, int h, int w,
                                   int D, float eps, void* stream) {
    if (B < 0 || B > 65535 || F < 1 || F > 4 || C <= 0 || h < 5 || w < 5 || D <= 0 || D > 65535) return PPEA_ERR_UNSUPPORTED;
    if (B == 0) return 0;
    if (!cur || !lookup || !P || !inv_K || !bins || !skip || !cost) return PPEA_ERR_ARG;
    return cost_volume_launch<false, false>(cur, lookup, P, inv_K, bins, skip, nullptr, cost, B, F, C, h, w, D, eps,
                                            (hipStream_t)stream);
}

// bf16 features (C even); `pairs`: caller-owned workspace of (1 + F) * B * C/2 * h * w uint32 (= the inputs' bytes).
// Same result, bit for bit, as ppea_cost_volume_multi_fwd_f32 on the features widened to fp32.
int ppea_cost_volume_multi_fwd_bf16(const void* cur, const void* lookup, void* pairs, const float* P, const float* inv_K,
                                    const float* bins, const int32_t* skip, float* cost, int B, int F, int C, int h, int w,
                                    int D, float eps, void* stream) {
    if (B < 0 || B > 65535 || F < 1 || F > 4 || C <= 0 || (C & 1) || h < 5 || w < 5 || D <= 0 || D > 65535)
        return PPEA_ERR_UNSUPPORTED;
    if (B == 0) return 0;
    if (!cur || !lookup || !pairs || !P || !inv_K || !bins || !skip || !cost) return PPEA_ERR_ARG;
    const long n = (long)B * (C / 2) * h * w;
    uint32_t* pc = (uint32_t*)pairs;
    hipLaunchKernelGGL(cv_pack_pairs, dim3((unsigned)((n * (1 + F) + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t*)cur, (const uint16_t*)lookup, pc, C / 2, h * w, n, n * (1 + F));
    return cost_volume_launch<true, false>((const uint32_t*)pc, (const uint32_t*)(pc + n), P, inv_K, bins, skip, nullptr,
                                           cost, B, F, C, h, w, D, eps, (hipStream_t)stream);
}

// Video streaming: the lookups are the last F frames in a device ring [F][B][C][h][w] (bf16: channel-pair dwords
// [F][B][C/2][h][w], as is `cur` [B][C/2][h][w]: ppea_cv_ring_store_bf16 writes both), frame f = slot (head - 1 - f) mod F.
// state [1 + B] int32 on the device: head, then per item the frames seen since its reset; frame f of item b is skipped where
// seen[b] <= f or skip[b][f] != 0 (skip may be NULL).  Same kernel and bits as the entries above on the gathered frames.
int ppea_cost_volume_ring_fwd_f32(const float* cur, const float* ring, const int32_t* state, const float* P,
                                  const float* inv_K, const float* bins, const int32_t* skip, float* cost, int B, int F,
                                  int C, int h, int w, int D, float eps, void* stream) {
    if (B < 0 || B > 65535 || F < 1 || F > 4 || C <= 0 || h < 5 || w < 5 || D <= 0 || D > 65535) return PPEA_ERR_UNSUPPORTED;
    if (B == 0) return 0;
    if (!cur || !ring || !state || !P || !inv_K || !bins || !cost) return PPEA_ERR_ARG;
    return cost_volume_launch<false, true>(cur, ring, P, inv_K, bins, skip, state, cost, B, F, C, h, w, D, eps,
                                           (hipStream_t)stream);
}

int ppea_cost_volume_ring_fwd_bf16(const void* cur_pairs, const void* ring_pairs, const int32_t* state, const float* P,
                                   const float* inv_K, const float* bins, const int32_t* skip, float* cost, int B, int F,
                                   int C, int h, int w, int D, float eps, void* stream) {
    if (B < 0 || B > 65535 || F < 1 || F > 4 || C <= 0 || (C & 1) || h < 5 || w < 5 || D <= 0 || D > 65535)
        return PPEA_ERR_UNSUPPORTED;
    if (B == 0) return 0;
    if (!cur_pairs || !ring_pairs || !state || !P || !inv_K || !bins || !cost) return PPEA_ERR_ARG;
    return cost_volume_launch<true, true>((const uint32_t*)cur_pairs, (const uint32_t*)ring_pairs, P, inv_K, bins, skip,
                                          state, cost, B, F, C, h, w, D, eps, (hipStream_t)stream);
}

// One feature map [B][C][h][w] into the slot the device-side head names of a ring [F][B][C][h][w] (bf16: as channel-pair
// dwords into [F][B][C/2][h][w], C even).  state NULL: `dst` is a plain [B][..] buffer (the current frame's packed feature).
int ppea_cv_ring_store_f32(const float* src, float* dst, const int32_t* state, int B, int F, int C, int h, int w,
                           void* stream) {
    if (B < 0 || F < 1 || F > 4 || C <= 0 || h <= 0 || w <= 0) return PPEA_ERR_UNSUPPORTED;
    if (B == 0) return 0;
    if (!src || !dst) return PPEA_ERR_ARG;
    const long n = (long)B * C * h * w;
    hipLaunchKernelGGL(cv_ring_store<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const void*)src, (void*)dst, state, F, C, h * w, n);
    return launch_status();
}

int ppea_cv_ring_store_bf16(const void* src, void* dst, const int32_t* state, int B, int F, int C, int h, int w,
                            void* stream) {
    if (B < 0 || F < 1 || F > 4 || C <= 0 || (C & 1) || h <= 0 || w <= 0) return PPEA_ERR_UNSUPPORTED;
    if (B == 0) return 0;
    if (!src || !dst) return PPEA_ERR_ARG;
    const long n = (long)B * (C / 2) * h * w;
    hipLaunchKernelGGL(cv_ring_store<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, dst,
                       state, F, C / 2, h * w, n);
    return launch_status();
}

// A frame has been pushed: head <- (head + 1) mod F, seen[b] <- min(seen[b] + 1, F).  Stream-ordered after the sweep that
// read the slot the store overwrote.
int ppea_cv_ring_advance(int32_t* state, int B, int F, void* stream) {
    if (B < 0 || F < 1 || F > 4) return PPEA_ERR_UNSUPPORTED;
    if (!state) return PPEA_ERR_ARG;
    hipLaunchKernelGGL(cv_ring_advance, dim3((B + 1 + 63) / 64), dim3(64), 0, (hipStream_t)stream, state, B, F);
    return launch_status();
}

int ppea_cost_volume_reduce_f32(const float* cost, const float* bins, float* cost_out, float* confidence,
                                int64_t* argmin, float* lowest, int B, int D, int h, int w, void* stream) {
    if (B < 0 || B > 65535 || D <= 0 || h <= 0 || w <= 0) return PPEA_ERR_UNSUPPORTED;      // B is gridDim.y
    if (B == 0) return 0;
    dim3 g((h * w + 255) / 256, B);
    hipLaunchKernelGGL(cost_volume_reduce, g, dim3(256), 0, (hipStream_t)stream, cost, bins, cost_out,
                       confidence, argmin, lowest, D, h * w);
    return launch_status();
}

}  // extern "C"
