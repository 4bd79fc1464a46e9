// Run monitor: one row per training step, appended to a ring that lives on the device.
//
// A row holds up to 8 device scalars (losses, depth bins, learning rate) copied bit for bit, the L2 norm and the largest
// magnitude of the finite elements of the flat fp32 gradient buffer, the exact count of its non-finite elements, and the
// step.  The host enqueues the call after every step and reads the ring once per log interval: no step waits for a host
// read of a loss, and a run that has gone non-finite is noticed at the next log line (`first_bad_step` is sticky).
//
// TWO launches, stream order is the hand-off between them:
//   scan    grid-stride over the buffer, 16-byte loads on the aligned body, scalar loads on the <= 3 elements before and
//           after it; fp64 sum of squares, max |x| and the non-finite count per thread -> wave shuffles -> LDS -> ONE
//           partial (sum, max, count) per block in the caller's scratch;
//   finish  one block adds the partials in a fixed order and writes the row, the row counter and first_bad_step.
// No atomics and no in-launch hand-off: with the same input (and the same device) every call gives the same bits.
// Nothing is allocated here; ring, state and scratch belong to the caller (runlog.RunLog).
//
// Row layout, PPEA_MONITOR_ROW_WORDS = 16 32-bit words:
//   [0..7]  the scalars' bits (0 where absent)      [8] grad_l2 fp32      [9] grad_max_abs fp32
//   [10]    bit k set: scalar k present             [11] 0
//   [12,13] step int64                              [14,15] non-finite count int64
// State: int64 [2] = {rows appended so far, first_bad_step or -1}.
#include "common.h"

#define MON_THREADS 256
#define MON_ROW_WORDS 16
#define MON_MAX_SCALARS 8
#define MON_MAX_BLOCKS 2048

namespace {

struct MonScalars {
    const uint32_t* p[MON_MAX_SCALARS];
};

struct MonAcc {
    double sum;
    uint32_t max_bits;      // bits of max |x| over the finite elements: for non-negative floats the integer order is the float order
    uint32_t bad;
};

__device__ __forceinline__ void mon_take(MonAcc& a, float x) {
    const uint32_t bits = __float_as_uint(x) & 0x7fffffffu;
    if (bits >= 0x7f800000u) {              // Inf or NaN
        a.bad += 1u;
    } else {
        const double d = (double)x;
        a.sum += d * d;
        a.max_bits = bits > a.max_bits ? bits : a.max_bits;
    }
}

__device__ __forceinline__ void mon_take4(MonAcc& a, const float4& v) {
    mon_take(a, v.x);
    mon_take(a, v.y);
    mon_take(a, v.z);
    mon_take(a, v.w);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(v, o, WAVE);
        v = w > v ? w : v;
    }
    return v;
}

// Block reduction of (sum, max, count), each as fp64 (a count is exact below 2^53); the result is valid in thread 0.
__device__ __forceinline__ void block_reduce3(double& s, double& m, double& c) {
    __shared__ double lds[3][MON_THREADS / WAVE];
    s = wave_sum_f64(s);
    m = wave_max_f64(m);
    c = wave_sum_f64(c);
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    if (lane == 0) {
        lds[0][wave] = s;
        lds[1][wave] = m;
        lds[2][wave] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        s = lds[0][0];
        m = lds[1][0];
        c = lds[2][0];
        for (int w = 1; w < MON_THREADS / WAVE; ++w) {
            s += lds[0][w];
            m = lds[1][w] > m ? lds[1][w] : m;
            c += lds[2][w];
        }
    }
}

// g: fp32 [n], 4-byte aligned.  head = elements before the first 16-byte boundary (<= 3, <= n), n4 = float4 count of the
// body, the rest (<= 3) is the tail.  partial: fp64 [gridDim.x][3].
__global__ __launch_bounds__(MON_THREADS) void monitor_scan_kernel(const float* __restrict__ g, long n, long head, long n4,
                                                                   double* __restrict__ partial) {
    MonAcc a = {0.0, 0u, 0u};
    const float4* __restrict__ body = reinterpret_cast<const float4*>(g + head);
    const long stride = (long)gridDim.x * MON_THREADS;
    long i = (long)blockIdx.x * MON_THREADS + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {      // four independent 16-byte loads in flight per thread
        const float4 v0 = body[i], v1 = body[i + stride], v2 = body[i + 2 * stride], v3 = body[i + 3 * stride];
        mon_take4(a, v0);
        mon_take4(a, v1);
        mon_take4(a, v2);
        mon_take4(a, v3);
    }
    for (; i < n4; i += stride) mon_take4(a, body[i]);
    if (blockIdx.x == 0) {
        const long tail0 = head + 4 * n4, t = threadIdx.x;
        if (t < head) mon_take(a, g[t]);
        if (tail0 + t < n) mon_take(a, g[tail0 + t]);
    }
    double s = a.sum, m = (double)__uint_as_float(a.max_bits), c = (double)a.bad;
    block_reduce3(s, m, c);
    if (threadIdx.x == 0) {
        partial[3 * (long)blockIdx.x + 0] = s;
        partial[3 * (long)blockIdx.x + 1] = m;
        partial[3 * (long)blockIdx.x + 2] = c;
    }
}

__global__ __launch_bounds__(MON_THREADS) void monitor_finish_kernel(const double* __restrict__ partial, int nblocks,
                                                                     MonScalars sc, long step, float grad_scale,
                                                                     uint32_t* __restrict__ ring, int capacity,
                                                                     long long* __restrict__ state) {
    double s = 0.0, m = 0.0, c = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += MON_THREADS) {
        const double ps = partial[3 * (long)b], pm = partial[3 * (long)b + 1], pc = partial[3 * (long)b + 2];
        s += ps;
        m = pm > m ? pm : m;
        c += pc;
    }
    block_reduce3(s, m, c);
    if (threadIdx.x != 0) return;
    const long long count = state[0];
    uint32_t* row = ring + (long)(count % capacity) * MON_ROW_WORDS;
    uint32_t mask = 0u;
    bool bad = c > 0.0;
#pragma unroll
    for (int k = 0; k < MON_MAX_SCALARS; ++k) {
        uint32_t bits = 0u;
        if (sc.p[k] != nullptr) {
            bits = *sc.p[k];
            mask |= 1u << k;
            bad = bad || (bits & 0x7f800000u) == 0x7f800000u;
        }
        row[k] = bits;
    }
    // the product of two fp32 values is exact in fp64: one rounding to fp32 each
    row[8] = __float_as_uint((float)((double)grad_scale * sqrt(s)));
    row[9] = __float_as_uint((float)((double)grad_scale * m));
    row[10] = mask;
    row[11] = 0u;
    const long long bad_count = (long long)c;
    row[12] = (uint32_t)((unsigned long long)step & 0xffffffffull);
    row[13] = (uint32_t)((unsigned long long)step >> 32);
    row[14] = (uint32_t)((unsigned long long)bad_count & 0xffffffffull);
    row[15] = (uint32_t)((unsigned long long)bad_count >> 32);
    state[0] = count + 1;
    if (bad && state[1] < 0) state[1] = step;
}

int monitor_block_cap() {
    static int cap = 0;
    if (cap == 0) {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
        const long want = (long)cus * 8;
        cap = (int)(want < MON_MAX_BLOCKS ? want : MON_MAX_BLOCKS);
    }
    return cap;
}

}  // namespace

extern "C" {

int ppea_run_monitor_row_words(void) { return MON_ROW_WORDS; }

// The most blocks the scan launches on this device (8 per CU, at most 2048): scratch holds 3 fp64 per block.
int ppea_run_monitor_max_blocks(void) { return monitor_block_cap(); }

// scalars: HOST array of 8 device pointers to fp32 scalars (NULL = absent); they travel as kernel arguments.
// grads: fp32 [n] at any 4-byte aligned address (NULL or n == 0: no gradient columns, written as 0).
// scratch: fp64 [scratch_blocks][3], scratch_blocks >= ppea_run_monitor_max_blocks().
// ring: int32 [capacity][16]; state: int64 [2] = {rows appended, first_bad_step}, initialised by the caller to {0, -1}.
int ppea_run_monitor_f32(const void* const* scalars, const float* grads, long n, long step, float grad_scale,
                         double* scratch, int scratch_blocks, void* ring, int capacity, void* state, void* stream) {
    if (scalars == nullptr || ring == nullptr || state == nullptr || capacity <= 0 || n < 0) return PPEA_ERR_ARG;
    if (grads == nullptr) n = 0;
    if (((uintptr_t)grads & 3u) != 0) return PPEA_ERR_ARG;
    int blocks = 0;
    if (n > 0) {
        if (scratch == nullptr) return PPEA_ERR_ARG;
        long head = (long)(((16u - ((uintptr_t)grads & 15u)) & 15u) >> 2);
        if (head > n) head = n;
        const long n4 = (n - head) >> 2;
        long want = (n4 + MON_THREADS - 1) / MON_THREADS;
        if (want < 1) want = 1;
        const int cap = monitor_block_cap();
        blocks = (int)(want < cap ? want : cap);
        if (blocks > scratch_blocks) return PPEA_ERR_ARG;
        hipLaunchKernelGGL(monitor_scan_kernel, dim3((unsigned)blocks), dim3(MON_THREADS), 0, (hipStream_t)stream, grads, n,
                           head, n4, scratch);
        const int err = launch_status();
        if (err != 0) return err;
    }
    MonScalars sc;
    for (int k = 0; k < MON_MAX_SCALARS; ++k) sc.p[k] = (const uint32_t*)scalars[k];
    hipLaunchKernelGGL(monitor_finish_kernel, dim3(1), dim3(MON_THREADS), 0, (hipStream_t)stream, (const double*)scratch,
                       blocks, sc, step, grad_scale, (uint32_t*)ring, capacity, (long long*)state);
    return launch_status();
}

}  // extern "C"
