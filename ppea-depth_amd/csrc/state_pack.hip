// Pack / unpack of scattered state in ONE launch (checkpoints, dist.py): the mutable state of a training engine is three
// large flat buffers (parameters and the two Adam moments) and ~1 300 small tensors (BatchNorm running statistics and their
// int64 counters, the depth-bin tracker, the optimizer's step / learning-rate scalars).  Copying them one by one costs
// thousands of launches per checkpoint on the step stream; here a device table describes every tensor as a SEGMENT
// (pointer, byte offset in the packed buffer, byte count) and one launch copies all of them into one contiguous buffer,
// one launch copies them back.  Bytes only: no dtype, no conversion.
//
// The work is split by BYTE RANGE, not by segment: a workgroup copies one unit of PPEA_PACK_UNIT bytes of one segment, so
// a 1 GB segment and 1 300 scalars share the launch without one workgroup walking the large one.  table[s] =
// {pointer, packed offset, bytes, first unit}; a workgroup finds its segment by binary search over `first unit`
// (wave-uniform loads, 11 steps for 1 300 segments).
//
// Alignment: packed offsets are multiples of 16 and so is the unit, so the packed side of a unit is 16-byte aligned.  A
// segment pointer is aligned to its element size only (a view with a storage offset).  The copy width of a unit is the
// largest power of two <= 16 that divides the segment-side address -- then BOTH sides are aligned to it -- and the bytes
// past the last whole item are copied one by one.  Plain vector loads and stores only.
#include "common.h"

#define PPEA_PACK_UNIT 16384L
#define PPEA_PACK_THREADS 256

namespace {

template <typename T>
__device__ __forceinline__ void copy_run(const unsigned char* __restrict__ s, unsigned char* __restrict__ d, long n) {
    const long items = n / (long)sizeof(T);
    const T* s4 = reinterpret_cast<const T*>(s);
    T* d4 = reinterpret_cast<T*>(d);
    for (long i = threadIdx.x; i < items; i += PPEA_PACK_THREADS) d4[i] = s4[i];
    for (long i = items * (long)sizeof(T) + threadIdx.x; i < n; i += PPEA_PACK_THREADS) d[i] = s[i];   // < sizeof(T) bytes
}

template <bool UNPACK>
__global__ __launch_bounds__(PPEA_PACK_THREADS) void segments_kernel(const long* __restrict__ table, int nseg,
                                                                     unsigned char* packed) {
    const long unit = blockIdx.x;
    int lo = 0, hi = nseg - 1;                  // the LAST segment whose first unit is <= unit (empty segments own none)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[4 * (long)mid + 3] <= unit) lo = mid; else hi = mid - 1;
    }
    const long* e = table + 4 * (long)lo;
    const long at = (unit - e[3]) * PPEA_PACK_UNIT;
    long n = e[2] - at;
    if (n > PPEA_PACK_UNIT) n = PPEA_PACK_UNIT;
    if (n <= 0) return;
    unsigned char* seg = reinterpret_cast<unsigned char*>(e[0]) + at;
    unsigned char* pk = packed + e[1] + at;
    const unsigned char* s = UNPACK ? pk : seg;
    unsigned char* d = UNPACK ? seg : pk;
    const unsigned a = (unsigned)(reinterpret_cast<uintptr_t>(seg) & 15u);      // the packed side is 16-byte aligned
    if (a == 0) copy_run<uint4>(s, d, n);
    else if ((a & 7u) == 0) copy_run<uint2>(s, d, n);
    else if ((a & 3u) == 0) copy_run<uint32_t>(s, d, n);
    else if ((a & 1u) == 0) copy_run<uint16_t>(s, d, n);
    else copy_run<unsigned char>(s, d, n);
}

int launch(bool unpack, const void* table, int nseg, long units, void* packed, void* stream) {
    if (nseg <= 0 || units < 0 || units > 0x7fffffffL) return PPEA_ERR_UNSUPPORTED;
    if (table == nullptr || (packed == nullptr && units > 0)) return PPEA_ERR_ARG;
    if (units == 0) return 0;                   // only empty segments
    if (unpack)
        hipLaunchKernelGGL(segments_kernel<true>, dim3((unsigned)units), dim3(PPEA_PACK_THREADS), 0, (hipStream_t)stream,
                           (const long*)table, nseg, (unsigned char*)packed);
    else
        hipLaunchKernelGGL(segments_kernel<false>, dim3((unsigned)units), dim3(PPEA_PACK_THREADS), 0, (hipStream_t)stream,
                           (const long*)table, nseg, (unsigned char*)packed);
    return launch_status();
}

}  // namespace

extern "C" {

long ppea_pack_unit_bytes(void) { return PPEA_PACK_UNIT; }

int ppea_pack_segments(const void* table, int nseg, long units, void* packed, void* stream) {
    return launch(false, table, nseg, units, packed, stream);
}

int ppea_unpack_segments(const void* table, int nseg, long units, const void* packed, void* stream) {
    return launch(true, table, nseg, units, const_cast<void*>(packed), stream);
}

}  // extern "C"
