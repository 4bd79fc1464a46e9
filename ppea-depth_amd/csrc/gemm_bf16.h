// What the bf16 MFMA GEMM kernels (pwconv.hip, pwgrad.hip) share: the fragment types, the transposing fragment read and the
// three-stage LDS ring filled by LDS-DMA.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;

// One MFMA fragment (8 consecutive k of this lane's row) out of a tile staged k-major, [k][row] with `row_stride` bytes per
// k: two `ds_read_b64_tr_b16` (the CDNA4 transposing LDS read), k 0-3 at p and k 4-7 four rows further.
__device__ __forceinline__ bf16x8 tr_frag(const uint8_t* p, int row_stride) {
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(p));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(p + 4 * row_stride));
    const s16x8 both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, both);
}

// ---- the LDS-DMA ring ----------------------------------------------------------------------------------------------------
// Three stages filled by `global_load_lds` (16 bytes per lane, no staging registers), a counted `s_waitcnt vmcnt(N)` and ONE
// raw `s_barrier` per step, two steps in flight across it:
//     issue(0); issue(1);
//     for step t:  ring_wait<LPS>(t + 1 < steps);  if (t + 2 < steps) issue(t + 2, ring_refill(cur));
//                  MFMAs on stage cur;  cur = ring_next(cur);
//   * a wave waits for ITS loads of stage t (vmcnt leaves the LPS loads of the newer stage in flight), the barrier publishes
//     all four waves' pieces and retires everybody's reads of stage t - 1, whose buffer the loads for stage t + 2 then
//     overwrite;
//   * LDS-DMA writes wave-uniform base + lane * 16, so a tile is a dense image and every bank swizzle sits on the SOURCE
//     address (the inverse permutation of the fragment reads).
constexpr int NSTAGE = 3;

__device__ __forceinline__ int ring_next(int cur) { return cur == NSTAGE - 1 ? 0 : cur + 1; }
__device__ __forceinline__ int ring_refill(int cur) { return cur >= 1 ? cur - 1 : NSTAGE - 1; }   // (cur + 2) % 3: read one step ago

// Row-major tiles of BK bf16 per row (128- / 64-byte rows) read with `ds_read_b128`: 16-byte slot s of row r holds chunk
// s ^ swz16<BK>(r) -- conflict free for the read's four 16-lane service groups.
template <int BK> __device__ __forceinline__ int swz16(int row) { return BK == 64 ? ((row >> 1) & 7) : (2 * ((row >> 2) & 1)); }

__device__ __forceinline__ unsigned lds_address(const uint8_t* lds) {
    return (unsigned)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)lds;
}

// One LDS-DMA load: 16 bytes per lane from `src` to LDS at dst (wave uniform) + lane * 16.  Inline asm: hipcc's wait-count
// pass would otherwise drain EVERY pending LDS-DMA (`vmcnt(0)`) in front of the first LDS read after an issue -- it cannot
// tell the stage being filled from the stage being read -- which is the whole pipeline.  M0 (the LDS destination base) is
// written in the statement that uses it and restored.
__device__ __forceinline__ void glds16(const uint16_t* src, unsigned dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
}

// The step's wait and barrier.  LPS: LDS-DMA loads per wave and stage; `more`: a newer stage is in flight and stays so.
template <int LPS> __device__ __forceinline__ void ring_wait(bool more) {
    if (more) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPS) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
}
