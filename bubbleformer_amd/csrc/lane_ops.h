// Lane, LDS-transpose, LDS-DMA and wait-count primitives of the gfx950 kernels: each defined once, device code only, no host state.
// What belongs here: a short __forceinline__ wrapper round one instruction sequence that more than one kernel file needs (DPP and
// v_permlane*_swap reductions, ds_read_tr16_b64 reads, global_load_lds issue, counted s_waitcnt, fences).  What does not: anything that
// knows a tile shape or an operand layout (gemm_common.h), and reductions whose summation order another kernel must reproduce: the ordered
// fp64 workgroup reduction is bf_common.h's block_reduce (beside wave_sum), the LDS transform and the radial shell are fft_lines.h's.
#pragma once
#include "bf_common.h"

typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(3))) s16x4* lds_s16x4;
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// ----------------------------------------------------------------------------- ordering
// the wave's own LDS traffic is in order; this only pins the compiler's ordering of it
__device__ __forceinline__ void wsync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// all waves' global stores and atomics have reached the L2 before anybody goes on
__device__ __forceinline__ void drain_and_sync() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); }

// All outstanding vector-memory operations complete, as an s_waitcnt the compiler's wait-count pass models (an inline-asm wait is opaque to
// it).  In front of a loop that prefetches the next problem's rows: the pass merges the loop header's pending-load state from the preheader
// and the back edge, and with the first problem's loads still pending there it counts every use of `cur` at the top of the body against
// them -- vmcnt(7), vmcnt(6), ... right behind the eight NEW loads, i.e. a full memory round trip per problem and no look-ahead at all.
__device__ __forceinline__ void drain_vm() { __builtin_amdgcn_s_waitcnt(0x0F70); }      // vmcnt(0), expcnt / lgkmcnt untouched

// Hand-counted waits (opaque to the compiler): a file that calls one of these orders memory by count, and tools/register_audit.py
// fails its build on a spill.
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void wait_vm_n(int n) {      // n is wave-uniform; a smaller count than asked for is always safe (in-order retirement)
    if (n >= 16) { wait_vm<16>(); return; }
    switch (n) {
        case 0: wait_vm<0>(); break;   case 1: wait_vm<1>(); break;   case 2: wait_vm<2>(); break;   case 3: wait_vm<3>(); break;
        case 4: wait_vm<4>(); break;   case 5: wait_vm<5>(); break;   case 6: wait_vm<6>(); break;   case 7: wait_vm<7>(); break;
        case 8: wait_vm<8>(); break;   case 9: wait_vm<9>(); break;   case 10: wait_vm<10>(); break; case 11: wait_vm<11>(); break;
        case 12: wait_vm<12>(); break; case 13: wait_vm<13>(); break; case 14: wait_vm<14>(); break; default: wait_vm<15>(); break;
    }
}
__device__ __forceinline__ void wait_vm_wide(int n) {      // as wait_vm_n, up to 40 outstanding operations (epilogue stores + look-ahead DMAs)
    if (n < 16) { wait_vm_n(n); return; }
    if (n >= 40) { wait_vm<40>(); return; }
    switch ((n - 16) >> 2) {          // steps of 4: a smaller count than asked for is always safe
        case 0: wait_vm<16>(); break; case 1: wait_vm<20>(); break; case 2: wait_vm<24>(); break;
        case 3: wait_vm<28>(); break; case 4: wait_vm<32>(); break; default: wait_vm<36>(); break;
    }
}

// ----------------------------------------------------------------------------- LDS-DMA (global -> LDS, no staging registers)
// One global_load_lds_dwordx4: lane l copies the 16 bytes at its OWN source address to LDS byte lds_dst + 16 * l (lds_dst wave-uniform).
// Written as inline asm on purpose: hipcc models the builtin's LDS write and then drains vmcnt(0) before the next ds_read of the same
// array, which serialises every K-step; hidden from it, the DMA is ordered for readers by the counted s_waitcnt vmcnt + s_barrier the
// kernels place themselves (cdna_hip_programming.md section 5.7 item 1).  M0 (the DMA's LDS base) is saved and restored.
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
// with an immediate byte offset (one source pointer serves the same rows of several sub-chunks).  The instruction adds its immediate to
// BOTH addresses -- the global source and the LDS destination (M0 + offset + 16 * lane) -- so M0 is given the destination minus the offset.
template <int OFF>
__device__ __forceinline__ void glds16_off(const void* gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off offset:%3\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst - (unsigned)OFF), "n"(OFF) : "memory");
}
// with a wave-uniform 64-bit base in SGPRs and a per-lane 32-bit byte offset: one offset register serves every piece of a wave
__device__ __forceinline__ void glds16_s(const void* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ unsigned lds_addr(const void* p) {
    return (unsigned)(uintptr_t)(__attribute__((address_space(3))) const char*)p;
}
// 4 / 8 / 16-byte loads the compiler does not count (it would drain the DMA queue at the first use): completion by the caller's wait_vm_n
__device__ __forceinline__ void gload4(float& dst, const void* p) { asm volatile("global_load_dword %0, %1, off" : "=v"(dst) : "v"(p) : "memory"); }
__device__ __forceinline__ void gload8(uint2& dst, const void* p) { asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(dst) : "v"(p) : "memory"); }
__device__ __forceinline__ void gload16(uint4& dst, const void* p) { asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst) : "v"(p) : "memory"); }

// ----------------------------------------------------------------------------- lane exchanges (VALU only, no LDS crossbar round trip)
// one DPP move (row_mask / bank_mask all, bound_ctrl): the value of the lane CTRL names, and keep + that value of send
template <int CTRL> __device__ __forceinline__ float dpp_get(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
template <int CTRL> __device__ __forceinline__ float dpp_add(float keep, float send) { return keep + dpp_get<CTRL>(send); }
// total of a 16-lane row in every lane of the row: xor-1 / xor-2 quad permutes, then the half-row and row mirrors
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_get<0xB1>(v);      // quad_perm [1,0,3,2]
    v += dpp_get<0x4E>(v);      // quad_perm [2,3,0,1]
    v += dpp_get<0x141>(v);     // row_half_mirror
    v += dpp_get<0x140>(v);     // row_mirror
    return v;
}
// Reductions over a lane quad {l, l+16, l+32, l+48} with the gfx950 row-swap VALU ops, result in every lane:
// v_permlane16_swap(a, b) exchanges the odd 16-lane rows of a with the even rows of b, v_permlane32_swap the upper half of a
// with the lower half of b; with a = b = v the two results are v and its xor-16 / xor-32 partner in every lane.
__device__ __forceinline__ float quad_sum(float v) {
    u32x2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float quad_max(float v) {
    u32x2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
    r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
// v + (v of lane ^ o), o = 8 / 16 / 32: row rotate by 8, then the row / half swaps
__device__ __forceinline__ float lane_xor_add(float v, int o) {
    if (o == 8) return v + dpp_get<0x128>(v);      // row_ror:8
    const unsigned u = __float_as_uint(v);
    const u32x2 r = o == 16 ? __builtin_amdgcn_permlane16_swap(u, u, false, false) : __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float rg8_sum(float v) { return lane_xor_add(lane_xor_add(lane_xor_add(v, 8), 16), 32); }      // over lanes l ^ {8, 16, 32}

// ----------------------------------------------------------------------------- transposing LDS reads
// transposing read of a 4-row x 16-col block of a bf16 LDS tile (row stride ld elements): lane i16 of the 16-lane group gets
// column c0 + i16 of rows r0..r0+3
__device__ __forceinline__ s16x4 tr4(const bf16* tile, int ld, int r0, int c0, int lane) {
    const int i16 = lane & 15, q = i16 >> 2, p = i16 & 3;
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(tile + (r0 + q) * ld + c0 + 4 * p));
}
// two such reads, four rows apart, make the eight consecutive k of an MFMA bf16 operand
__device__ __forceinline__ bf16x8 cat(s16x4 lo, s16x4 hi) {
    s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, r);
}

// ----------------------------------------------------------------------------- bf16 <-> bits
__device__ __forceinline__ short bfbits(float x) { return __builtin_bit_cast(short, (bf16)x); }
__device__ __forceinline__ float bf_bits_f(short b) { return __uint_as_float(((unsigned)(unsigned short)b) << 16); }

// ----------------------------------------------------------------------------- T5 relative-position bucket
// one-sided T5 bucket for |offset| (num_buckets 32 -> 16 per side, max_exact 8, max_distance 32: every |offset| >= 27 is bucket 15);
// restated from the reference formula, checked against the reference's tables in the tests.  The short-axis VALU, short-axis MFMA and
// long-axis attention kernels all index their bias table through this one function.
__device__ __forceinline__ int t5_bucket(int n) {
    const int a = n < 0 ? -n : n;
    int b;
    if (a < 8) b = a;
    else if (a < 10) b = 8;
    else if (a < 12) b = 9;
    else if (a < 14) b = 10;
    else if (a < 16) b = 11;
    else if (a < 20) b = 12;
    else if (a < 23) b = 13;
    else if (a < 27) b = 14;
    else b = 15;
    return b + (n < 0 ? 16 : 0);   // n = query - key; key after query -> upper half
}
