// cdna4.h -- the gfx950 (CDNA4) primitives the matrix-core kernels share: vector / address-space types, LDS-DMA, fragment reads by
// inline asm with their waits, counted vmcnt waits, the 64-byte-row swizzle, the bf16 pack.  A helper that one file uses stays there.
#pragma once
#include "common.h"
#include <type_traits>

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef short s16x4_t __attribute__((ext_vector_type(4)));
typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// 64 zero bytes: the source of every LDS-DMA piece that falls outside the volume / beyond the K range
// (static: one per translation unit that reads it -- the library is linked without relocatable device code)
static __device__ __attribute__((aligned(64))) unsigned int m1_zero_page[16];

// one wave-instruction: 64 lanes x 16 bytes from per-lane global addresses to lds_wave_base + lane*16
__device__ __forceinline__ void m1_glds16(const void* g, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)lds_wave_base, 16, 0, 0);
}

// 64 lanes x 16 bytes, global (buffer resource `rs`, per-lane byte offset `voff`; out of range -> zeros) -> LDS at the
// wave-uniform byte address `lds` + 16 * lane.  M0 carries the LDS base of an LDS-DMA.
__device__ __forceinline__ void m1_lds_dma(i32x4_t rs, unsigned lds, unsigned voff) {
    // (M0 is written here without a clobber: "m0" is a reserved register to hipcc -- it warns on the clobber -- and these kernels contain no
    // compiler-generated M0 use that a stale value could reach; tools/isa_async_check.py / tests/test_build_props.py verify that on the ISA)
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" :: "s"(lds), "v"(voff), "s"(rs) : "memory");
}
// the same with a wave-uniform byte offset `soff` in a scalar register
__device__ __forceinline__ void m1_lds_dma(i32x4_t rs, unsigned lds, unsigned voff, unsigned soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" :: "s"(lds), "v"(voff), "s"(rs), "s"(soff) : "memory");
}

__device__ __forceinline__ u32x4_t m1_lds_read128(unsigned lds_addr) {
    u32x4_t v;
    asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(lds_addr) : "memory");
    return v;
}
// transpose-read by inline asm: hipcc cannot tell an LDS-DMA still in flight from the buffer being read and would wait
// vmcnt(0) in front of every compiler-visible LDS read (no prefetch depth at all)
__device__ __forceinline__ u32x2_t m1_tr_read_asm(unsigned lds_addr) {
    u32x2_t v;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(lds_addr) : "memory");
    return v;
}
// all outstanding LDS reads have landed; tying the fragment makes its consumers wait behind this statement
__device__ __forceinline__ void m1_lds_wait(u32x4_t& v) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v)); }
__device__ __forceinline__ void m1_lds_wait(u32x2_t& a, u32x2_t& b) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b)); }
// the same with at most N younger LDS reads still in flight (LDS reads return in order)
template <int N> __device__ __forceinline__ void m1_lds_wait_n(u32x2_t& a, u32x2_t& b) {
    static_assert(N >= 0 && N <= 15, "lgkmcnt immediate");
    asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N));
}
// no instruction: only orders the consumers of v behind the preceding (volatile) wait
__device__ __forceinline__ void m1_lds_tie(u32x4_t& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ bf16x8_t m1_frag8(u32x2_t lo, u32x2_t hi) {
    return __builtin_bit_cast(bf16x8_t, __builtin_shufflevector(lo, hi, 0, 1, 2, 3));
}
// transpose read, compiler-visible (it packs the two halves of a fragment into one register quadruple, folds constant
// offsets into the instruction and schedules the lgkmcnt waits): 4 voxels x 16 channels block -> this lane's channel, 4 consecutive
// voxels.  For kernels whose LDS-DMA is issued from inline asm, so the compiler never sees a pending LDS write that it would drain
// with vmcnt(0) in front of every read.
__device__ __forceinline__ s16x4_t m1_tr_read(const unsigned char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)p);
}

// at most n LDS-DMA pieces of this wave still in flight (n wave-uniform); n > MAXN waits for all of them
template <int MAXN, int N = 0> __device__ __forceinline__ void m1_wait_vm(int n) {
    static_assert(MAXN >= 0 && MAXN <= 63, "vmcnt immediate");
    if constexpr (N > MAXN) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if (n == N) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
    else m1_wait_vm<MAXN, N + 1>(n);
}
template <int N_> __device__ __forceinline__ void m1_wait_vm_imm() {
    static_assert(N_ >= 0 && N_ <= 63, "vmcnt immediate");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N_) : "memory");
}

// segment XOR-swizzle of the 64-byte LDS rows: seg' = seg ^ ((-(row>>2))&3) makes every ds_read_b128 fragment read conflict-free on
// gfx950's 16-lane b128 groups
__device__ __forceinline__ int m1_swz64(int row, int seg) { return seg ^ ((-(row >> 2)) & 3); }

// pack two floats to bf16x2 (round to nearest even): one v_cvt_pk_bf16_f32
__device__ __forceinline__ unsigned m1_cvt_pk_bf16(float a, float b) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_t){a, b}, bf16x2_t));
}

// f(integral_constant<int, I>) for I = B .. E - 1: an unrolled loop whose index is a constant expression (asm immediates, slot numbers)
template <int B, int E, class F> __device__ __forceinline__ void m1_static_for(F&& f) {
    if constexpr (B < E) { f(std::integral_constant<int, B>{}); m1_static_for<B + 1, E>(f); }
}
