// Asm-issued loads, MFMAs and waits of the register-filter kernels (conv_rf.hip, conv_dblock2.hip): the compiler must not know the filter
// loads (it would sink them next to their use or spill what it cannot colour), so they are issued into a register class chosen here,
// waited for by hand and consumed by asm MFMAs.  Every statement carries a "memory" clobber: that keeps them in SOURCE order.
#pragma once
#include <type_traits>

#include "mfma_util.h"

typedef __attribute__((ext_vector_type(4))) int i32x4_t;

#if RCGAN_HALF_FP16
#define RF_MFMA "v_mfma_f32_16x16x32_f16"
#else
#define RF_MFMA "v_mfma_f32_16x16x32_bf16"
#endif

template <int OFF> __device__ __forceinline__ void rf_load_a(i32x4_t& dst, const void* p) {
  asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=a"(dst) : "v"(p), "n"(OFF) : "memory");
}
template <int OFF> __device__ __forceinline__ void rf_load_v(i32x4_t& dst, const void* p) {
  asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=v"(dst) : "v"(p), "n"(OFF) : "memory");
}
// ... into a register that holds a value this wavefront has finished with (a ring slot): the operand is tied, so the new value lives in the
// register of the old one and the allocator has no reason to move either while the load is in flight
template <int OFF> __device__ __forceinline__ void rf_load_a_inplace(i32x4_t& dst, const void* p) {
  asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "+a"(dst) : "v"(p), "n"(OFF) : "memory");
}
__device__ __forceinline__ void rf_mfma_a(f32x4_t& acc, const i32x4_t& w, const bf16x8_t& x) {
  asm volatile(RF_MFMA " %0, %1, %2, %0" : "+v"(acc) : "a"(w), "v"(x) : "memory");
}
__device__ __forceinline__ void rf_mfma_v(f32x4_t& acc, const i32x4_t& w, const bf16x8_t& x) {
  asm volatile(RF_MFMA " %0, %1, %2, %0" : "+v"(acc) : "v"(w), "v"(x) : "memory");
}
// first K-step of a group: C = 0 (an inline constant) -- a VALU zero-fill in front of an MFMA the compiler cannot see misses the wait
// states "VALU write -> MFMA SrcC read" needs: the group's first accumulator came out wrong
__device__ __forceinline__ void rf_mfma_a0(f32x4_t& acc, const i32x4_t& w, const bf16x8_t& x) {
  asm volatile(RF_MFMA " %0, %1, %2, 0" : "=v"(acc) : "a"(w), "v"(x) : "memory");
}
// ... the same where the operand registers die with this instruction (conv_dblock1.hip): early clobber, vDst must not be given SrcA's or SrcB's
__device__ __forceinline__ void rf_mfma_a0e(f32x4_t& acc, const i32x4_t& w, const bf16x8_t& x) {
  asm volatile(RF_MFMA " %0, %1, %2, 0" : "=&v"(acc) : "a"(w), "v"(x) : "memory");
}
// C = 0 with both operands in VGPRs: the one-MFMA image-end products of a kernel whose AccVGPRs hold a filter stream in flight (a builtin
// MFMA lets the compiler put its result in AccVGPRs, and it moves what it believes lives there out of the way -- before the loads land).
// The operands may come straight out of vector ALU instructions the compiler is free to place directly in front of this statement, and
// its hazard recogniser does not look inside: the wait states sit in the statement itself (without them the first product of a tile
// came out wrong).
__device__ __forceinline__ void rf_mfma_vv0(f32x4_t& acc, const bf16x8_t& w, const bf16x8_t& x) {
  asm volatile("s_nop 4\n\t" RF_MFMA " %0, %1, %2, 0" : "=&v"(acc) : "v"(w), "v"(x) : "memory");
}
__device__ __forceinline__ void rf_lds_read(bf16x8_t& dst, unsigned lds_byte_addr) {
  asm volatile("ds_read_b128 %0, %1" : "=v"(dst) : "v"(lds_byte_addr) : "memory");
}
template <int N> __device__ __forceinline__ void rf_wait() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }
__device__ __forceinline__ void rf_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <int I, int N, typename F> __device__ __forceinline__ void rf_for(F&& f) {
  if constexpr (I < N) { f(std::integral_constant<int, I>{}); rf_for<I + 1, N>(f); }
}

// rows [R][K] (rcgan_conv_prepare layout) -> fragment-major [block of 16*ctn rows][slice][step][tile ctn][lane 64][8]: lane (r = l & 15,
// kc = l >> 4) of (block b, slice sl, step s, tile ct) owns row b*16*ctn + ct*16 + r, elements (sl*ss + s)*32 + kc*8 ..+8.
struct FragItem { const bf16_t* src; bf16_t* dst; int K, ctn, ss, nsl, chunks; };

// The down block's fused forward (conv_dblock2.hip) reads two more copies, [Conv2 summed filters: 4 blocks of 32 rows][64 K-steps][2 tiles]
// followed by [Shortcut: 4 blocks][4 K-steps][2 tiles]: its fragment items, written by the fragment launch of conv_rf.hip.
// Its fused data gradient (conv_dblock2_bwd.hip) reads two more behind them: [Conv2's summed data-gradient filters, phase layout
// [4 phases][128][4 * 128] taken as 512 rows: 16 blocks of 32 rows (phase, channel block)][16 K-steps][2 tiles] and [Shortcut, rotated rows:
// 4 blocks][4 K-steps][2 tiles].
constexpr long DB2_FRAG_CONV2 = 16L * 128 * 128;      // elements of the gather layout [128][16 * 128]
constexpr long DB2_FRAG_SHORT = 128L * 128;
constexpr long DB2_FRAG_CONV2_BWD = DB2_FRAG_CONV2 + DB2_FRAG_SHORT;          // element offsets of the data gradient's copies
constexpr long DB2_FRAG_SHORT_BWD = DB2_FRAG_CONV2_BWD + DB2_FRAG_CONV2;
constexpr long DB2_FRAG_ELEMS = DB2_FRAG_SHORT_BWD + DB2_FRAG_SHORT;
constexpr int DB2_FRAG_ITEMS = 4;
inline void dblock2_frag_items(const bf16_t* conv2_sum_fwd, const bf16_t* shortcut_fwd, const bf16_t* conv2_sum_bwd, const bf16_t* shortcut_rot,
                               bf16_t* frag, FragItem* it) {
  it[0] = FragItem{conv2_sum_fwd, frag, 2048, 2, 64, 1, (int)(DB2_FRAG_CONV2 / 8)};
  it[1] = FragItem{shortcut_fwd, frag + DB2_FRAG_CONV2, 128, 2, 4, 1, (int)(DB2_FRAG_SHORT / 8)};
  it[2] = FragItem{conv2_sum_bwd, frag + DB2_FRAG_CONV2_BWD, 512, 2, 16, 1, (int)(DB2_FRAG_CONV2 / 8)};
  it[3] = FragItem{shortcut_rot, frag + DB2_FRAG_SHORT_BWD, 128, 2, 4, 1, (int)(DB2_FRAG_SHORT / 8)};
}

// The input block's fused forward (conv_dblock1.hip) reads one copy: [Conv2 summed filters: 4 blocks of 32 rows][64 K-steps][2 tiles], the
// layout of the down block's first item.  (Its Conv1 and shortcut rows, [128][32], are read where conv_image.hip's preparation leaves them:
// the 16 rows of a fragment are one contiguous KiB there already.)
constexpr long DB1_FRAG_ELEMS = 16L * 128 * 128;
constexpr int DB1_FRAG_ITEMS = 1;
inline void dblock1_frag_items(const bf16_t* conv2_sum_fwd, bf16_t* frag, FragItem* it) {
  it[0] = FragItem{conv2_sum_fwd, frag, 2048, 2, 64, 1, (int)(DB1_FRAG_ELEMS / 8)};
}
