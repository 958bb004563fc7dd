// Device primitives the two MFMA translation units (gemm.hip, flash.hip) share: the
// buffer-resource LDS-DMA and the types and LDS addressing of the transposed fragment reads.
// Everything here is __forceinline__ with internal linkage: no symbol of a code object comes
// from this header.
#pragma once
#include "fs2_common.h"

typedef __attribute__((ext_vector_type(4))) int i32x4;
__device__ void llvm_raw_buffer_load_lds(i32x4 rsrc, __attribute__((address_space(3))) uint32_t* lds,
                                         int size, int voffset, int soffset, int offset,
                                         int aux) __asm("llvm.amdgcn.raw.buffer.load.lds");

namespace {

// operands of ds_read_b64_tr_b16 (the builtin and the inline-asm form)
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// the 32-bit LDS address of a pointer into __shared__ memory, as inline-asm LDS reads take it
__device__ __forceinline__ uint32_t lds_off(const void* p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)p;
}

// Buffer-resource form of the LDS-DMA (buffer_load_dwordx4 ... lds): a wave-uniform base in
// SGPRs, a 32-bit per-lane byte offset and a uniform SGPR offset.  Lanes with the offset
// BUF_OOB fall outside num_records and load zeros -- no per-lane pointer selects.
constexpr int BUF_OOB = (int)0x80000000u;
__device__ __forceinline__ i32x4 make_rsrc(const void* base) {
  const uint64_t a = (uint64_t)base;
  i32x4 r;
  r[0] = __builtin_amdgcn_readfirstlane((int)(a & 0xffffffffu));
  r[1] = __builtin_amdgcn_readfirstlane((int)(a >> 32));
  r[2] = 0x7fffffff;
  r[3] = 0x00020000;
  return r;
}
__device__ __forceinline__ void blds16(i32x4 rsrc, int voff, int soff, char* lds_wave_base) {
  llvm_raw_buffer_load_lds(rsrc, (__attribute__((address_space(3))) uint32_t*)lds_wave_base, 16,
                           voff, soff, 0, 0);
}
// 4-byte variant: 64 lanes x 4 B land contiguously (one float per lane, e.g. a row statistic)
__device__ __forceinline__ void blds4(i32x4 rsrc, int voff, int soff, char* lds_wave_base) {
  llvm_raw_buffer_load_lds(rsrc, (__attribute__((address_space(3))) uint32_t*)lds_wave_base, 4,
                           voff, soff, 0, 0);
}

}  // namespace
