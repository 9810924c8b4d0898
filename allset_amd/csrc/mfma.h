// Device primitives shared by the dense (MFMA) kernels: fragment types, DPP row reductions, LDS layouts and reads, operand splits,
// and the macros of the role-split pipelines.  Include after common.h.  One definition each; a kernel file that needs a different
// form keeps it under a name that says what differs (docs/DESIGN_HISTORY.md has the rounds these came from).
#pragma once

#include <type_traits>

#include "common.h"

#ifdef __HIPCC__

namespace allset {

// ---- MFMA operand / accumulator vectors, and the 16-byte fragment seen as each of them -------------------------------------------
using bf16x8 = __attribute__((__vector_size__(8 * sizeof(__bf16)))) __bf16;        // A / B of v_mfma_f32_*_bf16
using f16x8 = __attribute__((__vector_size__(8 * sizeof(_Float16)))) _Float16;     // A / B of v_mfma_f32_*_f16
using f32x4 = __attribute__((ext_vector_type(4))) float;                           // C / D of the 16x16 tiles
using f32x16 = __attribute__((ext_vector_type(16))) float;                         // C / D of the 32x32 tiles
using i16x4 = __attribute__((ext_vector_type(4))) short;                           // one ds_read_b64_tr_b16 result
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;                         // an operand of v_dot2_f32_bf16
// u: as loaded (ds_read_b128 / four packed dwords); v / h: the bf16 / fp16 MFMA operand; t: the two halves of a transposing read
union Frag { uint4 u; bf16x8 v; f16x8 h; struct { i16x4 lo, hi; } t; };

// ---- DPP: the 16 lanes of a DPP row -----------------------------------------------------------------------------------------------
// v from the lane that v_mov_b32_dpp's control CTRL names (all rows and banks enabled, no bound control)
template <int CTRL>
__device__ __forceinline__ float dpp_row(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
// sum / max over the 16 lanes of a DPP row, result in every lane of it: 0xB1 quad_perm [1,0,3,2], 0x4E quad_perm [2,3,0,1],
// 0x141 row_half_mirror, 0x140 row_mirror -- four VALU instructions with DPP operands, no LDS permute
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_row<0xB1>(v);
  v += dpp_row<0x4E>(v);
  v += dpp_row<0x141>(v);
  v += dpp_row<0x140>(v);
  return v;
}
__device__ __forceinline__ float row16_max(float v) {       // (v >= 0)
  v = fmaxf(v, dpp_row<0xB1>(v));
  v = fmaxf(v, dpp_row<0x4E>(v));
  v = fmaxf(v, dpp_row<0x141>(v));
  v = fmaxf(v, dpp_row<0x140>(v));
  return v;
}

// ---- LDS layouts ------------------------------------------------------------------------------------------------------------------
// byte offset of (row, column byte) in a [rows][256 B] plane of 16-bit elements: 64-byte chunk XOR row & 3, 16-byte piece XOR
// (row >> 2) & 3 -- the row-wise 16-byte fragment reads, the row-wise 8-byte stores and the transposing reads are all conflict-free
__device__ __forceinline__ int swizzle256(int row, int colbyte) {
  return row * 256 + ((((colbyte >> 6) ^ row) & 3) << 6) + (((((colbyte >> 4) & 3) ^ (row >> 2)) & 3) << 4) + (colbyte & 15);
}
// dword offset of 16-byte piece t of (k-quarter g, column j) inside a weight plane [k-quarter][column][KQD dwords], GS dwords per
// quarter: the piece index is XOR-swizzled by the column so that a B fragment is one conflict-free ds_read_b128
template <int KQD, int GS>
__device__ __forceinline__ int plane_off(int g, int j, int t) {
  constexpr int PIECES = KQD / 4, ROWS64 = (64 / KQD) > 0 ? (64 / KQD) : 1;
  return g * GS + j * KQD + 4 * (t ^ ((j / ROWS64) % PIECES));
}

// ---- LDS reads --------------------------------------------------------------------------------------------------------------------
// LDS byte offsets as 32-bit integers (address space 3 kept: a round trip through a generic pointer turns the reads into flat loads)
using lds_u8 = __attribute__((address_space(3))) uint8_t;
__device__ __forceinline__ uint32_t lds_off(const void* p) { return static_cast<uint32_t>(reinterpret_cast<uintptr_t>((lds_u8*)(p))); }
__device__ __forceinline__ uint4 lds_read16(uint32_t off) {       // ds_read_b128
  const u32x4 v = *reinterpret_cast<const __attribute__((address_space(3))) u32x4*>(static_cast<uintptr_t>(off));
  return make_uint4(v.x, v.y, v.z, v.w);
}
// Two ds_read_b64_tr_b16 (hardware 4 x 4 transpose of 16-bit elements inside each 16-lane group): the MFMA fragment of 8 consecutive
// ROWS of one column out of a row-major image; lo / hi address the lane's 8 bytes of rows 0-3 / 4-7.  V: what the caller takes the
// fragment as -- bf16x8, f16x8 or the whole Frag.  Pointer form (also as pointer + byte stride to the upper half), offset form.
template <typename V>
__device__ __forceinline__ V frag_as(const Frag& f) {
  if constexpr (std::is_same<V, Frag>::value) return f;
  else if constexpr (std::is_same<V, f16x8>::value) return f.h;
  else return f.v;
}
template <typename V>
__device__ __forceinline__ V tr_frag2(const uint8_t* lo, const uint8_t* hi) {
  Frag f;
  f.t.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)(lo));
  f.t.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)(hi));
  return frag_as<V>(f);
}
template <typename V>
__device__ __forceinline__ V tr_frag2(const uint8_t* lo, int half_stride) { return tr_frag2<V>(lo, lo + half_stride); }
template <typename V>
__device__ __forceinline__ V tr_frag2_off(uint32_t lo, uint32_t hi) {
  Frag f;
  f.t.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<__attribute__((address_space(3))) i16x4*>(static_cast<uintptr_t>(lo)));
  f.t.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<__attribute__((address_space(3))) i16x4*>(static_cast<uintptr_t>(hi)));
  return frag_as<V>(f);
}

// ---- fp32 on the fp16 matrix pipe (the bf16 form, split3_bf16, is in common.h) ------------------------------------------------------
// "fp16x3".  x0, x1 -> packed fp16 planes {hi half: x1, lo half: x0}: h = RN16(x), l = RN16(x - h) (v_cvt_pk_f16_f32; x - h is exact
// in fp32, v_fma_mix_f32; fp16 denormals are produced and the f16 MFMA honours them): (x s)(w t) = h h' + h l' + l h' + (l l' <= 2^-22,
// dropped); the operands must have been scaled into fp16's window by a power of two (fused_bwd6.hip has the scheme and its error model)
__device__ __forceinline__ void split2_f16(float x0, float x1, uint32_t& ph, uint32_t& pl) {
  float r0, r1;
  asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(ph) : "v"(x0), "v"(x1));
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r0) : "v"(ph), "v"(x0));
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r1) : "v"(ph), "v"(x1));
  asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(pl) : "v"(r0), "v"(r1));
}

}  // namespace allset

// ---- macros of the role-split pipelines (vector waves | matrix waves, one workgroup barrier per tick) -----------------------------
// A lane id the compiler cannot hoist: v_mbcnt_lo / v_mbcnt_hi recompute it and the empty asm makes the copy opaque, so the addresses
// derived from it are re-derived per phase (a few integer instructions) instead of living in registers across the whole stage loop.
#define ALLSET_FRESH_LANE(name) \
  int name = static_cast<int>(__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u))); __asm__ volatile("" : "+v"(name))
// The tick: this wave's LDS operations retired (s_waitcnt lgkmcnt(0)), then the workgroup barrier.  A kernel file defines its
// ALLSET_TICK() as one of the two under its OWN ablation switch (ALLSET_ABL*_NOBAR: timing without the barriers, results wrong).
#define ALLSET_TICK_BARRIER() __asm__ volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
#define ALLSET_TICK_NO_BARRIER() __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
// Phase mark of the diagnostic timing builds: the cycles (s_memtime) since the previous mark go to tph[k].  A kernel declares
// `uint64_t tph[N], tlast` and defines its mark as this one under its OWN timing switch, as nothing otherwise.
#define ALLSET_PHASE_MARK(k) do { const uint64_t tn = __builtin_readcyclecounter(); tph[k] += tn - tlast; tlast = tn; } while (0)

#endif  // __HIPCC__
