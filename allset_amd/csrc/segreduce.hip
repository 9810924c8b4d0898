// Deep Sets aggregation kernels for gfx950:  out[t,:] = reduce_j w[j] * x[col[j],:]  over CSR rows.
// Replaces the index_select -> mul -> torch_scatter.scatter triple of reference layers.py:633-656
// (three [nnz,d] temporaries + atomics) with ONE gather pass: rows are never materialised per
// incidence, the segment is reduced in registers and written once, coalesced, without atomics.
//
// Mapping to the machine (CDNA4, wave = 64):
//   * one wavefront per CSR row, 4 rows per 256-thread workgroup;
//   * a feature row of d f32 is covered by LPR lanes x 16 B (VEC = 4); with d = 128 that is 32
//     lanes = one 512-B row per half-wave, so a single global_load_dwordx4 gathers NS = 64/LPR
//     different source rows at once (two for d = 128) -- every lane always moves 16 B;
//   * the up-to-64 column ids of the row are fetched with ONE coalesced load (lane j holds id j)
//     and broadcast with ds_bpermute, so the U*NS row gathers of an unrolled step are independent
//     loads issued back-to-back (U = 8: 8 KiB in flight per wave, > 1 MiB per CU at full occupancy);
//   * the NS partial sums are combined with log2(NS) xor-shuffles; slot 0 stores the row.
// HBM-bound by construction: algorithmic bytes per launch are nnz*(4*d + 4) + (n_t+1)*4 + n_t*4*d
// (SURVEY.md section 8(d3)); VALU work is one FMA per gathered element.
#include "common.h"
#include "flat_rows.h"
#include "mfma.h"     // dpp_row

namespace allset {

enum { kModeSum = 0, kModeExt = 1 };
constexpr int kUnroll = 8;
// gather batches of the one-wave-per-row kernel when a row takes the whole wave (NS = 1: d = 256 f32 / 512 bf16 and wider);
// tools/segreduce_ablation.py rebuilds with other values
#ifndef ALLSET_SEG_UNROLL_ONE_SLOT
#define ALLSET_SEG_UNROLL_ONE_SLOT 8
#endif
#ifndef ALLSET_SEG_MAX_LPR
#define ALLSET_SEG_MAX_LPR 64
#endif
constexpr int kBwdUnroll = 4;      // segmax_bwd: incidences per slot in flight (two 16-byte loads each)

template <typename T, int VEC, int LPR, int MODE, bool WEIGHTED>
__global__ __launch_bounds__(kBlock) void segreduce_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ w,
    const T* __restrict__ x, int64_t ldx, T* __restrict__ out, int64_t ldo,
    int32_t* __restrict__ argext, int n_t, int d, int mean, float sign, const int32_t* __restrict__ row_order) {
  constexpr int NS = kWave / LPR;
  constexpr int U = NS == 1 ? ALLSET_SEG_UNROLL_ONE_SLOT : kUnroll;
  const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int slot_row = static_cast<int>(blk) * kWavesPerBlock + (threadIdx.x >> 6);
  if (slot_row >= n_t) return;  // whole wave exits together
  // optional processing order (skewed degree distributions): the long rows of each XCD's range come first, so that
  // a 4096-member row, which keeps one wave busy for ~0.3 ms, starts at t = 0 instead of setting the kernel's tail
  const int row = row_order ? row_order[slot_row] : slot_row;
  const int lane = lane_id();
  const int slot = lane / LPR, li = lane % LPR;
  const int start = rowptr[row], end = rowptr[row + 1];

  for (int cb = 0; cb < d; cb += LPR * VEC) {
    const int c0 = cb + li * VEC;
    const bool active = c0 < d;
    float acc[VEC];
    int32_t arg[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) { acc[k] = 0.f; arg[k] = -1; }

    for (int base = start; base < end; base += kWave) {
      const int n = min(kWave, end - base);
      int my_col = 0;
      float my_w = 0.f;
      if (lane < n) {
        my_col = col[base + lane];
        if constexpr (WEIGHTED) my_w = w[base + lane];
      }
      for (int j = 0; j < n; j += NS * U) {
        Raw<T, VEC> raw[U];        // kept packed while in flight (16 B per lane and load)
        float ww[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int jj = j + u * NS + slot;
          ok[u] = (jj < n) && active;
          const int src = __shfl(my_col, jj & (kWave - 1));
          if constexpr (WEIGHTED) ww[u] = __shfl(my_w, jj & (kWave - 1)); else ww[u] = 1.f;
          if (ok[u]) raw[u] = load_raw<T, VEC>(x + static_cast<int64_t>(src) * ldx + c0);
          else raw[u] = zero_raw<T, VEC>();
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const FVec<VEC> v = unpack<T, VEC>(raw[u]);
          if constexpr (MODE == kModeSum) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = fmaf(ww[u], v.v[k], acc[k]);   // ok==false -> v == 0
          } else {
            if (ok[u]) {
              const int pos = base + j + u * NS + slot;
#pragma unroll
              for (int k = 0; k < VEC; ++k) {
                const float val = sign * (ww[u] * v.v[k]);
                if (arg[k] < 0 || val > acc[k]) { acc[k] = val; arg[k] = pos; }
              }
            }
          }
        }
      }
    }

    // combine the NS slots (each reduced a disjoint subset of the row's incidences)
#pragma unroll
    for (int off = LPR; off < kWave; off <<= 1) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const float o = __shfl_xor(acc[k], off);
        if constexpr (MODE == kModeSum) {
          acc[k] += o;
        } else {
          const int oa = __shfl_xor(arg[k], off);
          if (oa >= 0 && (arg[k] < 0 || o > acc[k] || (o == acc[k] && oa < arg[k]))) { acc[k] = o; arg[k] = oa; }
        }
      }
    }

    if (slot == 0 && active) {
      FVec<VEC> r;
      if constexpr (MODE == kModeSum) {
        const float scale = mean ? 1.f / static_cast<float>(max(end - start, 1)) : 1.f;
#pragma unroll
        for (int k = 0; k < VEC; ++k) r.v[k] = acc[k] * scale;
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) r.v[k] = arg[k] >= 0 ? sign * acc[k] : 0.f;   // empty row -> 0
        if (argext != nullptr) store_vec_i32<VEC>(argext + static_cast<int64_t>(row) * d + c0, arg);
      }
      store_vec<T, VEC>(out + static_cast<int64_t>(row) * ldo + c0, r);
    }
  }
}


// ---- short-row variant (flat_rows.h): sum / mean, single column chunk ------------------------------------------------
template <typename T, int VEC, int LPR, bool WEIGHTED>
__global__ __launch_bounds__(kBlock) void segreduce_flat_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ w,
    const T* __restrict__ x, int64_t ldx, T* __restrict__ out, int64_t ldo, int n_t, int d, int mean) {
  FlatSlot<LPR> s;
  if (s.wave_beyond(n_t)) return;
  s.open(rowptr, n_t);
  const int c0 = s.li * VEC;
  const bool active = c0 < d;
  int cur_start = s.q0;              // of the current row: the mean's count is cur_end - cur_start
  float acc[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
  int my_col = 0;
  float my_w = 0.f;
  Raw<T, VEC> raw[kUnroll];
  float ww[kUnroll];

  flat_walk<kUnroll>(
      s, active,
      [&](int base, int n) {
        my_col = 0;
        my_w = 0.f;
        if (s.li < n) {
          my_col = col[base + s.li];
          if constexpr (WEIGHTED) my_w = w[base + s.li];
        }
      },
      [&](int u, int jj, bool ok) {
        const int src = s.bcast(my_col, jj);
        if constexpr (WEIGHTED) ww[u] = s.bcast(my_w, jj); else ww[u] = 1.f;
        if (ok) raw[u] = load_raw<T, VEC>(x + static_cast<int64_t>(src) * ldx + c0);
        else raw[u] = zero_raw<T, VEC>();
      },
      [&](int u) {
        const FVec<VEC> v = unpack<T, VEC>(raw[u]);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = fmaf(ww[u], v.v[k], acc[k]);
      },
      [&] {
        if (active) {
          const float scale = mean ? 1.f / static_cast<float>(max(s.cur_end - cur_start, 1)) : 1.f;
          FVec<VEC> r;
#pragma unroll
          for (int k = 0; k < VEC; ++k) { r.v[k] = acc[k] * scale; acc[k] = 0.f; }
          store_vec<T, VEC>(out + static_cast<int64_t>(s.cur_row) * ldo + c0, r);
        }
        cur_start = s.cur_end;
      });
}

// gx[s,c] = sum_{j in T-row s} [argext[colT[j],c] == posT[j]] * wT[j] * gout[colT[j],c]
template <int VEC, int LPR, bool WEIGHTED>
__global__ __launch_bounds__(kBlock) void segmax_bwd_kernel(
    const int32_t* __restrict__ rowptrT, const int32_t* __restrict__ colT, const int32_t* __restrict__ posT,
    const float* __restrict__ wT, const int32_t* __restrict__ argext, const float* __restrict__ gout,
    int64_t ldg, float* __restrict__ gx, int64_t ldx, int n_s, int d) {
  constexpr int NS = kWave / LPR;
  const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int row = static_cast<int>(blk) * kWavesPerBlock + (threadIdx.x >> 6);
  if (row >= n_s) return;
  const int lane = lane_id();
  const int slot = lane / LPR, li = lane % LPR;
  const int start = rowptrT[row], end = rowptrT[row + 1];

  for (int cb = 0; cb < d; cb += LPR * VEC) {
    const int c0 = cb + li * VEC;
    const bool active = c0 < d;
    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
    for (int base = start; base < end; base += kWave) {
      const int n = min(kWave, end - base);
      int my_col = 0, my_pos = -2;
      float my_w = 1.f;
      if (lane < n) {
        my_col = colT[base + lane];
        my_pos = posT[base + lane];
        if constexpr (WEIGHTED) my_w = wT[base + lane];
      }
      // kBwdUnroll incidences per slot in flight: each is two independent 16-byte loads (the gradient row and the arg row of
      // the target), issued back to back before any of them is consumed
      for (int j = 0; j < n; j += NS * kBwdUnroll) {
        FVec<VEC> g[kBwdUnroll];
        int32_t a[kBwdUnroll][VEC];
        int pos[kBwdUnroll];
        float ww[kBwdUnroll];
#pragma unroll
        for (int u = 0; u < kBwdUnroll; ++u) {
          const int jj = j + u * NS + slot;
          const bool ok = (jj < n) && active;
          const int t = __shfl(my_col, jj & (kWave - 1));             // (shuffles run with every lane active: before the select)
          const int ps = __shfl(my_pos, jj & (kWave - 1));
          pos[u] = ok ? ps : -2;                                      // -2 never equals an arg entry (>= -1)
          ww[u] = __shfl(my_w, jj & (kWave - 1));
          if (jj < n && active) {
            g[u] = load_vec<float, VEC>(gout + static_cast<int64_t>(t) * ldg + c0);
            load_vec_i32<VEC>(argext + static_cast<int64_t>(t) * d + c0, a[u]);
          } else {
#pragma unroll
            for (int k = 0; k < VEC; ++k) { g[u].v[k] = 0.f; a[u][k] = -1; }
          }
        }
#pragma unroll
        for (int u = 0; u < kBwdUnroll; ++u)
#pragma unroll
          for (int k = 0; k < VEC; ++k)
            if (a[u][k] == pos[u]) acc[k] = fmaf(ww[u], g[u].v[k], acc[k]);
      }
    }
#pragma unroll
    for (int off = LPR; off < kWave; off <<= 1)
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] += __shfl_xor(acc[k], off);
    if (slot == 0 && active) {
      FVec<VEC> r;
#pragma unroll
      for (int k = 0; k < VEC; ++k) r.v[k] = acc[k];
      store_vec<float, VEC>(gx + static_cast<int64_t>(row) * ldx + c0, r);
    }
  }
}

// gw[j] = scale(t) * sum_c m(j,c) * x[col[j],c] * gout[t,c]   (one wave per CSR row t; LearnMask path)
template <int MODE>
__global__ __launch_bounds__(kBlock) void sddmm_rowdot_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ x,
    int64_t ldx, const float* __restrict__ gout, int64_t ldg, const int32_t* __restrict__ argext,
    float* __restrict__ gw, int n_t, int d, int mean) {
  const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int row = static_cast<int>(blk) * kWavesPerBlock + (threadIdx.x >> 6);
  if (row >= n_t) return;
  const int lane = lane_id();
  const int start = rowptr[row], end = rowptr[row + 1];
  const float scale = mean ? 1.f / static_cast<float>(max(end - start, 1)) : 1.f;
  const float* g = gout + static_cast<int64_t>(row) * ldg;
  const int32_t* ap = argext ? argext + static_cast<int64_t>(row) * d : nullptr;
  for (int j = start; j < end; ++j) {
    const float* xr = x + static_cast<int64_t>(col[j]) * ldx;
    float part = 0.f;
    for (int c = lane; c < d; c += kWave) {
      bool take = true;
      if constexpr (MODE == kModeExt) take = (ap[c] == j);
      if (take) part = fmaf(xr[c], g[c], part);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
    if (lane == 0) gw[j] = part * scale;
  }
}

// The same product on the segreduce skeleton (round 3): the target's gradient row lives in registers (16 bytes per lane,
// LPR lanes per row), the <= 64 column ids of a batch arrive in one coalesced load and are broadcast by ds_bpermute, the
// kUnroll * NS source-row gathers of a step are independent 16-byte loads issued back to back, every gathered row is
// reduced against the register row by four FMAs + a DPP slot sum, and the step's kUnroll * NS results leave in ONE store
// of contiguous floats (lane li < kUnroll of slot s holds incidence j + li * NS + s).  The scalar kernel above -- a serial
// loop over incidences with 4-byte loads, a 6-step shuffle reduction and a lane-0 store per incidence, nothing in flight --
// ran at 0.3 of the gather roofline (3.25 ms per pass at 1M rows x 16 x 128 where segreduce moves the same rows in 1.19).
template <int LPR>
__device__ __forceinline__ float slot_sum(float v) {      // sum over the LPR lanes of a slot, result in every lane of it
  v += dpp_row<0xB1>(v);                                 // quad_perm [1,0,3,2]
  v += dpp_row<0x4E>(v);                                 // quad_perm [2,3,0,1]
  v += dpp_row<0x141>(v);                                // row_half_mirror: the other quad of the 8
  if constexpr (LPR >= 16) v += dpp_row<0x140>(v);       // row_mirror: the other half of the 16
  if constexpr (LPR >= 32) v += __shfl_xor(v, 16);
  if constexpr (LPR >= 64) v += __shfl_xor(v, 32);
  return v;
}

template <int LPR, int MODE>
__global__ __launch_bounds__(kBlock) void sddmm_rowdot_vec_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ x,
    int64_t ldx, const float* __restrict__ gout, int64_t ldg, const int32_t* __restrict__ argext,
    float* __restrict__ gw, int n_t, int d, int mean) {
  constexpr int VEC = 4, NS = kWave / LPR;
  static_assert(LPR >= kUnroll, "the packed store needs a lane per unrolled incidence");
  const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int row = static_cast<int>(blk) * kWavesPerBlock + (threadIdx.x >> 6);
  if (row >= n_t) return;
  const int lane = lane_id();
  const int slot = lane / LPR, li = lane % LPR;
  const int start = rowptr[row], end = rowptr[row + 1];
  const float scale = mean ? 1.f / static_cast<float>(max(end - start, 1)) : 1.f;
  const int c0 = li * VEC;
  const bool active = c0 < d;
  FVec<VEC> g;
  int32_t ap[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) { g.v[k] = 0.f; ap[k] = -1; }
  if (active) {
    g = load_vec<float, VEC>(gout + static_cast<int64_t>(row) * ldg + c0);
    if constexpr (MODE == kModeExt) load_vec_i32<VEC>(argext + static_cast<int64_t>(row) * d + c0, ap);
  }
  for (int base = start; base < end; base += kWave) {
    const int n = min(kWave, end - base);
    const int my_col = lane < n ? col[base + lane] : 0;
    for (int j = 0; j < n; j += NS * kUnroll) {
      Raw<float, VEC> raw[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int jj = j + u * NS + slot;
        const int src = __shfl(my_col, jj & (kWave - 1));
        if (jj < n && active) raw[u] = load_raw<float, VEC>(x + static_cast<int64_t>(src) * ldx + c0);
        else raw[u] = zero_raw<float, VEC>();
      }
      float res = 0.f;
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const FVec<VEC> v = unpack<float, VEC>(raw[u]);
        float part = 0.f;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          if constexpr (MODE == kModeExt) part = (ap[k] == base + j + u * NS + slot) ? fmaf(v.v[k], g.v[k], part) : part;
          else part = fmaf(v.v[k], g.v[k], part);
        }
        part = slot_sum<LPR>(part);
        res = (li == u) ? part : res;
      }
      const int jo = j + li * NS + slot;                 // lanes li < kUnroll: kUnroll * NS consecutive incidences
      if (li < kUnroll && jo < n) gw[base + jo] = res * scale;
    }
  }
}

// ---- packed nonzero rows (include/allset_hip_ext.h: 128-bit occupancy mask + the occupied elements, 256 bytes per row) --------
// The forward aggregations gather dropout(relu(.)) tables, about 3/4 zeros: a packed row is two 128-byte lines where the dense row is
// four, and what bounds the gather is the count of line requests.
constexpr int kPackRowsPerWave = 4;      // pack_kernel:      two rows per 16-byte load instruction, two of them in flight
constexpr int kExpand = 2;               // segreduce_packed_kernel: gathered rows per slot expanded through LDS together (and skipped together)

// the LDS hand-off between lanes of ONE wave (the LDS serves a wave's operations in order): keeps the compiler from moving accesses across
__device__ __forceinline__ void lds_wave_handoff() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// 0xFFFFFFFF when bit `b` of `m` is set, else 0: one signed bit-field extract
__device__ __forceinline__ uint32_t all_ones_if_bit(uint32_t m, int b) {
  return static_cast<uint32_t>(__builtin_amdgcn_sbfe(static_cast<int>(m), static_cast<unsigned>(b), 1u));
}

__device__ __forceinline__ int mask_count(const uint4& m) { return __popc(m.x) + __popc(m.y) + __popc(m.z) + __popc(m.w); }

// Half a wave per row, 16 bytes per lane (columns 4 li .. 4 li + 3): the mask dwords are OR-reduced over the 8 lanes that share one, the
// values are scattered into an LDS image of the row, and the wave's four images leave in ONE coalesced 16-byte store per lane (1 KiB).
// The image is the format's (include/allset_hip_ext.h).  Mask rows: the mask in dwords 0 .. 3, the element of rank j at 4 + j.  Cell rows
// (CELLS): the element of rank j in cell j % 16, slot j / 16, its column in the cell's fourth dword.
template <bool CELLS>
__global__ __launch_bounds__(kBlock) void pack_kernel(const float* __restrict__ x, int64_t ldx, uint32_t* __restrict__ packed, int64_t n) {
  __shared__ __attribute__((aligned(16))) uint32_t image[kWavesPerBlock][kPackRowsPerWave][kPackPitchDw];
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const int slot = lane >> 5, li = lane & 31;
  const int64_t row0 = (static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave) * kPackRowsPerWave;
  if (row0 >= n) return;  // whole wave exits together
  uint4 raw[kPackRowsPerWave / 2];
#pragma unroll
  for (int p = 0; p < kPackRowsPerWave / 2; ++p) {
    const int64_t r = row0 + 2 * p + slot;
    raw[p] = r < n ? *reinterpret_cast<const uint4*>(x + r * ldx + 4 * li) : make_uint4(0u, 0u, 0u, 0u);
  }
#pragma unroll
  for (int p = 0; p < kPackRowsPerWave / 2; ++p) {
    uint32_t* dst = image[wave][2 * p + slot];
    const uint32_t v[4] = {raw[p].x, raw[p].y, raw[p].z, raw[p].w};
    const unsigned nib = (v[0] != 0u ? 1u : 0u) | (v[1] != 0u ? 2u : 0u) | (v[2] != 0u ? 4u : 0u) | (v[3] != 0u ? 8u : 0u);
    const int g = li >> 3, sh = 4 * (li & 7);                        // mask dword of this lane's columns, bit offset in it
    unsigned mw = nib << sh;
    mw |= __shfl_xor(mw, 1);
    mw |= __shfl_xor(mw, 2);
    mw |= __shfl_xor(mw, 4);                                         // all 8 lanes of a group: the group's mask dword
    uint4 m;
    m.x = __shfl(mw, slot * 32);
    m.y = __shfl(mw, slot * 32 + 8);
    m.z = __shfl(mw, slot * 32 + 16);
    m.w = __shfl(mw, slot * 32 + 24);
    // rank of this lane's first occupied column among the row's
    int j = (g > 0 ? __popc(m.x) : 0) + (g > 1 ? __popc(m.y) : 0) + (g > 2 ? __popc(m.z) : 0) + __popc(mw & ((1u << sh) - 1u));
    if constexpr (CELLS) {
      uint8_t* dstb = reinterpret_cast<uint8_t*>(dst);
      const uint32_t k = static_cast<uint32_t>(mask_count(m));
      // every cell starts empty: value bits 0, its own dummy column in the three column bytes, k in the fourth
      if (li < kCellsPerRow) *reinterpret_cast<uint4*>(dst + 4 * li) = make_uint4(0u, 0u, 0u, (128u + li) * 0x010101u | (k << 24));
      lds_wave_handoff();
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if ((nib >> i) & 1u) {
          if (j < kCellCap) {                                        // (an overflow row keeps its first kCellCap elements)
            dst[4 * (j & 15) + (j >> 4)] = v[i];
            dstb[16 * (j & 15) + 12 + (j >> 4)] = static_cast<uint8_t>(4 * li + i);
          }
          ++j;
        }
      }
    } else {
      int pos = 4 + j;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if ((nib >> i) & 1u) {
          if (pos < kPackPitchDw) dst[pos] = v[i];                   // (an overflow row keeps what fits)
          ++pos;
        }
      }
      if (li == 0) *reinterpret_cast<uint4*>(dst) = m;
    }
  }
  lds_wave_handoff();
  const int rr = lane >> 4, q = 4 * (lane & 15);                     // this lane's 16 bytes of the wave's four images
  const uint32_t* src = image[wave][rr];
  uint4 o = *reinterpret_cast<const uint4*>(src + q);
  if constexpr (!CELLS) {
    const int k = mask_count(*reinterpret_cast<const uint4*>(src));
    if (q + 0 >= 4 + k) o.x = 0u;                                    // never-written LDS behind the values
    if (q + 1 >= 4 + k) o.y = 0u;
    if (q + 2 >= 4 + k) o.z = 0u;
    if (q + 3 >= 4 + k) o.w = 0u;
  }
  if (row0 + rr < n) *reinterpret_cast<uint4*>(packed + (row0 + rr) * kPackPitchDw + q) = o;
}

// segreduce_kernel<float, 4, 32, kModeSum, false> over packed rows: the same wave-per-row mapping, block remap, row_order, 64-incidence
// column batches, kUnroll gathers per slot in flight and -- so that the result is BITWISE the dense kernel's -- for every output element
// the same additions in the same order (incidence j + u * NS + slot to slot `slot`, acc = fmaf(1, v, acc) from +0 in incidence order,
// the xor-shuffle slot sum).  A gather is one contiguous 256-byte access per slot (8 bytes per lane: two lines).  The row then goes
// through LDS and every lane reads the mask back (one broadcast 16-byte read).  Lane li owns columns li, li + 32, li + 64, li + 96 --
// bit li of each of the four mask dwords, not four neighbouring columns: the position of column li + 32 g is then (values of the dwords
// below g) + popcount(dword g below bit li), two instructions, where neighbouring columns cost a rank inside the lane's nibble and a
// select per column (measured: 75 vector instructions per gathered row pair and 1.02 ms per pass, vector-issue bound).
// An empty column reads some dword and masks it to +0.  Rows above kPackCap occupied columns are read from the dense table in a branch
// the wave takes only when a row of the step needs it.
constexpr int kImagePad = 128;           // a position is at most 4 + 127: reads nobody uses may run this far past the last image
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void segreduce_packed_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const uint32_t* __restrict__ packed,
    const float* __restrict__ x, int64_t ldx, float* __restrict__ out, int64_t ldo, int n_t, int mean,
    const int32_t* __restrict__ row_order) {
  constexpr int VEC = 4, LPR = 32, NS = 2, U = kUnroll;
  __shared__ __attribute__((aligned(16))) uint32_t image[kWavesPerBlock * U * NS * kPackPitchDw + kImagePad];      // 16.5 KiB
  const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int slot_row = static_cast<int>(blk) * kWavesPerBlock + (threadIdx.x >> 6);
  if (slot_row >= n_t) return;  // whole wave exits together
  const int row = row_order ? row_order[slot_row] : slot_row;
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const int slot = lane / LPR, li = lane % LPR;
  const int start = rowptr[row], end = rowptr[row + 1];
  const uint32_t below = (1u << li) - 1u;
  uint32_t* const mine = image + (wave * U * NS + slot) * kPackPitchDw;       // image of gather u: mine + u * NS * kPackPitchDw
  float acc[VEC];                                                             // acc[g]: column li + 32 g
#pragma unroll
  for (int g = 0; g < VEC; ++g) acc[g] = 0.f;

  for (int base = start; base < end; base += kWave) {
    const int n = min(kWave, end - base);
    int my_col = 0;
    if (lane < n) my_col = col[base + lane];
    for (int j = 0; j < n; j += NS * U) {
      uint2 raw[U];               // kept packed while in flight (8 B per lane and load)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int jj = j + u * NS + slot;
        const int src = __shfl(my_col, jj & (kWave - 1));
        if (jj < n) raw[u] = *reinterpret_cast<const uint2*>(packed + static_cast<int64_t>(src) * kPackPitchDw + 2 * li);
        else raw[u] = make_uint2(0u, 0u);                            // an empty mask: the row expands to zeros
      }
#pragma unroll
      for (int u = 0; u < U; ++u) *reinterpret_cast<uint2*>(mine + u * NS * kPackPitchDw + 2 * li) = raw[u];
      lds_wave_handoff();
      // expanded kExpand rows at a time: their mask reads, then their value reads, are independent LDS operations in flight together
#pragma unroll
      for (int u0 = 0; u0 < U; u0 += kExpand) {
        if (j + u0 * NS >= n) break;                                 // wave-uniform: nothing but empty images from here on (exact: they add +0)
        uint4 m[kExpand];
#pragma unroll
        for (int e = 0; e < kExpand; ++e) m[e] = *reinterpret_cast<const uint4*>(mine + (u0 + e) * NS * kPackPitchDw);
        uint32_t v[kExpand][VEC];
        bool over[kExpand];
        bool any_over = false;
#pragma unroll
        for (int e = 0; e < kExpand; ++e) {
          const uint32_t* r = mine + (u0 + e) * NS * kPackPitchDw;
          const int c1 = 4 + __popc(m[e].x), c2 = c1 + __popc(m[e].y), c3 = c2 + __popc(m[e].z);
          over[e] = c3 + __popc(m[e].w) > 4 + kPackCap;              // uniform over the slot: every lane of it read the same mask
          any_over |= over[e];
          v[e][0] = r[4 + __popc(m[e].x & below)] & all_ones_if_bit(m[e].x, li);
          v[e][1] = r[c1 + __popc(m[e].y & below)] & all_ones_if_bit(m[e].y, li);
          v[e][2] = r[c2 + __popc(m[e].z & below)] & all_ones_if_bit(m[e].z, li);
          v[e][3] = r[c3 + __popc(m[e].w & below)] & all_ones_if_bit(m[e].w, li);
        }
        if (__any(any_over)) {                                       // wave-uniform, rare: a row did not fit, read it dense
#pragma unroll
          for (int e = 0; e < kExpand; ++e) {
            const int src = __shfl(my_col, (j + (u0 + e) * NS + slot) & (kWave - 1));
            if (over[e]) {
              const uint32_t* xr = reinterpret_cast<const uint32_t*>(x + static_cast<int64_t>(src) * ldx) + li;
#pragma unroll
              for (int g = 0; g < VEC; ++g) v[e][g] = xr[32 * g];
            }
          }
        }
#pragma unroll
        for (int e = 0; e < kExpand; ++e)
#pragma unroll
          for (int g = 0; g < VEC; ++g) acc[g] = fmaf(1.f, __uint_as_float(v[e][g]), acc[g]);   // a skipped zero is an exact no-op of this sum
      }
      lds_wave_handoff();                                            // the next step's images overwrite these
    }
  }

#pragma unroll
  for (int off = LPR; off < kWave; off <<= 1)
#pragma unroll
    for (int g = 0; g < VEC; ++g) acc[g] += __shfl_xor(acc[g], off);

  if (slot == 0) {
    const float scale = mean ? 1.f / static_cast<float>(max(end - start, 1)) : 1.f;
    float* o = out + static_cast<int64_t>(row) * ldo + li;
#pragma unroll
    for (int g = 0; g < VEC; ++g) o[32 * g] = acc[g] * scale;        // four stores of one 128-byte line each
  }
}

// ---- cell rows (include/allset_hip_ext.h: 16 cells of {v0, v1, v2, {col0, col1, col2, k}}, 256 bytes per row) ------------------------
// The mask format's expansion pays for all 128 columns of a gathered row (a popcount, an LDS read at a computed address, a sign extract,
// an AND per column: about 45 vector instructions per row pair).  A cell row carries each occupied element's
// column beside it, so the lane that loaded a cell scatters the three values it holds into a dense LDS image of the row -- a byte
// extract, an address and one ds_write_b32 each -- and the row is read back dense: the cost follows the occupied elements.
#ifndef ALLSET_CELL_WAVES           // waves per SIMD the gather's registers are held to (8 images: LDS allows 8; 16 images: 4)
#define ALLSET_CELL_WAVES 8
#endif
constexpr int kCellImageDw = 128 + kCellsPerRow;       // a row's image: its 128 columns + one pad dword per cell (the dummy columns)

// segreduce_kernel<float, 4, 32, kModeSum, false> over cell rows: the wave-per-row mapping, block remap, row_order and 64-incidence column
// batches of segreduce_packed_kernel, and -- so that the result is BITWISE the dense kernel's -- for every output element the same
// additions in the same order.  A load instruction gathers FOUR rows (16 lanes x 16 bytes: lane >> 4 the row, lane & 15 the cell); Q of
// them are in flight per step (4 Q incidences) and go through LDS H at a time.  Incidence i of the step owns image i % (4 H), which is image
// (u, slot) = (i >> 1, i & 1) of the dense kernel's assignment jj = j + u * NS + slot.  The images are zero between sub-steps: the lane that
// holds a cell writes its three values at their columns (an unused slot's dummy column is a pad dword of its own), lane (slot, li) reads
// columns 4 li .. 4 li + 3 of its slot's images in u order -- every dword of them is the dense row's, occupied or +0, and an image nobody
// wrote adds +0 as the dense kernel's tail does -- and the writers clear what they wrote.  A row above kCellCap occupied columns is copied,
// dense, from the side table into its image, in a branch the wave takes only when a row of the step needs it.
// acc = fmaf(1, v, acc) as the dense kernel's machine code performs it: v_add_f32 with the gathered value as the FIRST operand.  The sum
// is the same either way, the bits of a NaN are not: where two NaNs meet (Inf - Inf earlier in the row gives 0xffc00000, a gathered NaN
// is usually 0x7fc00000) the instruction returns its first operand's, and "bitwise the dense kernel's" includes that.  The compiler
// commutes a plain addition as it pleases, hence the instruction by name.
__device__ __forceinline__ float add_value_first(uint32_t v, float acc) {
  float r;
  asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(v), "v"(acc));
  return r;
}

template <int Q, int H>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ALLSET_CELL_WAVES, ALLSET_CELL_WAVES))) void segreduce_cells_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const uint4* __restrict__ cells,
    const float* __restrict__ x, int64_t ldx, float* __restrict__ out, int64_t ldo, int n_t, int mean,
    const int32_t* __restrict__ row_order) {
  static_assert(Q % H == 0, "whole sub-steps");
  constexpr int NI = 4 * H;                                           // images per wave: 8 -> 4.5 KiB, 18 KiB per workgroup
  __shared__ __attribute__((aligned(16))) uint32_t image[kWavesPerBlock * NI * kCellImageDw];
  const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int slot_row = static_cast<int>(blk) * kWavesPerBlock + (threadIdx.x >> 6);
  if (slot_row >= n_t) return;  // whole wave exits together
  const int row = row_order ? row_order[slot_row] : slot_row;
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const int r4 = lane >> 4, cell = lane & 15;                         // as a loader: row of the instruction, cell of the row
  const int slot = lane >> 5, li = lane & 31;                         // as a reader: the dense kernel's slot and 16-byte column group
  const int start = rowptr[row], end = rowptr[row + 1];
  uint32_t* const wimg = image + wave * NI * kCellImageDw;
  for (int i = lane; i < NI * kCellImageDw / 4; i += kWave) reinterpret_cast<uint4*>(wimg)[i] = make_uint4(0u, 0u, 0u, 0u);
  uint32_t* const wr = wimg + r4 * kCellImageDw;                      // image of load h of a sub-step: wr + 4 h * kCellImageDw
  const uint32_t* const rd = wimg + slot * kCellImageDw + 4 * li;     // image (u, slot): rd + 2 u * kCellImageDw
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  lds_wave_handoff();

  for (int base = start; base < end; base += kWave) {
    const int n = min(kWave, end - base);
    int my_col = 0;
    if (lane < n) my_col = col[base + lane];
    for (int j = 0; j < n; j += 4 * Q) {
      uint4 raw[Q];
      uint32_t meta[Q];
      bool ok[Q];
      {
        int src[Q];                                                  // (the shuffles first: the loads then leave back to back)
#pragma unroll
        for (int q = 0; q < Q; ++q) src[q] = __shfl(my_col, (j + 4 * q + r4) & (kWave - 1));
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          ok[q] = j + 4 * q + r4 < n;                                // past the end: neither loaded nor scattered
          meta[q] = 0u;                                              // (k = 0)
          if (ok[q]) {
            raw[q] = cells[static_cast<int64_t>(src[q]) * kCellsPerRow + cell];
            meta[q] = raw[q].w;
          }
        }
      }
#pragma unroll
      for (int q0 = 0; q0 < Q; q0 += H) {
        if (q0 > 0 && j + 4 * q0 >= n) break;                        // wave-uniform: nothing was loaded from here on
        bool over[H];
        bool any_over = false;
#pragma unroll
        for (int h = 0; h < H; ++h) {
          uint32_t* im = wr + 4 * h * kCellImageDw;
          const uint32_t m = meta[q0 + h];
          over[h] = (m >> 24) > static_cast<uint32_t>(kCellCap);
          any_over |= over[h];
          if (ok[q0 + h]) {
            im[m & 0xffu] = raw[q0 + h].x;
            im[(m >> 8) & 0xffu] = raw[q0 + h].y;
            im[(m >> 16) & 0xffu] = raw[q0 + h].z;
          }
        }
        any_over = __any(any_over);
        if (any_over) {                                              // wave-uniform, rare: a row did not fit, its image is the dense row
#pragma unroll
          for (int h = 0; h < H; ++h) {
            const int src = __shfl(my_col, (j + 4 * (q0 + h) + r4) & (kWave - 1));
            if (over[h]) {
              const uint4* xr = reinterpret_cast<const uint4*>(x + static_cast<int64_t>(src) * ldx) + cell;
              uint4* im = reinterpret_cast<uint4*>(wr + 4 * h * kCellImageDw) + cell;
              im[0] = xr[0];
              im[16] = xr[16];
            }
          }
        }
        lds_wave_handoff();
#pragma unroll
        for (int u0 = 0; u0 < 2 * H; u0 += 2) {                      // two reads in flight (registers: 8 waves per SIMD need <= 64)
          uint4 v[2];
#pragma unroll
          for (int e = 0; e < 2; ++e) v[e] = *reinterpret_cast<const uint4*>(rd + 2 * (u0 + e) * kCellImageDw);
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            acc[0] = add_value_first(v[e].x, acc[0]);
            acc[1] = add_value_first(v[e].y, acc[1]);
            acc[2] = add_value_first(v[e].z, acc[2]);
            acc[3] = add_value_first(v[e].w, acc[3]);
          }
        }
        lds_wave_handoff();
        // the images are zero again for the next sub-step: every writer clears what it wrote
#ifdef ALLSET_CELL_ZERO16           // ablation builds only (tools/cell_gather_bench.py): 16-byte zero stores over the whole images instead
        for (int i = lane; i < NI * kCellImageDw / 4; i += kWave) reinterpret_cast<uint4*>(wimg)[i] = make_uint4(0u, 0u, 0u, 0u);
#else
#pragma unroll
        for (int h = 0; h < H; ++h) {
          uint32_t* im = wr + 4 * h * kCellImageDw;
          const uint32_t m = meta[q0 + h];
          if (ok[q0 + h]) {
            im[m & 0xffu] = 0u;
            im[(m >> 8) & 0xffu] = 0u;
            im[(m >> 16) & 0xffu] = 0u;
          }
        }
        if (any_over) {
#pragma unroll
          for (int h = 0; h < H; ++h) {
            if (over[h]) {
              uint4* im = reinterpret_cast<uint4*>(wr + 4 * h * kCellImageDw) + cell;
              im[0] = make_uint4(0u, 0u, 0u, 0u);
              im[16] = make_uint4(0u, 0u, 0u, 0u);
            }
          }
        }
#endif
        lds_wave_handoff();
      }
    }
  }

#pragma unroll
  for (int g = 0; g < 4; ++g) acc[g] = add_value_first(__float_as_uint(acc[g]), __shfl_xor(acc[g], 32));     // (own sum first, as there)

  if (slot == 0) {
    const float scale = mean ? 1.f / static_cast<float>(max(end - start, 1)) : 1.f;
    int lo = lane;
    asm volatile("" : "+v"(lo));                                     // the store's offset is formed here, not kept in registers across the loop
    *reinterpret_cast<float4*>(out + static_cast<int64_t>(row) * ldo + 4 * lo) =
        make_float4(acc[0] * scale, acc[1] * scale, acc[2] * scale, acc[3] * scale);
  }
}

// ---- host-side dispatch ------------------------------------------------------------------------

template <typename T, int VEC, int LPR>
static void launch_segreduce(int mode_ext, bool weighted, unsigned grid, hipStream_t st,
                             const int32_t* rowptr, const int32_t* col, const float* w, const T* x,
                             int64_t ldx, T* out, int64_t ldo, int32_t* argext, int n_t, int d, int mean,
                             float sign, const int32_t* row_order) {
  if (!mode_ext) {
    if (weighted) segreduce_kernel<T, VEC, LPR, kModeSum, true><<<grid, kBlock, 0, st>>>(rowptr, col, w, x, ldx, out, ldo, argext, n_t, d, mean, sign, row_order);
    else          segreduce_kernel<T, VEC, LPR, kModeSum, false><<<grid, kBlock, 0, st>>>(rowptr, col, w, x, ldx, out, ldo, argext, n_t, d, mean, sign, row_order);
  } else {
    if (weighted) segreduce_kernel<T, VEC, LPR, kModeExt, true><<<grid, kBlock, 0, st>>>(rowptr, col, w, x, ldx, out, ldo, argext, n_t, d, mean, sign, row_order);
    else          segreduce_kernel<T, VEC, LPR, kModeExt, false><<<grid, kBlock, 0, st>>>(rowptr, col, w, x, ldx, out, ldo, argext, n_t, d, mean, sign, row_order);
  }
}

// short-row path: sum/mean, 16-byte packets, the whole row in one column chunk
template <typename T, int WIDE>
static void dispatch_flat(bool weighted, hipStream_t st, const int32_t* rowptr, const int32_t* col, const float* w,
                          const T* x, int64_t ldx, T* out, int64_t ldo, int n_t, int d, int mean) {
  with_lpr(pick_lpr(d, WIDE), [&](auto lpr) {
    const unsigned grid = flat_grid<lpr()>(n_t);
    if (weighted) segreduce_flat_kernel<T, WIDE, lpr(), true><<<grid, kBlock, 0, st>>>(rowptr, col, w, x, ldx, out, ldo, n_t, d, mean);
    else          segreduce_flat_kernel<T, WIDE, lpr(), false><<<grid, kBlock, 0, st>>>(rowptr, col, w, x, ldx, out, ldo, n_t, d, mean);
  });
}

template <typename T, int WIDE>
static void dispatch_segreduce(bool wide_ok, int mode_ext, bool weighted, unsigned grid, hipStream_t st,
                               const int32_t* rowptr, const int32_t* col, const float* w, const T* x, int64_t ldx,
                               T* out, int64_t ldo, int32_t* argext, int n_t, int d, int mean, float sign,
                               const int32_t* row_order) {
  with_vec_lpr<WIDE>(wide_ok, d, ALLSET_SEG_MAX_LPR, [&](auto vec, auto lpr) {
    launch_segreduce<T, vec(), lpr()>(mode_ext, weighted, grid, st, rowptr, col, w, x, ldx, out, ldo, argext, n_t, d, mean, sign, row_order);
  });
}

template <int VEC, int LPR>
static void launch_segmax_bwd(bool weighted, unsigned grid, hipStream_t st, const int32_t* rowptrT,
                              const int32_t* colT, const int32_t* posT, const float* wT, const int32_t* argext,
                              const float* gout, int64_t ldg, float* gx, int64_t ldx, int n_s, int d) {
  if (weighted) segmax_bwd_kernel<VEC, LPR, true><<<grid, kBlock, 0, st>>>(rowptrT, colT, posT, wT, argext, gout, ldg, gx, ldx, n_s, d);
  else          segmax_bwd_kernel<VEC, LPR, false><<<grid, kBlock, 0, st>>>(rowptrT, colT, posT, wT, argext, gout, ldg, gx, ldx, n_s, d);
}

}  // namespace allset

using namespace allset;

static int segreduce_impl(int reduce, int dtype, int variant, int64_t nnz_hint, const int32_t* row_order,
                          const int32_t* rowptr, const int32_t* col,
                          const float* w, const void* x, int64_t ldx, void* out, int64_t ldo,
                          int32_t* argext, int64_t n_t, int64_t n_s, int64_t d, void* stream);

extern "C" int allset_segreduce_fwd(int reduce, int dtype, const int32_t* rowptr, const int32_t* col,
                                    const float* w, const void* x, int64_t ldx, void* out, int64_t ldo,
                                    int32_t* argext, int64_t n_t, int64_t n_s, int64_t d, void* stream) {
  return segreduce_impl(reduce, dtype, 0, -1, nullptr, rowptr, col, w, x, ldx, out, ldo, argext, n_t, n_s, d, stream);
}

extern "C" int allset_segreduce_fwd_ex(int reduce, int dtype, int variant, int64_t nnz, const int32_t* row_order,
                                       const int32_t* rowptr, const int32_t* col, const float* w, const void* x,
                                       int64_t ldx, void* out, int64_t ldo, int32_t* argext, int64_t n_t, int64_t n_s,
                                       int64_t d, void* stream) {
  return segreduce_impl(reduce, dtype, variant, nnz, row_order, rowptr, col, w, x, ldx, out, ldo, argext, n_t, n_s, d, stream);
}

static int segreduce_impl(int reduce, int dtype, int variant, int64_t nnz_hint, const int32_t* row_order,
                          const int32_t* rowptr, const int32_t* col,
                          const float* w, const void* x, int64_t ldx, void* out, int64_t ldo,
                          int32_t* argext, int64_t n_t, int64_t n_s, int64_t d, void* stream) {
  clear_error();
  ALLSET_REQUIRE(variant >= 0 && variant <= 2, "segreduce_fwd: bad variant %d", variant);
  ALLSET_REQUIRE(reduce >= ALLSET_SUM && reduce <= ALLSET_MIN, "segreduce_fwd: bad reduce %d", reduce);
  ALLSET_REQUIRE(n_t >= 0 && n_s >= 0 && d >= 0, "segreduce_fwd: negative size");
  ALLSET_REQUIRE(n_t < INT32_MAX && n_s < INT32_MAX && d < INT32_MAX, "segreduce_fwd: size exceeds int32");
  ALLSET_REQUIRE(dtype == ALLSET_F32 || dtype == ALLSET_BF16, "segreduce_fwd: bad dtype %d", dtype);
  if (n_t == 0 || d == 0) return ALLSET_OK;
  ALLSET_REQUIRE(rowptr && out, "segreduce_fwd: null rowptr/out");
  ALLSET_REQUIRE(ldx >= d && ldo >= d, "segreduce_fwd: leading dimension smaller than d");
  // col/x may only be null when there is nothing to gather; without the caller's nnz that cannot be known (no sync
  // here), so require them whenever a source table is declared -- unless nnz == 0 was stated (the _ex entry).
  ALLSET_REQUIRE(n_s == 0 || nnz_hint == 0 || (col && x), "segreduce_fwd: null col/x with n_s > 0");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const bool ext = (reduce == ALLSET_MAX || reduce == ALLSET_MIN);
  const float sign = (reduce == ALLSET_MIN) ? -1.f : 1.f;
  const int mean = (reduce == ALLSET_MEAN);
  const int wide = dtype == ALLSET_F32 ? 4 : 8;                       // elements in a 16-byte packet
  const bool wide_ok = (d % wide == 0) && (ldx % wide == 0) && (ldo % wide == 0) && aligned16(x) && aligned16(out) &&
                       (argext == nullptr || aligned16(argext));
  const unsigned grid = row_grid(n_t);
  const int nt = static_cast<int>(n_t), di = static_cast<int>(d);
  // variant: 0 = AUTO (short-row kernel when the caller's nnz says the mean degree is small), 1 = one wave per row,
  // 2 = short-row kernel.  The short-row kernel needs sum/mean, 16-byte packets and d <= 64 packets.
  const bool flat_ok = !ext && wide_ok && d <= 64 * wide;
  // (AUTO at dataset scale -- every row gets its own lane group on a machine this size anyway: the one-group-per-row kernel is one
  //  dependent round trip shorter than a slot walking seven rows as a stream, and the step there is a chain of such latencies)
  const bool use_flat = flat_ok && (variant == 2 || (variant == 0 && nnz_hint >= 0 && n_t > kFlatMinRows &&
                                                     static_cast<double>(nnz_hint) < kFlatMaxMeanDegree * static_cast<double>(n_t)));
  if (variant == 2 && !flat_ok) {
    set_error("segreduce_fwd: the short-row variant needs sum/mean, 16-byte aligned rows and d <= %d", 64 * wide);
    return ALLSET_ERR_UNSUPPORTED;
  }
  if (use_flat) {
    if (dtype == ALLSET_F32)
      dispatch_flat<float, 4>(w != nullptr, st, rowptr, col, w, static_cast<const float*>(x), ldx, static_cast<float*>(out), ldo, nt, di, mean);
    else
      dispatch_flat<bf16_t, 8>(w != nullptr, st, rowptr, col, w, static_cast<const bf16_t*>(x), ldx, static_cast<bf16_t*>(out), ldo, nt, di, mean);
    ALLSET_LAUNCH_CHECK();
    return ALLSET_OK;
  }
  if (dtype == ALLSET_F32)
    dispatch_segreduce<float, 4>(wide_ok, ext, w != nullptr, grid, st, rowptr, col, w, static_cast<const float*>(x), ldx,
                                 static_cast<float*>(out), ldo, argext, nt, di, mean, sign, row_order);
  else
    dispatch_segreduce<bf16_t, 8>(wide_ok, ext, w != nullptr, grid, st, rowptr, col, w, static_cast<const bf16_t*>(x), ldx,
                                  static_cast<bf16_t*>(out), ldo, argext, nt, di, mean, sign, row_order);
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_segmax_bwd(const int32_t* rowptrT, const int32_t* colT, const int32_t* posT,
                                 const float* wT, const int32_t* argext, const float* gout, int64_t ldg,
                                 float* gx, int64_t ldx, int64_t n_s, int64_t n_t, int64_t d, void* stream) {
  clear_error();
  ALLSET_REQUIRE(n_t >= 0 && n_s >= 0 && d >= 0, "segmax_bwd: negative size");
  ALLSET_REQUIRE(n_t < INT32_MAX && n_s < INT32_MAX && d < INT32_MAX, "segmax_bwd: size exceeds int32");
  if (n_s == 0 || d == 0) return ALLSET_OK;
  ALLSET_REQUIRE(rowptrT && gx, "segmax_bwd: null rowptrT/gx");
  ALLSET_REQUIRE(n_t == 0 || (colT && posT && argext && gout), "segmax_bwd: null input with n_t > 0");
  ALLSET_REQUIRE(ldg >= d && ldx >= d, "segmax_bwd: leading dimension smaller than d");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const bool vec4 = (d % 4 == 0) && (ldg % 4 == 0) && (ldx % 4 == 0) && aligned16(gout) && aligned16(gx);
  const unsigned grid = row_grid(n_s);
  const int ns = static_cast<int>(n_s), di = static_cast<int>(d);
  with_vec_lpr<4>(vec4, d, [&](auto vec, auto lpr) {
    launch_segmax_bwd<vec(), lpr()>(wT != nullptr, grid, st, rowptrT, colT, posT, wT, argext, gout, ldg, gx, ldx, ns, di);
  });
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_sddmm_rowdot(int reduce, const int32_t* rowptr, const int32_t* col, const float* x,
                                   int64_t ldx, const float* gout, int64_t ldg, const int32_t* argext,
                                   float* gw, int64_t n_t, int64_t n_s, int64_t d, void* stream) {
  clear_error();
  ALLSET_REQUIRE(reduce >= ALLSET_SUM && reduce <= ALLSET_MIN, "sddmm_rowdot: bad reduce %d", reduce);
  ALLSET_REQUIRE(n_t >= 0 && n_s >= 0 && d >= 0, "sddmm_rowdot: negative size");
  ALLSET_REQUIRE(n_t < INT32_MAX && n_s < INT32_MAX && d < INT32_MAX, "sddmm_rowdot: size exceeds int32");
  if (n_t == 0 || n_s == 0) return ALLSET_OK;
  ALLSET_REQUIRE(rowptr && col && x && gout && gw, "sddmm_rowdot: null pointer");
  ALLSET_REQUIRE(ldx >= d && ldg >= d, "sddmm_rowdot: leading dimension smaller than d");
  const bool ext = (reduce == ALLSET_MAX || reduce == ALLSET_MIN);
  ALLSET_REQUIRE(!ext || argext, "sddmm_rowdot: MAX/MIN need argext");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned grid = row_grid(n_t);
  const int mean = (reduce == ALLSET_MEAN);
  const int nt = static_cast<int>(n_t), di = static_cast<int>(d);
  // 16-byte path: one column block (d <= 256), aligned rows; anything else takes the scalar kernel
  const bool vec4 = (d % 4 == 0) && d <= 256 && (ldx % 4 == 0) && (ldg % 4 == 0) && aligned16(x) && aligned16(gout) &&
                    (!ext || aligned16(argext));
  if (vec4) {
    with_lpr(pick_lpr(d), [&](auto lpr) {
      if (ext) sddmm_rowdot_vec_kernel<lpr(), kModeExt><<<grid, kBlock, 0, st>>>(rowptr, col, x, ldx, gout, ldg, argext, gw, nt, di, mean);
      else     sddmm_rowdot_vec_kernel<lpr(), kModeSum><<<grid, kBlock, 0, st>>>(rowptr, col, x, ldx, gout, ldg, nullptr, gw, nt, di, mean);
    });
  } else if (ext) {
    sddmm_rowdot_kernel<kModeExt><<<grid, kBlock, 0, st>>>(rowptr, col, x, ldx, gout, ldg, argext, gw, nt, di, mean);
  } else {
    sddmm_rowdot_kernel<kModeSum><<<grid, kBlock, 0, st>>>(rowptr, col, x, ldx, gout, ldg, nullptr, gw, nt, di, mean);
  }
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

static inline bool aligned256(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 255u) == 0; }

// ---- the two packed formats' entry points: one body each, the exported name for the messages, the format for the kernel ------------
static int pack_impl(const char* fn, bool cells, const float* x, int64_t ldx, void* packed, int64_t n, int64_t d, void* stream) {
  clear_error();
  ALLSET_REQUIRE(n >= 0 && d >= 0, "%s: negative size", fn);
  ALLSET_REQUIRE(n < INT32_MAX, "%s: size exceeds int32", fn);
  if (d != 128) {
    set_error("%s: built for d = 128 only (got %lld)", fn, static_cast<long long>(d));
    return ALLSET_ERR_UNSUPPORTED;
  }
  if (n == 0) return ALLSET_OK;
  ALLSET_REQUIRE(x && packed, "%s: null x/packed", fn);
  ALLSET_REQUIRE(ldx >= d && ldx % 4 == 0 && aligned16(x), "%s: rows of x must be 16-byte aligned (pointer and leading dimension)", fn);
  ALLSET_REQUIRE(aligned256(packed), "%s: the packed buffer must be 256-byte aligned", fn);
  const int64_t rows_per_block = static_cast<int64_t>(kWavesPerBlock) * kPackRowsPerWave;
  const unsigned grid = static_cast<unsigned>((n + rows_per_block - 1) / rows_per_block);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (cells) pack_kernel<true><<<grid, kBlock, 0, st>>>(x, ldx, static_cast<uint32_t*>(packed), n);
  else       pack_kernel<false><<<grid, kBlock, 0, st>>>(x, ldx, static_cast<uint32_t*>(packed), n);
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

// segreduce_cells_kernel: load instructions (four rows each) in flight per step, and how many of them go through LDS together;
// tools/cell_gather_bench.py rebuilds with other values
#ifndef ALLSET_CELL_LOADS
#define ALLSET_CELL_LOADS 4
#endif
#ifndef ALLSET_CELL_SUBSTEP
#define ALLSET_CELL_SUBSTEP 2
#endif

static int segreduce_packed_impl(const char* fn, bool cells, int reduce, const int32_t* row_order, const int32_t* rowptr, const int32_t* col,
                                 const void* packed, const float* x, int64_t ldx, float* out, int64_t ldo, int64_t n_t, int64_t n_s,
                                 int64_t d, void* stream) {
  clear_error();
  ALLSET_REQUIRE(reduce == ALLSET_SUM || reduce == ALLSET_MEAN, "%s: reduce must be SUM or MEAN (got %d)", fn, reduce);
  ALLSET_REQUIRE(n_t >= 0 && n_s >= 0 && d >= 0, "%s: negative size", fn);
  ALLSET_REQUIRE(n_t < INT32_MAX && n_s < INT32_MAX, "%s: size exceeds int32", fn);
  if (d != 128) {
    set_error("%s: built for d = 128 only (got %lld)", fn, static_cast<long long>(d));
    return ALLSET_ERR_UNSUPPORTED;
  }
  if (n_t == 0) return ALLSET_OK;
  ALLSET_REQUIRE(rowptr && out, "%s: null rowptr/out", fn);
  ALLSET_REQUIRE(n_s == 0 || (col && packed && x), "%s: null col/packed/x with n_s > 0", fn);
  ALLSET_REQUIRE(ldx >= d && ldo >= d && ldx % 4 == 0 && ldo % 4 == 0 && aligned16(x) && aligned16(out),
                 "%s: rows of x and out must be 16-byte aligned (pointers and leading dimensions)", fn);
  ALLSET_REQUIRE(aligned256(packed), "%s: the packed buffer must be 256-byte aligned", fn);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int nt = static_cast<int>(n_t), mean = reduce == ALLSET_MEAN;
  if (cells) segreduce_cells_kernel<ALLSET_CELL_LOADS, ALLSET_CELL_SUBSTEP><<<row_grid(n_t), kBlock, 0, st>>>(
                 rowptr, col, static_cast<const uint4*>(packed), x, ldx, out, ldo, nt, mean, row_order);
  else       segreduce_packed_kernel<<<row_grid(n_t), kBlock, 0, st>>>(
                 rowptr, col, static_cast<const uint32_t*>(packed), x, ldx, out, ldo, nt, mean, row_order);
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_pack_rows_f32(const float* x, int64_t ldx, void* packed, int64_t n, int64_t d, void* stream) {
  return pack_impl("pack_rows_f32", false, x, ldx, packed, n, d, stream);
}

extern "C" int allset_pack_cells_f32(const float* x, int64_t ldx, void* cells, int64_t n, int64_t d, void* stream) {
  return pack_impl("pack_cells_f32", true, x, ldx, cells, n, d, stream);
}

extern "C" int allset_segreduce_packed_fwd(int reduce, const int32_t* row_order, const int32_t* rowptr, const int32_t* col,
                                           const void* packed, const float* x, int64_t ldx, float* out, int64_t ldo, int64_t n_t,
                                           int64_t n_s, int64_t d, void* stream) {
  return segreduce_packed_impl("segreduce_packed_fwd", false, reduce, row_order, rowptr, col, packed, x, ldx, out, ldo, n_t, n_s, d, stream);
}

extern "C" int allset_segreduce_cells_fwd(int reduce, const int32_t* row_order, const int32_t* rowptr, const int32_t* col,
                                          const void* cells, const float* x, int64_t ldx, float* out, int64_t ldo, int64_t n_t,
                                          int64_t n_s, int64_t d, void* stream) {
  return segreduce_packed_impl("segreduce_cells_fwd", true, reduce, row_order, rowptr, col, cells, x, ldx, out, ldo, n_t, n_s, d, stream);
}
