// The short-row ("flat") CSR walk shared by segreduce_flat_kernel, pma_fwd_flat_kernel, pma_bwd_src_flat_kernel,
// unigcn_flat_kernel, unignn_flat_kernel and e2v_flat_kernel (hconv_flat_kernel follows the same scheme in its own text, see
// hconv.hip), and the launch helpers that pick a compile-time lanes-per-row for every CSR kernel of those files.
//
// One wave per row spends a wave launch and three dependent round trips (rowptr -> col -> gather) on every row; at
// degree <= 4 that overhead, not bandwidth, sets the time (profiles: 4M rows take ~1.6 ms whether they hold 1 or 4
// incidences).  Here each LPR-lane group ("slot") owns kFlatRows consecutive rows and walks their incidences as ONE
// stream: the rows' rowptr entries arrive in one load (lane i holds rowptr[r0+i]), the column ids of consecutive rows
// are contiguous in the CSR and arrive LPR at a time, the gathers of a batch are in flight together regardless of row
// boundaries, and a row is flushed (one coalesced store) whenever the stream crosses its end.  Slots never combine:
// everything that steers the walk is uniform within a slot, so its lanes reach every flush together and a flush may
// reduce across them.  The whole row sits in one column chunk (d <= LPR * VEC).
//
// A kernel keeps what is its own -- the unroll depth, the accumulators, the packets in flight and the flush body -- and
// hands them to flat_walk() as four callables; the slot geometry, the row advance and the stream walk live here only.
#pragma once

#include <type_traits>

#include "common.h"

namespace allset {

constexpr int kFlatRows = 7;       // rows per slot; kFlatRows + 1 rowptr entries must fit in the smallest slot (8 lanes)

// ---- launch helpers -----------------------------------------------------------------------------------------------------------
template <int LPR>
inline unsigned flat_grid(int64_t n_rows) {
  const int64_t rows_per_block = static_cast<int64_t>(kWavesPerBlock) * (kWave / LPR) * kFlatRows;
  return static_cast<unsigned>((n_rows + rows_per_block - 1) / rows_per_block);
}

template <int N>
using IntC = std::integral_constant<int, N>;

// pick_lpr()'s result as a compile-time constant: f(IntC<LPR>{}), to be used as `lpr()` in a template argument
template <class F>
inline void with_lpr(int lpr, F&& f) {
  switch (lpr) {
    case 8:  f(IntC<8>{}); break;
    case 16: f(IntC<16>{}); break;
    case 32: f(IntC<32>{}); break;
    default: f(IntC<64>{}); break;
  }
}

// The (VEC, LPR) pair of a wave-per-row kernel: 16-byte packets of WIDE elements on pick_lpr() lanes when the rows allow
// them, one element per lane across the whole wave otherwise.  f(IntC<VEC>{}, IntC<LPR>{}).
template <int WIDE, class F>
inline void with_vec_lpr(bool wide_ok, int64_t d, int max_lpr, F&& f) {
  if (wide_ok) with_lpr(pick_lpr(d, WIDE, max_lpr), [&](auto lpr) { f(IntC<WIDE>{}, lpr); });
  else f(IntC<1>{}, IntC<64>{});
}
template <int WIDE, class F>
inline void with_vec_lpr(bool wide_ok, int64_t d, F&& f) { with_vec_lpr<WIDE>(wide_ok, d, 64, f); }

#ifdef __HIPCC__

// ---- one slot's view of its rows ----------------------------------------------------------------------------------------------
template <int LPR>
struct FlatSlot {
  static_assert(kFlatRows + 1 <= LPR, "a slot's rowptr entries are held one per lane");
  int slot, li, lane0;     // the slot's index in the wave; this lane's index in the slot; the slot's first lane
  int64_t first_row;       // of the slot, before clamping to the row count (int64: the last workgroup's slots may lie past 2^31)
  int r_begin, r_end;      // the slot's rows (empty beyond the last row)
  int rp;                  // lane i of the slot holds rowptr[r_begin + i], i = 0 .. r_end - r_begin
  int q0, q_end;           // the slot's stream: CSR positions [q0, q_end)
  int cur_row, cur_end;    // the row the stream is in, and the position where it ends

  // the lane geometry alone: which slot of the grid this lane is in, and that slot's first row
  __device__ __forceinline__ FlatSlot() {
    const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
    const int lane = lane_id();
    slot = lane / LPR;
    li = lane % LPR;
    lane0 = slot * LPR;
    const int64_t slot_global = (static_cast<int64_t>(blk) * kWavesPerBlock + (threadIdx.x >> 6)) * (kWave / LPR) + slot;
    first_row = slot_global * kFlatRows;
  }

  // The whole wave lies beyond the last row (its first slot does).  The kernel returns on this BEFORE open(), with the `return`
  // in the kernel body, so that no wave shuffles with some of its slots gone.
  __device__ __forceinline__ bool wave_beyond(int n_rows) const {
    return first_row - static_cast<int64_t>(slot) * kFlatRows >= n_rows;
  }

  __device__ __forceinline__ void open(const int32_t* __restrict__ rowptr, int n_rows) {
    r_begin = static_cast<int>(min(first_row, static_cast<int64_t>(n_rows)));
    r_end = min(r_begin + kFlatRows, n_rows);
    rp = (li <= r_end - r_begin) ? rowptr[r_begin + li] : 0;
    q0 = __shfl(rp, lane0);
    q_end = __shfl(rp, lane0 + (r_end - r_begin));
    cur_row = r_begin;
    cur_end = (r_begin < r_end) ? __shfl(rp, lane0 + 1) : q0;
  }

  // step to the next row (past the slot's last row the clamp re-reads an entry that nothing consumes)
  __device__ __forceinline__ void next_row() {
    ++cur_row;
    cur_end = __shfl(rp, lane0 + min(cur_row - r_begin + 1, LPR - 1));
  }

  // the value lane jj (mod LPR) of this slot holds
  template <class V>
  __device__ __forceinline__ V bcast(V v, int jj) const { return __shfl(v, lane0 + (jj & (LPR - 1))); }
};

// The walk over a slot's stream, U gathers in flight.  `active`: this lane holds columns of the row (c0 < d); the walk folds it into
// the gather's condition itself, so that a packet costs one branch.
//   stage(base, n)     the coalesced per-position loads of a batch: lane li takes position base + li when li < n
//   gather(u, jj, ok)  request packet u for position base + jj of the batch (s.bcast(staged, jj)); !ok -- the position is past the
//                      batch's end, or the lane holds no column (`active` false) -- request nothing and leave a zero
//   accum(u)           fold packet u into the current row
//   flush()            finish row s.cur_row, whose positions end at s.cur_end, and reset the row state; slot-uniform
//                      control flow, called for empty rows too
template <int U, int LPR, class Stage, class Gather, class Accum, class Flush>
__device__ __forceinline__ void flat_walk(FlatSlot<LPR>& s, bool active, Stage&& stage, Gather&& gather, Accum&& accum, Flush&& flush) {
  for (int base = s.q0; base < s.q_end; base += LPR) {
    const int n = min(LPR, s.q_end - base);
    stage(base, n);
    for (int j = 0; j < n; j += U) {
#pragma unroll
      for (int u = 0; u < U; ++u) gather(u, j + u, j + u < n && active);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int pos = base + j + u;
        if (j + u < n) {
          while (pos >= s.cur_end) { flush(); s.next_row(); }     // also steps over empty rows
          accum(u);
        }
      }
    }
  }
  while (s.cur_row < s.r_end) { flush(); s.next_row(); }          // last row and trailing empty rows
}

#endif  // __HIPCC__

}  // namespace allset
