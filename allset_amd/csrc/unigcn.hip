// The E->V hop of UniGCNII (reference models.py:911-996, UniGCNIIConv) with GCNII's initial-residual step in the same launch, for
// gfx950.  For every vertex row v of the vertex-major CSR (rows = vertices, col = hyperedges):
//   a        = degV[v] * sum_{j in row v} Xe[col_j, :]
//   t        = use_norm ? (||a||_2 > 0 ? 1 / ||a||_2 : 0) : 1                       -> t_out[v] when use_norm
//   Xi[v, :] = (1 - alpha) * t * a + alpha * x0[v, :]
// t is the reference's normalize_l2 scale (computed from the detached row, so a constant of the backward); an empty row gives
// a = 0 and Xi = alpha * x0.  The backward needs no kernel of its own: with r'[v] = (1 - alpha) * degV[v] * t[v],
// gXe = allset_hconv_fwd over the transposed CSR with r = r', and gx0 = alpha * gXi.
//
// Mapping: hconv.hip's, without the per-incidence scale and with the row tail in place of the epilogue:
//   * one wavefront OWNS a whole output row: LPR lanes x 16 B per feature row, NS = 64 / LPR hyperedge rows gathered per load; widths
//     above 256 take two 16-byte packets per lane (NCH = 2, LPR = 64), so d <= 512 stays in registers and the row norm is a
//     cross-lane reduction -- no second pass over the row, no atomics;
//   * the up-to-64 column ids of the row arrive in ONE coalesced load and are broadcast with ds_bpermute, 8 gathers (4 x 2 packets
//     at NCH = 2) in flight per slot;
//   * XCD-contiguous workgroup order, and the CSR's long-rows-first order (row_order) when the caller has one;
//   * a short-row variant (kFlatRows consecutive rows per LPR-lane group, one stream of incidences; d <= 256) below a mean degree of
//     6: the lane group owns its rows, the norm is reduced over the group's lanes.
// Built for fp32, d a multiple of 4 up to 512, 16-byte aligned rows (anything else: ALLSET_ERR_UNSUPPORTED, the caller composes the
// hop from allset_hconv_fwd).
// Algorithmic bytes per launch: those of allset_hconv_fwd without r, nnz * (4d + 4) + (n_t + 1) * 4 + n_t * 4d, plus one read of
// x0, n_t * 4d (and n_t * 4 each for degV and t_out).
#include "common.h"
#include "flat_rows.h"

namespace allset {
namespace unigcn {

constexpr int kMaxWidth = 512;
constexpr int kFlatUnroll = 8;

struct Tail {
  const float* degV;      // per output row, or NULL (= ones)
  const float* x0;
  int64_t ldx0;
  float* t_out;           // per output row; written when use_norm
  float alpha;
  int use_norm;
};

// The row tail for the LPR lanes that together hold row `row`: lane li has columns (ch * LPR + li) * 4 .. + 3 of the gathered sum in
// acc[ch] (zeros beyond d).  Every lane of the group calls it (the norm is reduced across them); `writer` lanes store.
template <int LPR, int NCH>
__device__ __forceinline__ void finish_row(const Tail& tl, int row, int li, int d, float (&acc)[NCH][4], float* __restrict__ xi,
                                           int64_t ldxi, bool writer) {
  const float dv = tl.degV ? tl.degV[row] : 1.f;
  float ss = 0.f;
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      acc[ch][k] *= dv;
      ss = fmaf(acc[ch][k], acc[ch][k], ss);
    }
  float t = 1.f;
  if (tl.use_norm) {
#pragma unroll
    for (int off = 1; off < LPR; off <<= 1) ss += __shfl_xor(ss, off);
    t = ss > 0.f ? 1.f / sqrtf(ss) : 0.f;
  }
  if (!writer) return;
  if (tl.use_norm && li == 0) tl.t_out[row] = t;
  const float sa = (1.f - tl.alpha) * t;
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int c0 = (ch * LPR + li) * 4;
    if (c0 < d) {
      const FVec<4> z = load_vec<float, 4>(tl.x0 + static_cast<int64_t>(row) * tl.ldx0 + c0);
      FVec<4> o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o.v[k] = fmaf(sa, acc[ch][k], tl.alpha * z.v[k]);
      store_vec<float, 4>(xi + static_cast<int64_t>(row) * ldxi + c0, o);
    }
  }
}

template <int LPR, int NCH>
__global__ __launch_bounds__(kBlock) void unigcn_hop_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ xe, int64_t ldxe, Tail tl,
    float* __restrict__ xi, int64_t ldxi, int n_t, int d, const int32_t* __restrict__ row_order) {
  static_assert(NCH == 1 || LPR == kWave, "two packets per lane only with the whole wave on one row");
  constexpr int NS = kWave / LPR;
  constexpr int U = NCH == 1 ? 8 : 4;
  const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int slot_row = static_cast<int>(blk) * kWavesPerBlock + (threadIdx.x >> 6);
  if (slot_row >= n_t) return;  // whole wave exits together
  const int row = row_order ? row_order[slot_row] : slot_row;
  const int lane = lane_id();
  const int slot = lane / LPR, li = lane % LPR;
  const int start = rowptr[row], end = rowptr[row + 1];

  float acc[NCH][4];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[ch][k] = 0.f;

  for (int base = start; base < end; base += kWave) {
    const int n = min(kWave, end - base);
    const int my_col = lane < n ? col[base + lane] : 0;
    for (int j = 0; j < n; j += NS * U) {
      Raw<float, 4> raw[U][NCH];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int jj = j + u * NS + slot;
        const int src = __shfl(my_col, jj & (kWave - 1));
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
          const int c0 = (ch * LPR + li) * 4;
          if (jj < n && c0 < d) raw[u][ch] = load_raw<float, 4>(xe + static_cast<int64_t>(src) * ldxe + c0);
          else raw[u][ch] = zero_raw<float, 4>();
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
          const FVec<4> v = unpack<float, 4>(raw[u][ch]);
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[ch][k] += v.v[k];
        }
    }
  }
  // the slots' partial sums meet in every lane (xor butterfly): all NS lane groups then hold the whole row
#pragma unroll
  for (int off = LPR; off < kWave; off <<= 1)
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[ch][k] += __shfl_xor(acc[ch][k], off);

  finish_row<LPR, NCH>(tl, row, li, d, acc, xi, ldxi, slot == 0);
}

// short-row variant (flat_rows.h); single column chunk (d <= LPR * 4).  Every lane of the slot calls finish_row: the norm's
// butterfly stays inside the slot.
template <int LPR>
__global__ __launch_bounds__(kBlock) void unigcn_flat_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ xe, int64_t ldxe, Tail tl,
    float* __restrict__ xi, int64_t ldxi, int n_t, int d) {
  FlatSlot<LPR> s;
  if (s.wave_beyond(n_t)) return;
  s.open(rowptr, n_t);
  const int c0 = s.li * 4;
  const bool active = c0 < d;
  float acc[1][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) acc[0][k] = 0.f;
  int my_col = 0;
  Raw<float, 4> raw[kFlatUnroll];

  flat_walk<kFlatUnroll>(
      s, active, [&](int base, int n) { my_col = s.li < n ? col[base + s.li] : 0; },
      [&](int u, int jj, bool ok) {
        const int src = s.bcast(my_col, jj);
        if (ok) raw[u] = load_raw<float, 4>(xe + static_cast<int64_t>(src) * ldxe + c0);
        else raw[u] = zero_raw<float, 4>();
      },
      [&](int u) {
        const FVec<4> v = unpack<float, 4>(raw[u]);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[0][k] += v.v[k];
      },
      [&] {
        finish_row<LPR, 1>(tl, s.cur_row, s.li, d, acc, xi, ldxi, true);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[0][k] = 0.f;
      });
}

template <int LPR, int NCH>
static void launch_rows(hipStream_t st, const int32_t* rowptr, const int32_t* col, const float* xe, int64_t ldxe, const Tail& tl,
                        float* xi, int64_t ldxi, int n_t, int d, const int32_t* row_order) {
  const unsigned grid = static_cast<unsigned>((static_cast<int64_t>(n_t) + kWavesPerBlock - 1) / kWavesPerBlock);
  unigcn_hop_kernel<LPR, NCH><<<grid, kBlock, 0, st>>>(rowptr, col, xe, ldxe, tl, xi, ldxi, n_t, d, row_order);
}

}  // namespace unigcn
}  // namespace allset

using namespace allset;
using namespace allset::unigcn;

extern "C" int allset_unigcn_supported(void) { return 1; }

extern "C" int allset_unigcn_hop_fwd(int variant, int64_t nnz, const int32_t* row_order, const int32_t* rowptr, const int32_t* col,
                                     const float* degV, const float* xe, int64_t ldxe, const float* x0, int64_t ldx0, float alpha,
                                     int use_norm, float* xi, int64_t ldxi, float* t_out, int64_t n_t, int64_t n_s, int64_t d,
                                     void* stream) {
  clear_error();
  ALLSET_REQUIRE(variant >= 0 && variant <= 2, "unigcn_hop_fwd: bad variant %d", variant);
  ALLSET_REQUIRE(n_t >= 0 && n_s >= 0 && d >= 0 && nnz >= 0, "unigcn_hop_fwd: negative size");
  ALLSET_REQUIRE(n_t < INT32_MAX && n_s < INT32_MAX && nnz < INT32_MAX, "unigcn_hop_fwd: size exceeds int32");
  ALLSET_REQUIRE(alpha == alpha, "unigcn_hop_fwd: alpha is NaN");
  if (d > kMaxWidth || d % 4 != 0) {
    set_error("unigcn_hop_fwd: width %lld is not built (multiples of 4 up to the maximum %d)", static_cast<long long>(d), kMaxWidth);
    return ALLSET_ERR_UNSUPPORTED;
  }
  if (n_t == 0 || d == 0) return ALLSET_OK;
  ALLSET_REQUIRE(rowptr && xi && x0, "unigcn_hop_fwd: null rowptr/xi/x0");
  ALLSET_REQUIRE(!use_norm || t_out, "unigcn_hop_fwd: null t_out with use_norm");
  ALLSET_REQUIRE(ldxe >= d && ldx0 >= d && ldxi >= d, "unigcn_hop_fwd: leading dimension smaller than d");
  ALLSET_REQUIRE(nnz == 0 || (col && xe), "unigcn_hop_fwd: null col/xe with nnz > 0");
  if (!((ldxe % 4 == 0) && (ldx0 % 4 == 0) && (ldxi % 4 == 0) && aligned16(xe) && aligned16(x0) && aligned16(xi))) {
    set_error("unigcn_hop_fwd: rows must be 16-byte aligned (pointers and leading dimensions)");
    return ALLSET_ERR_UNSUPPORTED;
  }
  if (variant == 2 && d > 256) {
    set_error("unigcn_hop_fwd: the short-row variant needs d <= 256");
    return ALLSET_ERR_UNSUPPORTED;
  }
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const Tail tl{degV, x0, ldx0, t_out, alpha, use_norm ? 1 : 0};
  const int nt = static_cast<int>(n_t), di = static_cast<int>(d);
  const bool use_flat = d <= 256 && (variant == 2 || (variant == 0 && n_t > kFlatMinRows &&
                                                      static_cast<double>(nnz) < kFlatMaxMeanDegree * static_cast<double>(n_t)));
  if (use_flat) {
    with_lpr(pick_lpr(d), [&](auto lpr) {
      unigcn_flat_kernel<lpr()><<<flat_grid<lpr()>(n_t), kBlock, 0, st>>>(rowptr, col, xe, ldxe, tl, xi, ldxi, nt, di);
    });
  } else if (d > 256) {
    launch_rows<64, 2>(st, rowptr, col, xe, ldxe, tl, xi, ldxi, nt, di, row_order);
  } else {
    with_lpr(pick_lpr(d), [&](auto lpr) { launch_rows<lpr(), 1>(st, rowptr, col, xe, ldxe, tl, xi, ldxi, nt, di, row_order); });
  }
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}
