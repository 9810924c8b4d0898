// Degree-scaled propagate of the hypergraph-convolution baselines (reference layers.py:233-494: HNHNConv and HypergraphConv,
// HCHA / HGNN) for gfx950:
//   y[t,:] = drop_p( act( s[t] * sum_{j in row t} r[col_j] * x[col_j,:] + bias ) )
// r (one scale per GATHERED row), s (one per OUTPUT row) and bias may each be NULL; act is none / relu / elu.  Both hops of a
// conv (V->E over inc.by_dst, E->V over inc.by_src) are this one launch, and so is the backward of either hop: over the
// transposed CSR with r and s swapped and no epilogue, gx[v] = r[v] * sum_t s[t] * g[t].  The only other kernel is the
// epilogue's backward (allset_hconv_bwd_epi below): g = gy * keep / (1 - p) * act'(y), with act' recovered from y alone.
//
// Mapping: segreduce.hip's, with the per-source scale and the epilogue added:
//   * one wavefront per CSR row, LPR lanes x 16 B per feature row, NS = 64 / LPR source rows gathered per load;
//   * the up-to-64 column ids of the row arrive in ONE coalesced load (lane j holds id j, and r[id j] when r is given) and
//     are broadcast with ds_bpermute, kUnroll = 8 gathers in flight per slot;
//   * XCD-contiguous workgroup order, and the CSR's long-rows-first order (row_order) when the caller has one;
//   * a short-row variant (several consecutive rows per lane group, one stream of incidences: flat_rows.h) below a mean degree of 6.
// Algorithmic bytes per launch: nnz * (4d + 4) + (n_t + 1) * 4 + n_t * 4d, plus 4 * nnz for the r gathers.
//
// allset_hconv_fwd_w (CEGCN's GCNConv hop over the clique expansion) is the same launch with a per-INCIDENCE weight w[j] in place
// of the per-source r[col_j]: w is read in CSR order next to the column ids (one coalesced load per 64 incidences), so the
// backward over the transposed CSR takes w permuted into that CSR's order, once per graph.
#include "common.h"
#include "flat_rows.h"
#include "row_epilogue.h"

namespace allset {
namespace hconv {

enum { kScNone = 0, kScR = 1, kScW = 2 };   // per-incidence scale: none, r[col_j] (per gathered row), w[j] (per CSR position)
constexpr int kUnroll = 8;

struct Epi {
  const float* s;         // per output row, or NULL
  RowEpi row;
};

// epilogue of VEC consecutive columns c0.. of output row `row`
template <int VEC>
__device__ __forceinline__ void epilogue(const Epi& e, int row, int c0, int d, float (&acc)[VEC]) {
  const float sc = e.s ? e.s[row] : 1.f;
#pragma unroll
  for (int k = 0; k < VEC; ++k)
    acc[k] = row_epilogue<true>(e.row, acc[k] * sc, c0 + k, [=] { return static_cast<int64_t>(row) * d + c0 + k; });
}

template <int VEC>
__device__ __forceinline__ void store_row(float* __restrict__ y, int64_t ldy, int row, int c0, const float (&acc)[VEC]) {
  FVec<VEC> o;
#pragma unroll
  for (int k = 0; k < VEC; ++k) o.v[k] = acc[k];
  store_vec<float, VEC>(y + static_cast<int64_t>(row) * ldy + c0, o);
}

// SC: kScNone, kScR (r indexed by the gathered row id) or kScW (r is the weight stream, indexed by CSR position)
template <int VEC, int LPR, int SC>
__global__ __launch_bounds__(kBlock) void hconv_fwd_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ r,
    const float* __restrict__ x, int64_t ldx, float* __restrict__ y, int64_t ldy, int n_t, int d,
    const int32_t* __restrict__ row_order, Epi e, const uint64_t* __restrict__ seed_base) {
  constexpr int NS = kWave / LPR;
  const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int slot_row = static_cast<int>(blk) * kWavesPerBlock + (threadIdx.x >> 6);
  if (slot_row >= n_t) return;  // whole wave exits together
  const int row = row_order ? row_order[slot_row] : slot_row;
  e.row.seed = resolve_seed(seed_base, e.row.seed);
  const int lane = lane_id();
  const int slot = lane / LPR, li = lane % LPR;
  const int start = rowptr[row], end = rowptr[row + 1];

  for (int cb = 0; cb < d; cb += LPR * VEC) {
    const int c0 = cb + li * VEC;
    const bool active = c0 < d;
    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;

    for (int base = start; base < end; base += kWave) {
      const int n = min(kWave, end - base);
      int my_col = 0;
      float my_r = 0.f;
      if (lane < n) {
        my_col = col[base + lane];
        if constexpr (SC == kScR) my_r = r[my_col];
        if constexpr (SC == kScW) my_r = r[base + lane];
      }
      for (int j = 0; j < n; j += NS * kUnroll) {
        Raw<float, VEC> raw[kUnroll];
        float rr[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const int jj = j + u * NS + slot;
          const int src = __shfl(my_col, jj & (kWave - 1));
          if constexpr (SC != kScNone) rr[u] = __shfl(my_r, jj & (kWave - 1)); else rr[u] = 1.f;
          if (jj < n && active) raw[u] = load_raw<float, VEC>(x + static_cast<int64_t>(src) * ldx + c0);
          else raw[u] = zero_raw<float, VEC>();
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const FVec<VEC> v = unpack<float, VEC>(raw[u]);
          // (a skipped slot holds v == 0, but its rr is the broadcast of another incidence's scale, which may be inf (HNHN's
          //  deg^beta of an isolated vertex): skip it explicitly so that 0 * inf never reaches the sum)
          if constexpr (SC != kScNone) {
            if (j + u * NS + slot < n) {
#pragma unroll
              for (int k = 0; k < VEC; ++k) acc[k] = fmaf(rr[u], v.v[k], acc[k]);
            }
          } else {
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] += v.v[k];
          }
        }
      }
    }
#pragma unroll
    for (int off = LPR; off < kWave; off <<= 1)
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] += __shfl_xor(acc[k], off);

    if (slot == 0 && active) {
      epilogue<VEC>(e, row, c0, d, acc);
      store_row<VEC>(y, ldy, row, c0, acc);
    }
  }
}

// short-row variant (the scheme of flat_rows.h); single column chunk (d <= LPR * 4), 16-byte rows.  The walk is written out here,
// not taken from flat_walk(): over the header this kernel measured 0.5 % slower with a per-incidence scale (hipcc 7.2 orders the
// loop bodies differently; profiles/flat_walk_refactor.md), so it keeps its own text.
template <int LPR, int SC>
__global__ __launch_bounds__(kBlock) void hconv_flat_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ r,
    const float* __restrict__ x, int64_t ldx, float* __restrict__ y, int64_t ldy, int n_t, int d, Epi e,
    const uint64_t* __restrict__ seed_base) {
  constexpr int VEC = 4;
  constexpr int NS = kWave / LPR;
  const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int lane = lane_id();
  const int slot = lane / LPR, li = lane % LPR;
  const int lane0 = slot * LPR;
  const int64_t slot_global = (static_cast<int64_t>(blk) * kWavesPerBlock + (threadIdx.x >> 6)) * NS + slot;
  const int64_t r_begin64 = slot_global * kFlatRows;
  if (r_begin64 - static_cast<int64_t>(slot) * kFlatRows >= n_t) return;      // whole wave beyond the last row
  e.row.seed = resolve_seed(seed_base, e.row.seed);
  const int r_begin = static_cast<int>(min(r_begin64, static_cast<int64_t>(n_t)));
  const int r_end = min(r_begin + kFlatRows, n_t);
  const int c0 = li * VEC;
  const bool active = c0 < d;
  const int rp = (li <= r_end - r_begin) ? rowptr[r_begin + li] : 0;
  const int q0 = __shfl(rp, lane0);
  const int q_end = __shfl(rp, lane0 + (r_end - r_begin));

  int cur_row = r_begin;
  int cur_end = (r_begin < r_end) ? __shfl(rp, lane0 + 1) : q0;
  float acc[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc[k] = 0.f;

  auto flush = [&]() {
    if (active) {
      epilogue<VEC>(e, cur_row, c0, d, acc);
      store_row<VEC>(y, ldy, cur_row, c0, acc);
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
    ++cur_row;
    cur_end = __shfl(rp, lane0 + min(cur_row - r_begin + 1, LPR - 1));
  };

  for (int base = q0; base < q_end; base += LPR) {
    const int n = min(LPR, q_end - base);
    int my_col = 0;
    float my_r = 0.f;
    if (li < n) {
      my_col = col[base + li];
      if constexpr (SC == kScR) my_r = r[my_col];
      if constexpr (SC == kScW) my_r = r[base + li];
    }
    for (int j = 0; j < n; j += kUnroll) {
      Raw<float, VEC> raw[kUnroll];
      float rr[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int jj = j + u;
        const int src = __shfl(my_col, lane0 + (jj & (LPR - 1)));
        if constexpr (SC != kScNone) rr[u] = __shfl(my_r, lane0 + (jj & (LPR - 1))); else rr[u] = 1.f;
        if (jj < n && active) raw[u] = load_raw<float, VEC>(x + static_cast<int64_t>(src) * ldx + c0);
        else raw[u] = zero_raw<float, VEC>();
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int pos = base + j + u;
        if (j + u < n) {
          while (pos >= cur_end) flush();                          // also steps over empty rows
          const FVec<VEC> v = unpack<float, VEC>(raw[u]);
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc[k] = fmaf(rr[u], v.v[k], acc[k]);
        }
      }
    }
  }
  while (cur_row < r_end) flush();                                 // last row and trailing empty rows
}

// g = gy * keep / (1 - p) * act'(y), and per-slab column sums of g (the bias gradient's partials).  act' from the saved
// output alone: relu -> y > 0; elu -> with a = y * (1 - p) the pre-dropout activation of a KEPT element, 1 if a > 0 else
// a + 1 (elu'(z) = exp(z) = elu(z) + 1 for z <= 0).  Grid: x = 64-column chunks, y = row slabs; 4 waves per workgroup
// walk the slab's rows with stride 4, lane = column; the 4 waves' column sums meet in LDS.
__global__ __launch_bounds__(kBlock) void hconv_bwd_epi_kernel(
    const float* __restrict__ gy, int64_t ldg, const float* __restrict__ y, int64_t ldy, int act, float p, uint64_t seed,
    const uint64_t* __restrict__ seed_base, float* __restrict__ g, int64_t ldo, float* __restrict__ part, int64_t M,
    int64_t n, int d, int64_t rows_per_slab) {
  __shared__ float red[kWavesPerBlock][kWave];
  seed = resolve_seed(seed_base, seed);
  const uint32_t thr = drop_threshold(p);
  const float keep = 1.f - p;
  const float inv_keep = p > 0.f ? 1.f / keep : 1.f;
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  const int c = static_cast<int>(blockIdx.x) * kWave + lane;
  const int64_t r0 = static_cast<int64_t>(blockIdx.y) * rows_per_slab;
  const int64_t r1 = min(n, r0 + rows_per_slab);
  float sum = 0.f;
  if (c < d) {
    for (int64_t row = r0 + wv; row < r1; row += kWavesPerBlock) {
      const float gv = gy[row * ldg + c];
      const float yv = y[row * ldy + c];
      float k = 1.f;
      if (p > 0.f) k = keep_scale(seed, row * d + c, thr, inv_keep);
      const float out = row_epilogue_bwd(gv, yv, k, act, keep);
      g[row * ldo + c] = out;
      sum += out;
    }
  }
  if (part == nullptr) return;
  red[wv][lane] = sum;
  __syncthreads();
  if (wv == 0 && c < M) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) t += red[w][lane];
    part[static_cast<int64_t>(blockIdx.y) * M + c] = c < d ? t : 0.f;
  }
}

constexpr int64_t kEpiMaxSlabs = 256;

template <int VEC, int LPR>
static void launch_fwd(int sc, unsigned grid, hipStream_t st, const int32_t* rowptr, const int32_t* col, const float* r,
                       const float* x, int64_t ldx, float* y, int64_t ldy, int n_t, int d, const int32_t* row_order, const Epi& e,
                       const uint64_t* seed_base) {
  if (sc == kScR)      hconv_fwd_kernel<VEC, LPR, kScR><<<grid, kBlock, 0, st>>>(rowptr, col, r, x, ldx, y, ldy, n_t, d, row_order, e, seed_base);
  else if (sc == kScW) hconv_fwd_kernel<VEC, LPR, kScW><<<grid, kBlock, 0, st>>>(rowptr, col, r, x, ldx, y, ldy, n_t, d, row_order, e, seed_base);
  else                 hconv_fwd_kernel<VEC, LPR, kScNone><<<grid, kBlock, 0, st>>>(rowptr, col, r, x, ldx, y, ldy, n_t, d, row_order, e, seed_base);
}

template <int LPR>
static void launch_flat(int sc, hipStream_t st, const int32_t* rowptr, const int32_t* col, const float* r, const float* x,
                        int64_t ldx, float* y, int64_t ldy, int n_t, int d, const Epi& e, const uint64_t* seed_base) {
  const unsigned grid = flat_grid<LPR>(n_t);
  if (sc == kScR)      hconv_flat_kernel<LPR, kScR><<<grid, kBlock, 0, st>>>(rowptr, col, r, x, ldx, y, ldy, n_t, d, e, seed_base);
  else if (sc == kScW) hconv_flat_kernel<LPR, kScW><<<grid, kBlock, 0, st>>>(rowptr, col, r, x, ldx, y, ldy, n_t, d, e, seed_base);
  else                 hconv_flat_kernel<LPR, kScNone><<<grid, kBlock, 0, st>>>(rowptr, col, r, x, ldx, y, ldy, n_t, d, e, seed_base);
}

}  // namespace hconv
}  // namespace allset

using namespace allset;
using namespace allset::hconv;

extern "C" int allset_hconv_supported(void) { return 1; }

// r: per gathered row (sc = kScR) or per CSR position (sc = kScW); NULL = ones
static int hconv_fwd_impl(int sc, int variant, int64_t nnz, const int32_t* row_order, const int32_t* rowptr, const int32_t* col,
                          const float* r, const float* s, const float* x, int64_t ldx, const float* bias, int act, float p,
                          uint64_t seed, const uint64_t* seed_base, float* y, int64_t ldy, int64_t n_t, int64_t n_s,
                          int64_t d, void* stream) {
  ALLSET_REQUIRE(variant >= 0 && variant <= 2, "hconv_fwd: bad variant %d", variant);
  ALLSET_REQUIRE(act >= kActNone && act <= kActElu, "hconv_fwd: bad act %d", act);
  ALLSET_REQUIRE(p >= 0.f && p < 1.f, "hconv_fwd: dropout p must be in [0,1)");
  ALLSET_REQUIRE(n_t >= 0 && n_s >= 0 && d >= 0, "hconv_fwd: negative size");
  ALLSET_REQUIRE(n_t < INT32_MAX && n_s < INT32_MAX && d < INT32_MAX && n_t * d < INT64_MAX / 2, "hconv_fwd: size exceeds int32");
  if (n_t == 0 || d == 0) return ALLSET_OK;
  ALLSET_REQUIRE(rowptr && y, "hconv_fwd: null rowptr/y");
  ALLSET_REQUIRE(ldx >= d && ldy >= d, "hconv_fwd: leading dimension smaller than d");
  ALLSET_REQUIRE(nnz == 0 || (col && x), "hconv_fwd: null col/x with nnz > 0");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const bool vec4 = (d % 4 == 0) && (ldx % 4 == 0) && (ldy % 4 == 0) && aligned16(x) && aligned16(y);
  const Epi ep{s, row_epi(bias, act, p, seed)};
  const int nt = static_cast<int>(n_t), di = static_cast<int>(d);
  const bool flat_ok = vec4 && d <= 256;
  const bool use_flat = flat_ok && (variant == 2 || (variant == 0 && nnz >= 0 && n_t > kFlatMinRows &&
                                                     static_cast<double>(nnz) < kFlatMaxMeanDegree * static_cast<double>(n_t)));
  if (variant == 2 && !flat_ok) {
    set_error("hconv_fwd: the short-row variant needs 16-byte aligned rows and d <= 256");
    return ALLSET_ERR_UNSUPPORTED;
  }
  const int has_r = r != nullptr ? sc : kScNone;
  if (use_flat) {
    with_lpr(pick_lpr(d), [&](auto lpr) { launch_flat<lpr()>(has_r, st, rowptr, col, r, x, ldx, y, ldy, nt, di, ep, seed_base); });
  } else {
    with_vec_lpr<4>(vec4, d, [&](auto vec, auto lpr) {
      launch_fwd<vec(), lpr()>(has_r, row_grid(n_t), st, rowptr, col, r, x, ldx, y, ldy, nt, di, row_order, ep, seed_base);
    });
  }
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_hconv_fwd(int variant, int64_t nnz, const int32_t* row_order, const int32_t* rowptr, const int32_t* col,
                                const float* r, const float* s, const float* x, int64_t ldx, const float* bias, int act, float p,
                                uint64_t seed, const uint64_t* seed_base, float* y, int64_t ldy, int64_t n_t, int64_t n_s,
                                int64_t d, void* stream) {
  clear_error();
  return hconv_fwd_impl(kScR, variant, nnz, row_order, rowptr, col, r, s, x, ldx, bias, act, p, seed, seed_base, y, ldy, n_t, n_s, d,
                        stream);
}

extern "C" int allset_hconv_fwd_w(int variant, int64_t nnz, const int32_t* row_order, const int32_t* rowptr, const int32_t* col,
                                  const float* w, const float* s, const float* x, int64_t ldx, const float* bias, int act, float p,
                                  uint64_t seed, const uint64_t* seed_base, float* y, int64_t ldy, int64_t n_t, int64_t n_s,
                                  int64_t d, void* stream) {
  clear_error();
  return hconv_fwd_impl(kScW, variant, nnz, row_order, rowptr, col, w, s, x, ldx, bias, act, p, seed, seed_base, y, ldy, n_t, n_s, d,
                        stream);
}

extern "C" int allset_hconv_bwd_epi_slices(int64_t n, int64_t* n_slices) {
  clear_error();
  ALLSET_REQUIRE(n >= 0 && n_slices, "hconv_bwd_epi_slices: bad arguments");
  const int64_t want = (n + 255) / 256;                            // at least 256 rows per slab
  *n_slices = want < 1 ? 1 : (want > kEpiMaxSlabs ? kEpiMaxSlabs : want);
  return ALLSET_OK;
}

extern "C" int allset_hconv_bwd_epi(const float* gy, int64_t ldg, const float* y, int64_t ldy, int act, float p, uint64_t seed,
                                    const uint64_t* seed_base, float* g, int64_t ldo, float* part, int64_t n_slices, int64_t M,
                                    int64_t n, int64_t d, void* stream) {
  clear_error();
  ALLSET_REQUIRE(act >= kActNone && act <= kActElu, "hconv_bwd_epi: bad act %d", act);
  ALLSET_REQUIRE(p >= 0.f && p < 1.f, "hconv_bwd_epi: dropout p must be in [0,1)");
  ALLSET_REQUIRE(n >= 0 && d >= 0 && d < INT32_MAX, "hconv_bwd_epi: bad size");
  ALLSET_REQUIRE(part == nullptr || (n_slices >= 1 && n_slices <= kEpiMaxSlabs && M >= d && M <= (d + kWave - 1) / kWave * kWave),
                 "hconv_bwd_epi: bad partial layout (n_slices %lld, M %lld)", static_cast<long long>(n_slices), static_cast<long long>(M));
  if (d == 0 || (n == 0 && part == nullptr)) return ALLSET_OK;
  ALLSET_REQUIRE(n == 0 || (g && gy && y), "hconv_bwd_epi: null pointer");
  ALLSET_REQUIRE(ldg >= d && ldy >= d && ldo >= d, "hconv_bwd_epi: leading dimension smaller than d");
  const int64_t slabs = part ? n_slices : ((n + 255) / 256 < kEpiMaxSlabs ? (n + 255) / 256 : kEpiMaxSlabs);
  const int64_t rows_per_slab = (n + slabs - 1) / slabs;
  const dim3 grid(static_cast<unsigned>((d + kWave - 1) / kWave), static_cast<unsigned>(slabs < 1 ? 1 : slabs));
  hconv_bwd_epi_kernel<<<grid, kBlock, 0, static_cast<hipStream_t>(stream)>>>(gy, ldg, y, ldy, act, p, seed, seed_base, g, ldo, part,
                                                                               M, n, static_cast<int>(d), rows_per_slab < 1 ? 1 : rows_per_slab);
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}
