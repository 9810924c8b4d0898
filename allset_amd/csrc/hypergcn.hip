// HyperGCN (reference utils.py:11-199, models.py:29-77) for gfx950: the per-hyperedge Laplacian approximation built on the device and
// one hop  out = drop_p(act(A x + bias)),  A = D^-1/2 (W + I) D^-1/2,  without ever forming the N x N matrix.
//
// Structure (three launches, no feature-width traffic beyond the one projection):
//   project : p[v] = Z[v, :] . rv                                      (every row summed in the same order: equal rows -> equal bits)
//   select  : per hyperedge e (row of the hyperedge-major CSR) S[e] / I[e] = the member at the FIRST arg-max / arg-min of p in the
//             caller's edge-list order (the CSR's perm is carried along as the tie-break), w[e] = 1 / (2k - 3) with mediators, 1 / k
//             without, and the size k
//   degree  : per vertex v (row of the vertex-major CSR) D[v] = 1 + rowsum(W)[v] from the roles alone, dinv[v] = D^-1/2,
//             selfc[v] = 1 - sum of w[e] over the hyperedges in which v is ONE of two distinct extremes, and per incidence the row
//             of the per-hyperedge buffer PQ that the E->V pass gathers for it (colx, below)
// Hop (two launches).  With y = dinv * x, T_e = sum_{u in e} y[u] and f = (S == I ? 2 : 1):
//   v2e     : mediators:    PQ[2e] = P_e = f w * (sum of y[u] over the members u that are S or I)   (= w (y[S] + y[I]) either way),
//                           PQ[2e + 1] = Q_e = f w T_e                  -- one gather of the members, two accumulators
//             no mediators: PQ[e] = w (y[S] + y[I])                     -- two rows per hyperedge, no CSR walk
//   e2v     : out[v] = epilogue( dinv[v] * ( selfc[v] * y[v] + sum_{j in row v, colx_j >= 0} PQ[colx_j] ) )
//             colx = 2e + 1 for an extreme of e, 2e for a mediator (mediators); e for an extreme, -1 otherwise (no mediators).
//             An extreme of a hyperedge with S != I is owed Q_e - w y[v] (resp. P_e - w y[v]): the subtraction is the selfc term.
//             epilogue: + bias, relu, hash dropout with hconv.hip's element index (row * d + column), so allset_hconv_bwd_epi is
//             its backward; A is symmetric, so the backward in x is the same two launches on the masked gradient.
//
// Mapping of the two hop kernels: hconv.hip's (one wavefront per CSR row, LPR lanes x 16 B per feature row, NS = 64 / LPR rows per
// load, the row's column ids in one coalesced load broadcast with ds_bpermute, 8 gathers in flight per slot, XCD-contiguous
// workgroup order, row_order for skewed CSRs, and for e2v the short-row variant of several rows per lane group).
// Built for fp32 and widths d % 4 == 0 up to 256 with 16-byte aligned rows, plus any d <= 64 one column per lane (the class counts
// of the last layer); anything else: ALLSET_ERR_UNSUPPORTED and the caller composes the hop from allset_hconv_fwd.
// Algorithmic bytes: v2e nnz * (4d + 8) + (n_e + 1) * 4 + 12 n_e + 2 n_e * 4d;  e2v nnz * (4d + 4) + (n_v + 1) * 4 + 8 n_v + 2 n_v * 4d.
#include "common.h"
#include "flat_rows.h"
#include "row_epilogue.h"

namespace allset {
namespace hypergcn {

constexpr int kUnroll = 8;
constexpr int kMaxWidth = 256;
constexpr int kMaxScalarWidth = 64;

// ---- structure ------------------------------------------------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(kBlock) void project_kernel(const float* __restrict__ z, int64_t ldz, const float* __restrict__ rv,
                                                         float* __restrict__ p, int n, int d, int g) {
  const int lane = lane_id();
  const int rows_per_wave = kWave / g;
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t row = wave * rows_per_wave + lane / g;
  const int li = lane % g;
  float acc = 0.f;
  if (row < n) {
    const float* zr = z + row * ldz;
    for (int c = li * VEC; c < d; c += g * VEC) {
      const FVec<VEC> a = load_vec<float, VEC>(zr + c);
      const FVec<VEC> b = load_vec<float, VEC>(rv + c);
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc = fmaf(a.v[k], b.v[k], acc);
    }
  }
  for (int off = 1; off < g; off <<= 1) acc += __shfl_xor(acc, off);
  if (row < n && li == 0) p[row] = acc;
}

struct Pick {
  float val;
  int pos;     // position in the caller's edge list (the tie-break); INT32_MAX = nothing yet
  int idx;     // the member
};
// does b beat a?  SIGN = +1: larger value wins; -1: smaller.  Equal values: the earlier position.  A NaN never wins.
template <int SIGN>
__device__ __forceinline__ bool beats(const Pick& b, const Pick& a) {
  if (b.pos == INT32_MAX) return false;
  if (a.pos == INT32_MAX) return b.val == b.val;
  const bool better = SIGN > 0 ? b.val > a.val : b.val < a.val;
  return better || (b.val == a.val && b.pos < a.pos);
}

template <int G>
__global__ __launch_bounds__(kBlock) void select_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                        const int32_t* __restrict__ perm, const float* __restrict__ p, int mediators,
                                                        int32_t* __restrict__ S, int32_t* __restrict__ I, float* __restrict__ w,
                                                        int32_t* __restrict__ size, int n_e) {
  constexpr int NS = kWave / G;
  const int lane = lane_id();
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t row64 = wave * NS + lane / G;
  const int li = lane % G;
  const bool live = row64 < n_e;
  const int row = live ? static_cast<int>(row64) : 0;
  const int start = live ? rowptr[row] : 0, end = live ? rowptr[row + 1] : 0;
  Pick hi{0.f, INT32_MAX, -1}, lo{0.f, INT32_MAX, -1};
  for (int j = start + li; j < end; j += G) {
    const int v = col[j];
    const Pick c{p[v], perm[j], v};
    if (beats<1>(c, hi)) hi = c;
    if (beats<-1>(c, lo)) lo = c;
  }
#pragma unroll
  for (int off = 1; off < G; off <<= 1) {
    const Pick oh{__shfl_xor(hi.val, off), __shfl_xor(hi.pos, off), __shfl_xor(hi.idx, off)};
    const Pick ol{__shfl_xor(lo.val, off), __shfl_xor(lo.pos, off), __shfl_xor(lo.idx, off)};
    if (beats<1>(oh, hi)) hi = oh;
    if (beats<-1>(ol, lo)) lo = ol;
  }
  if (live && li == 0) {
    const int k = end - start;
    S[row] = hi.idx;
    I[row] = lo.idx;
    size[row] = k;
    w[row] = k == 0 ? 0.f : 1.f / static_cast<float>(mediators ? 2 * k - 3 : k);
  }
}

template <int G>
__global__ __launch_bounds__(kBlock) void degree_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                        const int32_t* __restrict__ S, const int32_t* __restrict__ I,
                                                        const float* __restrict__ w, const int32_t* __restrict__ size, int mediators,
                                                        float* __restrict__ dinv, float* __restrict__ selfc,
                                                        int32_t* __restrict__ colx, int n_v) {
  constexpr int NS = kWave / G;
  const int lane = lane_id();
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t row64 = wave * NS + lane / G;
  const int li = lane % G;
  const bool live = row64 < n_v;
  const int v = live ? static_cast<int>(row64) : 0;
  const int start = live ? rowptr[v] : 0, end = live ? rowptr[v + 1] : 0;
  float deg = 0.f, sub = 0.f;
  for (int j = start + li; j < end; j += G) {
    const int e = col[j];
    const int s = S[e], i = I[e];
    const float we = w[e];
    const bool ext = s == v || i == v;
    int cx;
    if (mediators) {
      const float k = static_cast<float>(size[e]);
      if (s != i) {
        deg += ext ? we * (k - 1.f) : 2.f * we;
        if (ext) sub += we;
      } else {
        deg += ext ? 2.f * we * k : 2.f * we;
      }
      cx = 2 * e + (ext ? 1 : 0);
    } else {
      if (ext) {
        deg += s != i ? we : 2.f * we;
        if (s != i) sub += we;
      }
      cx = ext ? e : -1;
    }
    colx[j] = cx;
  }
#pragma unroll
  for (int off = 1; off < G; off <<= 1) {
    deg += __shfl_xor(deg, off);
    sub += __shfl_xor(sub, off);
  }
  if (live && li == 0) {
    const float D = 1.f + deg;
    dinv[v] = D == 0.f ? 0.f : 1.f / sqrtf(D);     // (the reference: inf -> 0; a negative degree is its NaN)
    selfc[v] = 1.f - sub;
  }
}

// ---- V -> E ---------------------------------------------------------------------------------------------------------------------
template <int VEC, int LPR>
__global__ __launch_bounds__(kBlock) void v2e_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                     const int32_t* __restrict__ S, const int32_t* __restrict__ I,
                                                     const float* __restrict__ w, const float* __restrict__ dinv,
                                                     const float* __restrict__ x, int64_t ldx, float* __restrict__ pq, int64_t ldpq,
                                                     int n_e, int d, const int32_t* __restrict__ row_order) {
  constexpr int NS = kWave / LPR;
  const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int slot_row = static_cast<int>(blk) * kWavesPerBlock + (threadIdx.x >> 6);
  if (slot_row >= n_e) return;  // whole wave exits together
  const int row = row_order ? row_order[slot_row] : slot_row;
  const int lane = lane_id();
  const int slot = lane / LPR, li = lane % LPR;
  const int start = rowptr[row], end = rowptr[row + 1];
  const int s = S[row], i = I[row];
  const float wf = w[row] * (s == i ? 2.f : 1.f);
  const int c0 = li * VEC;
  const bool active = c0 < d;
  float accT[VEC], accP[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) accT[k] = accP[k] = 0.f;

  for (int base = start; base < end; base += kWave) {
    const int n = min(kWave, end - base);
    int my_col = 0, my_ext = 0;
    float my_r = 0.f;
    if (lane < n) {
      my_col = col[base + lane];
      my_r = dinv[my_col];
      my_ext = (my_col == s || my_col == i) ? 1 : 0;
    }
    for (int j = 0; j < n; j += NS * kUnroll) {
      Raw<float, VEC> raw[kUnroll];
      float rr[kUnroll];
      int ex[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int jj = j + u * NS + slot;
        const int src = __shfl(my_col, jj & (kWave - 1));
        rr[u] = __shfl(my_r, jj & (kWave - 1));
        ex[u] = __shfl(my_ext, jj & (kWave - 1));
        if (jj < n && active) raw[u] = load_raw<float, VEC>(x + static_cast<int64_t>(src) * ldx + c0);
        else raw[u] = zero_raw<float, VEC>();
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        if (j + u * NS + slot < n) {
          const FVec<VEC> v = unpack<float, VEC>(raw[u]);
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            const float t = rr[u] * v.v[k];
            accT[k] += t;
            if (ex[u]) accP[k] += t;
          }
        }
      }
    }
  }
#pragma unroll
  for (int off = LPR; off < kWave; off <<= 1)
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      accT[k] += __shfl_xor(accT[k], off);
      accP[k] += __shfl_xor(accP[k], off);
    }
  if (slot == 0 && active) {
    FVec<VEC> op, oq;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      op.v[k] = wf * accP[k];
      oq.v[k] = wf * accT[k];
    }
    store_vec<float, VEC>(pq + static_cast<int64_t>(2 * row) * ldpq + c0, op);
    store_vec<float, VEC>(pq + static_cast<int64_t>(2 * row + 1) * ldpq + c0, oq);
  }
}

// without mediators: PQ[e] = w (y[S] + y[I]), one thread per VEC columns of a hyperedge
template <int VEC>
__global__ __launch_bounds__(kBlock) void v2e_pair_kernel(const int32_t* __restrict__ S, const int32_t* __restrict__ I,
                                                          const float* __restrict__ w, const float* __restrict__ dinv,
                                                          const float* __restrict__ x, int64_t ldx, float* __restrict__ pq,
                                                          int64_t ldpq, int n_e, int d, int chunks) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int64_t e = t / chunks;
  const int c0 = static_cast<int>(t % chunks) * VEC;
  if (e >= n_e || c0 >= d) return;
  const int s = S[e], i = I[e];
  FVec<VEC> o;
  if (s < 0 || i < 0) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) o.v[k] = 0.f;
  } else {
    const float we = w[e], ds = dinv[s], di = dinv[i];
    const FVec<VEC> a = load_vec<float, VEC>(x + static_cast<int64_t>(s) * ldx + c0);
    const FVec<VEC> b = load_vec<float, VEC>(x + static_cast<int64_t>(i) * ldx + c0);
#pragma unroll
    for (int k = 0; k < VEC; ++k) o.v[k] = we * (ds * a.v[k] + di * b.v[k]);
  }
  store_vec<float, VEC>(pq + e * ldpq + c0, o);
}

// ---- E -> V ---------------------------------------------------------------------------------------------------------------------
struct Tail {
  const float* dinv;      // per output row
  const float* selfc;     // per output row
  const float* x;         // the hop's input (the self term)
  int64_t ldx;
  RowEpi epi;
};

template <int VEC>
__device__ __forceinline__ void finish_row(const Tail& tl, int row, int c0, int d, float (&acc)[VEC], float* __restrict__ y,
                                           int64_t ldy) {
  const float dv = tl.dinv[row];
  const float sc = tl.selfc[row] * dv;
  const FVec<VEC> xs = load_vec<float, VEC>(tl.x + static_cast<int64_t>(row) * tl.ldx + c0);
  FVec<VEC> o;
#pragma unroll
  for (int k = 0; k < VEC; ++k)
    o.v[k] = row_epilogue<false>(tl.epi, dv * fmaf(sc, xs.v[k], acc[k]), c0 + k, [=] { return static_cast<int64_t>(row) * d + c0 + k; });
  store_vec<float, VEC>(y + static_cast<int64_t>(row) * ldy + c0, o);
}

template <int VEC, int LPR>
__global__ __launch_bounds__(kBlock) void e2v_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colx,
                                                     const float* __restrict__ pq, int64_t ldpq, int n_pq, Tail tl,
                                                     const uint64_t* __restrict__ seed_base, float* __restrict__ y, int64_t ldy,
                                                     int n_v, int d, const int32_t* __restrict__ row_order) {
  constexpr int NS = kWave / LPR;
  const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int slot_row = static_cast<int>(blk) * kWavesPerBlock + (threadIdx.x >> 6);
  if (slot_row >= n_v) return;  // whole wave exits together
  const int row = row_order ? row_order[slot_row] : slot_row;
  tl.epi.seed = resolve_seed(seed_base, tl.epi.seed);
  const int lane = lane_id();
  const int slot = lane / LPR, li = lane % LPR;
  const int start = rowptr[row], end = rowptr[row + 1];
  const int c0 = li * VEC;
  const bool active = c0 < d;
  float acc[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc[k] = 0.f;

  for (int base = start; base < end; base += kWave) {
    const int n = min(kWave, end - base);
    int my_col = -1;
    if (lane < n) {
      my_col = colx[base + lane];
      if (my_col >= n_pq) my_col = -1;                                  // (never, for a structure the degree kernel wrote)
    }
    for (int j = 0; j < n; j += NS * kUnroll) {
      Raw<float, VEC> raw[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int jj = j + u * NS + slot;
        const int src = __shfl(my_col, jj & (kWave - 1));
        if (jj < n && active && src >= 0) raw[u] = load_raw<float, VEC>(pq + static_cast<int64_t>(src) * ldpq + c0);
        else raw[u] = zero_raw<float, VEC>();
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const FVec<VEC> v = unpack<float, VEC>(raw[u]);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] += v.v[k];
      }
    }
  }
#pragma unroll
  for (int off = LPR; off < kWave; off <<= 1)
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] += __shfl_xor(acc[k], off);

  if (slot == 0 && active) finish_row<VEC>(tl, row, c0, d, acc, y, ldy);
}

// short-row variant (flat_rows.h); 16-byte rows, d <= LPR * 4
template <int LPR>
__global__ __launch_bounds__(kBlock) void e2v_flat_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colx,
                                                          const float* __restrict__ pq, int64_t ldpq, int n_pq, Tail tl,
                                                          const uint64_t* __restrict__ seed_base, float* __restrict__ y, int64_t ldy,
                                                          int n_v, int d) {
  constexpr int VEC = 4;
  FlatSlot<LPR> s;
  if (s.wave_beyond(n_v)) return;
  tl.epi.seed = resolve_seed(seed_base, tl.epi.seed);
  s.open(rowptr, n_v);
  const int c0 = s.li * VEC;
  const bool active = c0 < d;
  float acc[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
  int my_col = -1;
  Raw<float, VEC> raw[kUnroll];

  flat_walk<kUnroll>(
      s, active,
      [&](int base, int n) {
        my_col = -1;
        if (s.li < n) {
          my_col = colx[base + s.li];
          if (my_col >= n_pq) my_col = -1;
        }
      },
      [&](int u, int jj, bool ok) {
        const int src = s.bcast(my_col, jj);
        if (ok && src >= 0) raw[u] = load_raw<float, VEC>(pq + static_cast<int64_t>(src) * ldpq + c0);
        else raw[u] = zero_raw<float, VEC>();
      },
      [&](int u) {
        const FVec<VEC> v = unpack<float, VEC>(raw[u]);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] += v.v[k];
      },
      [&] {
        if (active) finish_row<VEC>(tl, s.cur_row, c0, d, acc, y, ldy);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
      });
}

static inline int pick_group(int64_t nnz, int64_t rows) {   // lanes per CSR row of the structure kernels
  const double mean = rows > 0 ? static_cast<double>(nnz) / static_cast<double>(rows) : 0.0;
  return mean <= 8.0 ? 8 : (mean <= 32.0 ? 16 : 64);
}

template <int G>
static inline unsigned group_grid(int64_t rows) {
  const int64_t waves = (rows + (kWave / G) - 1) / (kWave / G);
  return static_cast<unsigned>((waves + kWavesPerBlock - 1) / kWavesPerBlock);
}

// 1: 16-byte lanes; 0: one column per lane; -1: not built
static inline int width_class(int64_t d, bool rows16) {
  if (d % 4 == 0 && d <= kMaxWidth && rows16) return 1;
  if (d <= kMaxScalarWidth) return 0;
  return -1;
}

}  // namespace hypergcn
}  // namespace allset

using namespace allset;
using namespace allset::hypergcn;

extern "C" int allset_hypergcn_supported(void) { return 1; }

extern "C" int allset_hypergcn_project(const float* z, int64_t ldz, const float* rv, float* p, int64_t n, int64_t d, void* stream) {
  clear_error();
  ALLSET_REQUIRE(n >= 0 && d >= 0 && n < INT32_MAX && d < INT32_MAX, "hypergcn_project: bad size");
  if (n == 0) return ALLSET_OK;
  ALLSET_REQUIRE(p, "hypergcn_project: null p");
  ALLSET_REQUIRE(d == 0 || (z && rv), "hypergcn_project: null z/rv");
  ALLSET_REQUIRE(ldz >= d, "hypergcn_project: leading dimension smaller than d");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const bool vec4 = (d % 4 == 0) && (ldz % 4 == 0) && aligned16(z) && aligned16(rv);
  const int vec = vec4 ? 4 : 1;
  int g = 1;                                     // lanes per row: enough for one pass over the row, at most the wave
  while (g < kWave && static_cast<int64_t>(g) * vec < d) g <<= 1;
  const int64_t waves = (n + (kWave / g) - 1) / (kWave / g);
  const unsigned grid = static_cast<unsigned>((waves + kWavesPerBlock - 1) / kWavesPerBlock);
  if (vec4) project_kernel<4><<<grid, kBlock, 0, st>>>(z, ldz, rv, p, static_cast<int>(n), static_cast<int>(d), g);
  else      project_kernel<1><<<grid, kBlock, 0, st>>>(z, ldz, rv, p, static_cast<int>(n), static_cast<int>(d), g);
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_hypergcn_select(const int32_t* rowptr, const int32_t* col, const int32_t* perm, const float* p, int mediators,
                                      int32_t* S, int32_t* I, float* w, int32_t* size, int64_t n_e, int64_t n_v, int64_t nnz,
                                      void* stream) {
  clear_error();
  ALLSET_REQUIRE(n_e >= 0 && n_v >= 0 && nnz >= 0 && n_e < INT32_MAX && n_v < INT32_MAX && nnz < INT32_MAX, "hypergcn_select: bad size");
  if (n_e == 0) return ALLSET_OK;
  ALLSET_REQUIRE(rowptr && S && I && w && size, "hypergcn_select: null rowptr/S/I/w/size");
  ALLSET_REQUIRE(nnz == 0 || (col && perm && p), "hypergcn_select: null col/perm/p with nnz > 0");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int ne = static_cast<int>(n_e), m = mediators ? 1 : 0;
  switch (pick_group(nnz, n_e)) {
    case 8:  select_kernel<8><<<group_grid<8>(n_e), kBlock, 0, st>>>(rowptr, col, perm, p, m, S, I, w, size, ne); break;
    case 16: select_kernel<16><<<group_grid<16>(n_e), kBlock, 0, st>>>(rowptr, col, perm, p, m, S, I, w, size, ne); break;
    default: select_kernel<64><<<group_grid<64>(n_e), kBlock, 0, st>>>(rowptr, col, perm, p, m, S, I, w, size, ne); break;
  }
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_hypergcn_degree(const int32_t* rowptr, const int32_t* col, const int32_t* S, const int32_t* I, const float* w,
                                      const int32_t* size, int mediators, float* dinv, float* selfc, int32_t* colx, int64_t n_v,
                                      int64_t n_e, int64_t nnz, void* stream) {
  clear_error();
  ALLSET_REQUIRE(n_e >= 0 && n_v >= 0 && nnz >= 0 && n_v < INT32_MAX && nnz < INT32_MAX, "hypergcn_degree: bad size");
  ALLSET_REQUIRE(n_e < INT32_MAX / 2, "hypergcn_degree: 2 * n_e exceeds int32");
  if (n_v == 0) return ALLSET_OK;
  ALLSET_REQUIRE(rowptr && dinv && selfc, "hypergcn_degree: null rowptr/dinv/selfc");
  ALLSET_REQUIRE(nnz == 0 || (col && S && I && w && size && colx), "hypergcn_degree: null col/S/I/w/size/colx with nnz > 0");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int nv = static_cast<int>(n_v), m = mediators ? 1 : 0;
  switch (pick_group(nnz, n_v)) {
    case 8:  degree_kernel<8><<<group_grid<8>(n_v), kBlock, 0, st>>>(rowptr, col, S, I, w, size, m, dinv, selfc, colx, nv); break;
    case 16: degree_kernel<16><<<group_grid<16>(n_v), kBlock, 0, st>>>(rowptr, col, S, I, w, size, m, dinv, selfc, colx, nv); break;
    default: degree_kernel<64><<<group_grid<64>(n_v), kBlock, 0, st>>>(rowptr, col, S, I, w, size, m, dinv, selfc, colx, nv); break;
  }
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_hypergcn_v2e(int mediators, int64_t nnz, const int32_t* row_order, const int32_t* rowptr, const int32_t* col,
                                   const int32_t* S, const int32_t* I, const float* w, const float* dinv, const float* x, int64_t ldx,
                                   float* pq, int64_t ldpq, int64_t n_e, int64_t n_v, int64_t d, void* stream) {
  clear_error();
  ALLSET_REQUIRE(n_e >= 0 && n_v >= 0 && d >= 0 && nnz >= 0, "hypergcn_v2e: negative size");
  ALLSET_REQUIRE(n_e < INT32_MAX / 2 && n_v < INT32_MAX && nnz < INT32_MAX, "hypergcn_v2e: size exceeds int32");
  const bool rows16 = (ldx % 4 == 0) && (ldpq % 4 == 0) && aligned16(x) && aligned16(pq);
  const int wc = width_class(d, rows16);
  if (wc < 0) {
    set_error("hypergcn_v2e: width %lld is not built (multiples of 4 up to %d with 16-byte aligned rows, or any width up to %d)",
              static_cast<long long>(d), kMaxWidth, kMaxScalarWidth);
    return ALLSET_ERR_UNSUPPORTED;
  }
  if (n_e == 0 || d == 0) return ALLSET_OK;
  ALLSET_REQUIRE(S && I && w && dinv && x && pq, "hypergcn_v2e: null S/I/w/dinv/x/pq");
  ALLSET_REQUIRE(ldx >= d && ldpq >= d, "hypergcn_v2e: leading dimension smaller than d");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int ne = static_cast<int>(n_e), di = static_cast<int>(d);
  if (!mediators) {
    const int vec = wc == 1 ? 4 : 1;
    const int chunks = (di + vec - 1) / vec;
    const unsigned grid = static_cast<unsigned>((n_e * chunks + kBlock - 1) / kBlock);
    if (wc == 1) v2e_pair_kernel<4><<<grid, kBlock, 0, st>>>(S, I, w, dinv, x, ldx, pq, ldpq, ne, di, chunks);
    else         v2e_pair_kernel<1><<<grid, kBlock, 0, st>>>(S, I, w, dinv, x, ldx, pq, ldpq, ne, di, chunks);
    ALLSET_LAUNCH_CHECK();
    return ALLSET_OK;
  }
  ALLSET_REQUIRE(rowptr && (nnz == 0 || col), "hypergcn_v2e: null rowptr/col");
  const unsigned grid = row_grid(n_e);
  with_vec_lpr<4>(wc == 1, d, [&](auto vec, auto lpr) {
    v2e_kernel<vec(), lpr()><<<grid, kBlock, 0, st>>>(rowptr, col, S, I, w, dinv, x, ldx, pq, ldpq, ne, di, row_order);
  });
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_hypergcn_e2v(int variant, int64_t nnz, const int32_t* row_order, const int32_t* rowptr, const int32_t* colx,
                                   const float* pq, int64_t ldpq, int64_t n_pq, const float* dinv, const float* selfc, const float* x,
                                   int64_t ldx, const float* bias, int act, float p, uint64_t seed, const uint64_t* seed_base, float* y,
                                   int64_t ldy, int64_t n_v, int64_t d, void* stream) {
  clear_error();
  ALLSET_REQUIRE(variant >= 0 && variant <= 2, "hypergcn_e2v: bad variant %d", variant);
  ALLSET_REQUIRE(act == kActNone || act == kActRelu, "hypergcn_e2v: bad act %d (none or relu)", act);
  ALLSET_REQUIRE(p >= 0.f && p < 1.f, "hypergcn_e2v: dropout p must be in [0,1)");
  ALLSET_REQUIRE(n_v >= 0 && n_pq >= 0 && d >= 0 && nnz >= 0, "hypergcn_e2v: negative size");
  ALLSET_REQUIRE(n_v < INT32_MAX && n_pq < INT32_MAX && nnz < INT32_MAX && n_v * d < INT64_MAX / 2, "hypergcn_e2v: size exceeds int32");
  const bool rows16 = (ldx % 4 == 0) && (ldpq % 4 == 0) && (ldy % 4 == 0) && aligned16(x) && aligned16(pq) && aligned16(y);
  const int wc = width_class(d, rows16);
  if (wc < 0) {
    set_error("hypergcn_e2v: width %lld is not built (multiples of 4 up to %d with 16-byte aligned rows, or any width up to %d)",
              static_cast<long long>(d), kMaxWidth, kMaxScalarWidth);
    return ALLSET_ERR_UNSUPPORTED;
  }
  if (variant == 2 && wc != 1) {
    set_error("hypergcn_e2v: the short-row variant needs 16-byte aligned rows");
    return ALLSET_ERR_UNSUPPORTED;
  }
  if (n_v == 0 || d == 0) return ALLSET_OK;
  ALLSET_REQUIRE(rowptr && dinv && selfc && x && y, "hypergcn_e2v: null rowptr/dinv/selfc/x/y");
  ALLSET_REQUIRE(ldx >= d && ldy >= d && ldpq >= d, "hypergcn_e2v: leading dimension smaller than d");
  ALLSET_REQUIRE(nnz == 0 || (colx && pq), "hypergcn_e2v: null colx/pq with nnz > 0");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const Tail tl{dinv, selfc, x, ldx, row_epi(bias, act, p, seed)};
  const int nv = static_cast<int>(n_v), di = static_cast<int>(d), npq = static_cast<int>(n_pq);
  const bool use_flat = wc == 1 && (variant == 2 || (variant == 0 && n_v > kFlatMinRows &&
                                                     static_cast<double>(nnz) < kFlatMaxMeanDegree * static_cast<double>(n_v)));
  if (use_flat) {
    with_lpr(pick_lpr(d), [&](auto lpr) {
      e2v_flat_kernel<lpr()><<<flat_grid<lpr()>(n_v), kBlock, 0, st>>>(rowptr, colx, pq, ldpq, npq, tl, seed_base, y, ldy, nv, di);
    });
  } else {
    with_vec_lpr<4>(wc == 1, d, [&](auto vec, auto lpr) {
      e2v_kernel<vec(), lpr()><<<row_grid(n_v), kBlock, 0, st>>>(rowptr, colx, pq, ldpq, npq, tl, seed_base, y, ldy, nv, di, row_order);
    });
  }
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}
