// The two hops of the plain UniGNN convs (reference models.py:601-907: UniGCNConv, UniGCNConv2, UniGINConv, UniSAGEConv,
// UniGATConv) with what the reference runs behind them as separate [N, d] / [M, d] torch ops in the same launch, for gfx950.
//
// K1  allset_unignn_hop_fwd -- the E->V sum hop with the whole row tail.  For every vertex row v of the vertex-major CSR:
//   a    = s[v] * sum_{j in row v} xe[col_j, :] + c * xs[v, :]
//   t    = use_norm ? (||a||_2 > 0 ? 1 / ||a||_2 : 0) : 1                        -> t_out[v] when use_norm
//   y[v] = drop_p(act(t * a))
// s (degV, or 1 / deg for UniSAGE's mean) and xs (the self term of UniGIN / UniSAGE) are optional; c is a host float or a
// device pointer to one float (UniGIN's 1 + eps is a parameter: a captured graph reads its value at every replay).  The
// self term enters BEFORE the norm, as in the reference.  t is the reference's normalize_l2 scale (from the detached row, a
// constant of the backward).  Dropout is the library's hash of (seed, v * d + column) with the seed_base counter of
// hconv.hip's epilogue, so allset_hconv_bwd_epi rebuilds mask and relu' from y.  The backward needs no gather kernel of its
// own: gxe = allset_hconv_fwd over the transposed CSR with r = s * t, gxs = c * t * g.
//
// K2  allset_unignn_v2e_att_fwd -- UniGAT's V->E hop with the attention logit in its epilogue.  For every hyperedge row e of
// the hyperedge-major CSR:
//   xe[e, :] = s[e] * sum_{v in e} x[v, :]
//   ae[e, h] = <xe[e, h, :], att[h, :]>                     h < H, C columns per head, taken from the row while in registers
// which saves the logit pass's read of [M, d].
//
// Mapping: unigcn.hip's, with the row's finish as a template parameter:
//   * one wavefront OWNS a whole output row: LPR lanes x 16 B per feature row, NS = 64 / LPR rows gathered per load; widths above
//     256 take two 16-byte packets per lane (NCH = 2, LPR = 64), so d <= 512 stays in registers and the row norm / the per-head
//     dot products are cross-lane reductions -- no second pass over the row, no atomics;
//   * the up-to-64 column ids of the row arrive in ONE coalesced load and are broadcast across the lanes, 8 gathers (4 x 2
//     packets at NCH = 2) in flight per slot;
//   * XCD-contiguous workgroup order, and the CSR's long-rows-first order (row_order) when the caller has one;
//   * a short-row variant (kFlatRows consecutive rows per LPR-lane group, one stream of incidences; d <= 256) below a mean
//     degree of 6: the lane group owns its rows, every reduction stays inside the group.
// Built for fp32, d a multiple of 4 up to 512 (K2: C a multiple of 4 as well), 16-byte aligned rows; anything else:
// ALLSET_ERR_UNSUPPORTED, the caller composes the hop from allset_hconv_fwd and torch ops.  Plain C++ and vector stores only;
// every sum has one fixed order: results are bit-identical from run to run.
// Algorithmic bytes per launch, K1: nnz * (4d + 4) + (n_t + 1) * 4 + n_t * 4d, plus n_t * 4d for xs and n_t * 4 each for s and
// t_out; K2: nnz * (4d + 4) + (n_t + 1) * 4 + n_t * (4d + 4H + 4) + 4d.
#include "common.h"
#include "flat_rows.h"
#include "row_epilogue.h"

namespace allset {
namespace unignn {

constexpr int kMaxWidth = 512;
constexpr int kFlatUnroll = 8;

// K1's row tail.  The LPR lanes that together hold row `row` call finish(): lane li has columns (ch * LPR + li) * 4 .. + 3 of the
// gathered sum in acc[ch] (zeros beyond d).  Every lane of the group calls it (the norm is reduced across them); `writer`
// lanes load the self term and store.  Not row_epilogue.h's RowEpi / row_epilogue: the row is scaled by t, has no bias and masks a
// quad with one keep_scale4; the activation and the threshold are the shared ones.
struct VertexTail {
  const float* s;         // per output row, or NULL (= ones)
  const float* xs;        // self-term rows, or NULL
  int64_t ldxs;
  const float* c_dev;     // device scalar, or NULL: then `c`
  float c;
  float* t_out;           // per output row; written when use_norm
  int use_norm;
  int act;
  float p;
  uint64_t seed;          // resolved (seed_base folded in) at kernel start
  uint32_t thr;
  float inv_keep;
  float* y;
  int64_t ldy;

  __device__ __forceinline__ void prepare(const uint64_t* seed_base) {
    seed = resolve_seed(seed_base, seed);
    if (c_dev) c = *c_dev;
  }

  template <int LPR, int NCH>
  __device__ __forceinline__ void finish(int row, int li, int d, float (&acc)[NCH][4], bool writer) const {
    const float sv = s ? s[row] : 1.f;
    float ss = 0.f;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c0 = (ch * LPR + li) * 4;
      FVec<4> z;
#pragma unroll
      for (int k = 0; k < 4; ++k) z.v[k] = 0.f;
      if (xs && writer && c0 < d) z = load_vec<float, 4>(xs + static_cast<int64_t>(row) * ldxs + c0);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        acc[ch][k] = fmaf(c, z.v[k], sv * acc[ch][k]);
        ss = fmaf(acc[ch][k], acc[ch][k], ss);
      }
    }
    float t = 1.f;
    if (use_norm) {
#pragma unroll
      for (int off = 1; off < LPR; off <<= 1) ss += __shfl_xor(ss, off);
      t = ss > 0.f ? 1.f / sqrtf(ss) : 0.f;
    }
    if (!writer) return;
    if (use_norm && li == 0) t_out[row] = t;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c0 = (ch * LPR + li) * 4;
      if (c0 < d) {
        float4 keep = make_float4(1.f, 1.f, 1.f, 1.f);
        if (p > 0.f) keep = keep_scale4(seed, static_cast<int64_t>(row) * d + c0, thr, inv_keep);
        const float kk[4] = {keep.x, keep.y, keep.z, keep.w};
        FVec<4> o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          o.v[k] = row_act<false>(t * acc[ch][k], act) * kk[k];
        }
        store_vec<float, 4>(y + static_cast<int64_t>(row) * ldy + c0, o);
      }
    }
  }
};

// K2's row finish: the per-hyperedge scale, the row store and the H per-head dot products with att.
struct EdgeLogit {
  const float* s;         // per output row, or NULL (= ones)
  const float* att;       // [H * C]
  float* xe;
  int64_t ldxe;
  float* ae;              // [n_t, H]
  int H, C;

  __device__ __forceinline__ void prepare(const uint64_t*) {}

  template <int LPR, int NCH>
  __device__ __forceinline__ void finish(int row, int li, int d, float (&acc)[NCH][4], bool writer) const {
    const float sv = s ? s[row] : 1.f;
    const int lph = C >> 2;                               // lanes per head
    float red[NCH];
    int head[NCH], first[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c0 = (ch * LPR + li) * 4;
      float part = 0.f;
      if (c0 < d) {
        const FVec<4> w = load_vec<float, 4>(att + c0);
        FVec<4> o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          o.v[k] = sv * acc[ch][k];
          part = fmaf(o.v[k], w.v[k], part);
        }
        if (writer) store_vec<float, 4>(xe + static_cast<int64_t>(row) * ldxe + c0, o);
      }
      // the head's lanes inside this chunk: [first, last) of the group's LPR lanes
      const int h = c0 / C;
      head[ch] = h;
      first[ch] = max(h * lph - ch * LPR, 0);
      const int last = min((h + 1) * lph - ch * LPR, LPR);
      red[ch] = head_group_reduce<LPR>(part, li, last);
    }
    if constexpr (NCH == 2) {
      // a head that straddles the two chunks (LPR = 64: columns 255 | 256): its second part sits in lane 0 of chunk 1
      const bool straddle = d > LPR * 4 && (LPR * 4) % C != 0;
      const float carry = __shfl(red[1], 0);
      if (straddle && li == first[0] && head[0] == (LPR * 4 - 1) / C) red[0] += carry;
      if (straddle && li == 0) first[1] = -1;             // (no lane writes that part on its own)
    }
    if (!writer) return;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c0 = (ch * LPR + li) * 4;
      if (c0 < d && li == first[ch]) ae[static_cast<int64_t>(row) * H + head[ch]] = red[ch];
    }
  }
};

template <int LPR, int NCH, class Finish>
__global__ __launch_bounds__(kBlock) void unignn_rows_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ x, int64_t ldx, Finish fin,
    int n_t, int d, const int32_t* __restrict__ row_order, const uint64_t* __restrict__ seed_base) {
  static_assert(NCH == 1 || LPR == kWave, "two packets per lane only with the whole wave on one row");
  constexpr int NS = kWave / LPR;
  constexpr int U = NCH == 1 ? 8 : 4;
  const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int slot_row = static_cast<int>(blk) * kWavesPerBlock + (threadIdx.x >> 6);
  if (slot_row >= n_t) return;  // whole wave exits together
  fin.prepare(seed_base);
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
          if (jj < n && c0 < d) raw[u][ch] = load_raw<float, 4>(x + static_cast<int64_t>(src) * ldx + c0);
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

  fin.template finish<LPR, NCH>(row, li, d, acc, slot == 0);
}

// short-row variant (flat_rows.h); single column chunk (d <= LPR * 4).  Every lane of the slot calls the finish: its reductions
// stay inside the slot.
template <int LPR, class Finish>
__global__ __launch_bounds__(kBlock) void unignn_flat_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ x, int64_t ldx, Finish fin,
    int n_t, int d, const uint64_t* __restrict__ seed_base) {
  FlatSlot<LPR> s;
  if (s.wave_beyond(n_t)) return;
  fin.prepare(seed_base);
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
        if (ok) raw[u] = load_raw<float, 4>(x + static_cast<int64_t>(src) * ldx + c0);
        else raw[u] = zero_raw<float, 4>();
      },
      [&](int u) {
        const FVec<4> v = unpack<float, 4>(raw[u]);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[0][k] += v.v[k];
      },
      [&] {
        fin.template finish<LPR, 1>(s.cur_row, s.li, d, acc, true);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[0][k] = 0.f;
      });
}

template <int LPR, int NCH, class Finish>
static void launch_rows(hipStream_t st, const int32_t* rowptr, const int32_t* col, const float* x, int64_t ldx, const Finish& fin,
                        int n_t, int d, const int32_t* row_order, const uint64_t* seed_base) {
  const unsigned grid = static_cast<unsigned>((static_cast<int64_t>(n_t) + kWavesPerBlock - 1) / kWavesPerBlock);
  unignn_rows_kernel<LPR, NCH, Finish><<<grid, kBlock, 0, st>>>(rowptr, col, x, ldx, fin, n_t, d, row_order, seed_base);
}

// variant 0 auto / 1 one wavefront per row / 2 short rows (the caller has checked that 2 comes with d <= 256)
template <class Finish>
static void dispatch(int variant, int64_t nnz, hipStream_t st, const int32_t* rowptr, const int32_t* col, const float* x, int64_t ldx,
                     const Finish& fin, int n_t, int d, const int32_t* row_order, const uint64_t* seed_base) {
  const bool use_flat = d <= 256 && (variant == 2 || (variant == 0 && n_t > kFlatMinRows &&
                                                      static_cast<double>(nnz) < kFlatMaxMeanDegree * static_cast<double>(n_t)));
  if (use_flat) {
    with_lpr(pick_lpr(d), [&](auto lpr) {
      unignn_flat_kernel<lpr(), Finish><<<flat_grid<lpr()>(n_t), kBlock, 0, st>>>(rowptr, col, x, ldx, fin, n_t, d, seed_base);
    });
  } else if (d > 256) {
    launch_rows<64, 2>(st, rowptr, col, x, ldx, fin, n_t, d, row_order, seed_base);
  } else {
    with_lpr(pick_lpr(d), [&](auto lpr) { launch_rows<lpr(), 1>(st, rowptr, col, x, ldx, fin, n_t, d, row_order, seed_base); });
  }
}

}  // namespace unignn
}  // namespace allset

using namespace allset;
using namespace allset::unignn;

extern "C" int allset_unignn_supported(void) { return 1; }

extern "C" int allset_unignn_hop_fwd(int variant, int64_t nnz, const int32_t* row_order, const int32_t* rowptr, const int32_t* col,
                                     const float* s, const float* xe, int64_t ldxe, const float* xs, int64_t ldxs, float c,
                                     const float* c_dev, int use_norm, int act, float p, uint64_t seed, const uint64_t* seed_base,
                                     float* y, int64_t ldy, float* t_out, int64_t n_t, int64_t n_s, int64_t d, void* stream) {
  clear_error();
  ALLSET_REQUIRE(variant >= 0 && variant <= 2, "unignn_hop_fwd: bad variant %d", variant);
  ALLSET_REQUIRE(act == kActNone || act == kActRelu, "unignn_hop_fwd: bad act %d", act);
  ALLSET_REQUIRE(p >= 0.f && p < 1.f, "unignn_hop_fwd: dropout p must be in [0,1)");
  ALLSET_REQUIRE(n_t >= 0 && n_s >= 0 && d >= 0 && nnz >= 0, "unignn_hop_fwd: negative size");
  ALLSET_REQUIRE(n_t < INT32_MAX && n_s < INT32_MAX && nnz < INT32_MAX, "unignn_hop_fwd: size exceeds int32");
  ALLSET_REQUIRE(c == c, "unignn_hop_fwd: c is NaN");
  if (d > kMaxWidth || d % 4 != 0) {
    set_error("unignn_hop_fwd: width %lld is not built (multiples of 4 up to the maximum %d)", static_cast<long long>(d), kMaxWidth);
    return ALLSET_ERR_UNSUPPORTED;
  }
  if (n_t == 0 || d == 0) return ALLSET_OK;
  ALLSET_REQUIRE(rowptr && y, "unignn_hop_fwd: null rowptr/y");
  ALLSET_REQUIRE(!use_norm || t_out, "unignn_hop_fwd: null t_out with use_norm");
  ALLSET_REQUIRE(ldxe >= d && ldy >= d && (!xs || ldxs >= d), "unignn_hop_fwd: leading dimension smaller than d");
  ALLSET_REQUIRE(nnz == 0 || (col && xe), "unignn_hop_fwd: null col/xe with nnz > 0");
  if (!((ldxe % 4 == 0) && (ldy % 4 == 0) && (!xs || ldxs % 4 == 0) && aligned16(xe) && aligned16(xs) && aligned16(y))) {
    set_error("unignn_hop_fwd: rows must be 16-byte aligned (pointers and leading dimensions)");
    return ALLSET_ERR_UNSUPPORTED;
  }
  if (variant == 2 && d > 256) {
    set_error("unignn_hop_fwd: the short-row variant needs d <= 256");
    return ALLSET_ERR_UNSUPPORTED;
  }
  const VertexTail tl{s, xs, ldxs, c_dev, c, t_out, use_norm ? 1 : 0, act, p, seed, drop_threshold(p), drop_inv_keep(p), y, ldy};
  dispatch(variant, nnz, static_cast<hipStream_t>(stream), rowptr, col, xe, ldxe, tl, static_cast<int>(n_t), static_cast<int>(d),
           row_order, seed_base);
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_unignn_v2e_att_fwd(int variant, int64_t nnz, const int32_t* row_order, const int32_t* rowptr, const int32_t* col,
                                         const float* s, const float* x, int64_t ldx, const float* att, float* xe, int64_t ldxe,
                                         float* ae, int64_t n_t, int64_t n_s, int64_t H, int64_t C, void* stream) {
  clear_error();
  ALLSET_REQUIRE(variant >= 0 && variant <= 2, "unignn_v2e_att_fwd: bad variant %d", variant);
  ALLSET_REQUIRE(n_t >= 0 && n_s >= 0 && H >= 0 && C >= 0 && nnz >= 0, "unignn_v2e_att_fwd: negative size");
  ALLSET_REQUIRE(n_t < INT32_MAX && n_s < INT32_MAX && nnz < INT32_MAX && H < INT32_MAX && C < INT32_MAX,
                 "unignn_v2e_att_fwd: size exceeds int32");
  const int64_t d = H * C;
  if (d > kMaxWidth || C % 4 != 0) {
    set_error("unignn_v2e_att_fwd: %lld heads of %lld channels are not built (channels a multiple of 4, heads * channels up to %d)",
              static_cast<long long>(H), static_cast<long long>(C), kMaxWidth);
    return ALLSET_ERR_UNSUPPORTED;
  }
  if (n_t == 0 || d == 0) return ALLSET_OK;
  ALLSET_REQUIRE(rowptr && xe && ae && att, "unignn_v2e_att_fwd: null rowptr/xe/ae/att");
  ALLSET_REQUIRE(ldx >= d && ldxe >= d, "unignn_v2e_att_fwd: leading dimension smaller than heads * channels");
  ALLSET_REQUIRE(nnz == 0 || (col && x), "unignn_v2e_att_fwd: null col/x with nnz > 0");
  if (!((ldx % 4 == 0) && (ldxe % 4 == 0) && aligned16(x) && aligned16(xe) && aligned16(att))) {
    set_error("unignn_v2e_att_fwd: rows must be 16-byte aligned (pointers and leading dimensions)");
    return ALLSET_ERR_UNSUPPORTED;
  }
  if (variant == 2 && d > 256) {
    set_error("unignn_v2e_att_fwd: the short-row variant needs heads * channels <= 256");
    return ALLSET_ERR_UNSUPPORTED;
  }
  const EdgeLogit fin{s, att, xe, ldxe, ae, static_cast<int>(H), static_cast<int>(C)};
  dispatch(variant, nnz, static_cast<hipStream_t>(stream), rowptr, col, x, ldx, fin, static_cast<int>(n_t), static_cast<int>(d),
           row_order, nullptr);
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}
