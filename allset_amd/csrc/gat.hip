// GAT attention hop of the clique-expansion baseline CEGAT (reference models.py:131-183; torch_geometric 1.6.3 GATConv) for gfx950:
//   e_j        = leaky_relu(al[col_j, h] + ar[t, h])                       j over the incidences of target row t
//   p_j        = exp(e_j - m[t,h]) / (l[t,h] + 1e-16),  m = max_j e_j,  l = sum_j exp(e_j - m)
//   agg[t,h,:] = sum_j p_j * x[col_j, h, :]
//   concat:      y[t, :]  = drop_p(act(agg[t, :] + bias[H*C]))
//   mean heads:  y[t, :C] = drop_p(act(mean_h agg[t,h,:] + bias[C]))
// The logit's non-linearity sits on the SUM of a source and a target term, so pma.hip's kernels (source-only logit) cannot be
// reused by folding one term away; the skeleton is theirs.
//
//   forward  (target-major CSR): one wavefront per row, LPR lanes x VEC floats per feature row, NS = 64 / LPR incidences per
//            wave-wide gather; every lane runs its own online softmax (its head's al[src] rides with the row gather, ar[t] is
//            loaded once per row), the NS slots merge at the end, the epilogue runs on the merged row in the same launch.  When
//            the caller will differentiate, a second accumulator keeps the POSITIVE-LOGIT part of the row,
//            aggpos[t,h,:] = sum_{e_j > 0} p_j x[col_j,h,:] and ppos[t,h] = sum_{e_j > 0} p_j (see gar below).
//   backward, target side (gat_bwd_stats, one pass over [n_t, H*C], no incidences): M = m + log(l + 1e-16),
//            delta = <agg, g>, and the whole of gar.  With lrelu' = slope + (1 - slope) [e > 0] and sum_j p_j = 1,
//              gar[t,h] = sum_j p_j lrelu'_j (<x_j, g_t> - delta) = (1 - slope) * (<aggpos[t,h,:], g[t,h,:]> - delta * ppos[t,h])
//            (the slope part is slope * (<agg, g> - delta) = 0): no per-incidence gradient is ever formed, no atomics, one
//            fixed summation order.  agg is read where the caller saved it (head-mean form) or rebuilt from the output,
//            agg = y * (1 - p) - bias, wherever g != 0 (where g == 0 the element was dropped or clipped and contributes nothing).
//   backward, source side (source-major CSR, gat_bwd_src): gx[s,h,:] = sum_j p_j g[t_j,h,:] and, by the same split,
//              gal[s,h] = slope * (<x_s, gx_s> - sum_j p_j delta_j) + (1 - slope) * (<x_s, gxpos_s> - sum_{e_j > 0} p_j delta_j)
//            so the dot products happen once per ROW on the accumulated vectors, as in pma_bwd_src.
// Algorithmic bytes: forward nnz * (4d + 4H + 4) + n_t * (4d [+ 4d aggpos] + 12H) ; stats 3 * n_t * 4d ; source pass
// nnz * (4d + 12H + 4) + n_s * 8d.  fp32 only.  Vector stores only.
#include <float.h>

#include "common.h"
#include "row_epilogue.h"

namespace allset {
namespace gat {

constexpr int kUnroll = 8;
constexpr int kMaxHeads = 64;            // one lane group per head in the stats kernel
constexpr int kMaxWidth = 512;           // H * C: the head-mean epilogue stages one row per wave in LDS
constexpr float kSoftmaxEps = 1e-16f;    // torch_geometric.utils.softmax denominator guard

template <int VEC, int LPR, bool POS>
__global__ __launch_bounds__(kBlock) void gat_fwd_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ al, const float* __restrict__ ar,
    const float* __restrict__ x, int64_t ldx, float slope, float* __restrict__ y, int64_t ldy, float* __restrict__ agg, int64_t lda,
    float* __restrict__ aggpos, int64_t ldp, float* __restrict__ ppos, float* __restrict__ m_out, float* __restrict__ l_out, int n_t,
    int H, int C, int concat, const int32_t* __restrict__ row_order, RowEpi epi, const uint64_t* __restrict__ seed_base) {
  constexpr int NS = kWave / LPR;
  __shared__ float stage[kWavesPerBlock][kMaxWidth];               // head-mean form: the row's agg, one wave's worth
  const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int wave = threadIdx.x >> 6;
  const int slot_row = static_cast<int>(blk) * kWavesPerBlock + wave;
  if (slot_row >= n_t) return;  // whole wave exits together
  const int row = row_order ? row_order[slot_row] : slot_row;
  epi.seed = resolve_seed(seed_base, epi.seed);
  const int lane = lane_id();
  const int slot = lane / LPR, li = lane % LPR;
  const int start = rowptr[row], end = rowptr[row + 1];
  const int d = H * C;

  for (int cb = 0; cb < d; cb += LPR * VEC) {
    const int c0 = cb + li * VEC;
    const bool active = c0 < d;
    const int h = active ? c0 / C : 0;
    const float ar_t = active ? ar[static_cast<int64_t>(row) * H + h] : 0.f;
    float m = -FLT_MAX, l = 0.f, lp = 0.f;
    float acc[VEC], accp[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) { acc[k] = 0.f; accp[k] = 0.f; }

    for (int base = start; base < end; base += kWave) {
      const int n = min(kWave, end - base);
      const int my_col = (lane < n) ? col[base + lane] : 0;
      for (int j = 0; j < n; j += NS * kUnroll) {
        Raw<float, VEC> raw[kUnroll];
        float a[kUnroll];
        bool ok[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const int jj = j + u * NS + slot;
          ok[u] = (jj < n) && active;
          const int src = __shfl(my_col, jj & (kWave - 1));
          if (ok[u]) {
            a[u] = al[static_cast<int64_t>(src) * H + h];
            raw[u] = load_raw<float, VEC>(x + static_cast<int64_t>(src) * ldx + c0);
          }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          if (ok[u]) {
            const FVec<VEC> vu = unpack<float, VEC>(raw[u]);
            const float e = a[u] + ar_t;
            const float av = leaky_relu(e, slope);
            const float m_new = fmaxf(m, av);
            const float sc = __expf(m - m_new);       // 0 on the first incidence (m = -FLT_MAX)
            const float pe = __expf(av - m_new);
            l = fmaf(l, sc, pe);
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = fmaf(acc[k], sc, pe * vu.v[k]);
            if constexpr (POS) {
              const float pp = e > 0.f ? pe : 0.f;
              lp = fmaf(lp, sc, pp);
#pragma unroll
              for (int k = 0; k < VEC; ++k) accp[k] = fmaf(accp[k], sc, pp * vu.v[k]);
            }
            m = m_new;
          }
        }
      }
    }

    // merge the NS slots' states
#pragma unroll
    for (int off = LPR; off < kWave; off <<= 1) {
      const float mo = __shfl_xor(m, off);
      const float lo = __shfl_xor(l, off);
      const float m_new = fmaxf(m, mo);
      const float s1 = __expf(m - m_new), s2 = __expf(mo - m_new);   // both -FLT_MAX -> exp(0) * (l = 0)
      l = l * s1 + lo * s2;
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = acc[k] * s1 + __shfl_xor(acc[k], off) * s2;
      if constexpr (POS) {
        lp = lp * s1 + __shfl_xor(lp, off) * s2;
#pragma unroll
        for (int k = 0; k < VEC; ++k) accp[k] = accp[k] * s1 + __shfl_xor(accp[k], off) * s2;
      }
      m = m_new;
    }

    if (slot == 0 && active) {
      const float inv = l > 0.f ? 1.f / (l + kSoftmaxEps) : 0.f;   // empty row -> 0
      FVec<VEC> r;
#pragma unroll
      for (int k = 0; k < VEC; ++k) r.v[k] = acc[k] * inv;
      if constexpr (POS) {
        FVec<VEC> rp;
#pragma unroll
        for (int k = 0; k < VEC; ++k) rp.v[k] = accp[k] * inv;
        store_vec<float, VEC>(aggpos + static_cast<int64_t>(row) * ldp + c0, rp);
      }
      if (c0 % C == 0) {
        const int64_t th = static_cast<int64_t>(row) * H + h;
        m_out[th] = l > 0.f ? m : 0.f;
        l_out[th] = l;
        if constexpr (POS) ppos[th] = lp * inv;
      }
      if (concat) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const int c = c0 + k;
          r.v[k] = row_epilogue<false>(epi, r.v[k], c, [=] { return static_cast<int64_t>(row) * d + c; });
        }
        store_vec<float, VEC>(y + static_cast<int64_t>(row) * ldy + c0, r);
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) stage[wave][c0 + k] = r.v[k];
        if (agg) store_vec<float, VEC>(agg + static_cast<int64_t>(row) * lda + c0, r);
      }
    }
  }
  if (!concat) {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    const float inv_h = 1.f / static_cast<float>(H);
    for (int c = lane; c < C; c += kWave) {
      float s = 0.f;
      for (int h = 0; h < H; ++h) s += stage[wave][h * C + c];
      y[static_cast<int64_t>(row) * ldy + c] = row_epilogue<false>(epi, s * inv_h, c, [=] { return static_cast<int64_t>(row) * C + c; });
    }
  }
}

// One wavefront per target row; LH = 64 / Hp lanes per head (Hp = H rounded up to a power of two), each striding its head's C
// channels.  Writes stats[t,h] = {M, delta} and gar[t,h].
__global__ __launch_bounds__(kBlock) void gat_bwd_stats_kernel(
    const float* __restrict__ y, int64_t ldy, const float* __restrict__ bias, float keep, const float* __restrict__ agg, int64_t lda,
    const float* __restrict__ aggpos, int64_t ldp, const float* __restrict__ ppos, const float* __restrict__ g, int64_t ldg,
    const float* __restrict__ m, const float* __restrict__ l, float slope, float* __restrict__ stats, float* __restrict__ gar,
    int n_t, int H, int C, int LH) {
  const int row = static_cast<int>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  if (row >= n_t) return;
  const int lane = lane_id();
  const int h = lane / LH, sub = lane % LH;
  float delta = 0.f, dpos = 0.f;
  if (h < H) {
    for (int c = sub; c < C; c += LH) {
      const int cc = h * C + c;
      const float gv = g[static_cast<int64_t>(row) * ldg + cc];
      if (gv != 0.f) {
        const float a = agg ? agg[static_cast<int64_t>(row) * lda + cc]
                            : y[static_cast<int64_t>(row) * ldy + cc] * keep - (bias ? bias[cc] : 0.f);
        delta = fmaf(a, gv, delta);
        dpos = fmaf(aggpos[static_cast<int64_t>(row) * ldp + cc], gv, dpos);
      }
    }
  }
  for (int off = 1; off < LH; off <<= 1) {
    delta += __shfl_xor(delta, off);
    dpos += __shfl_xor(dpos, off);
  }
  if (h < H && sub == 0) {
    const int64_t th = static_cast<int64_t>(row) * H + h;
    const float lv = l[th];
    float2 s;
    s.x = lv > 0.f ? m[th] + logf(lv + kSoftmaxEps) : FLT_MAX;     // empty target: never gathered
    s.y = delta;
    *reinterpret_cast<float2*>(stats + th * 2) = s;
    gar[th] = (1.f - slope) * (dpos - delta * ppos[th]);
  }
}

template <int VEC, int LPR>
__global__ __launch_bounds__(kBlock) void gat_bwd_src_kernel(
    const int32_t* __restrict__ rowptrT, const int32_t* __restrict__ colT, const float* __restrict__ al, const float* __restrict__ ar,
    const float* __restrict__ x, int64_t ldx, const float* __restrict__ g, int64_t ldg, const float* __restrict__ stats, float slope,
    float* __restrict__ gx, int64_t ldgx, float* __restrict__ gal, int n_s, int H, int C, const int32_t* __restrict__ row_order) {
  constexpr int NS = kWave / LPR;
  __shared__ float red[kWavesPerBlock][kMaxHeads];
  const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int wave = threadIdx.x >> 6;
  const int slot_row = static_cast<int>(blk) * kWavesPerBlock + wave;
  if (slot_row >= n_s) return;
  const int row = row_order ? row_order[slot_row] : slot_row;
  const int lane = lane_id();
  const int slot = lane / LPR, li = lane % LPR;
  const int start = rowptrT[row], end = rowptrT[row + 1];
  const int d = H * C, G = C / VEC;
  for (int h = lane; h < H; h += kWave) red[wave][h] = 0.f;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");

  for (int cb = 0; cb < d; cb += LPR * VEC) {
    const int c0 = cb + li * VEC;
    const bool active = c0 < d;
    const int h = active ? c0 / C : 0;
    const int q = active ? (c0 % C) / VEC : 0;
    FVec<VEC> vown;
    float al_s = 0.f;
    if (active) {
      vown = load_vec<float, VEC>(x + static_cast<int64_t>(row) * ldx + c0);
      al_s = al[static_cast<int64_t>(row) * H + h];
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) vown.v[k] = 0.f;
    }
    float gv[VEC], gvp[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) { gv[k] = 0.f; gvp[k] = 0.f; }
    float D = 0.f, Dp = 0.f;

    for (int base = start; base < end; base += kWave) {
      const int n = min(kWave, end - base);
      const int my_col = (lane < n) ? colT[base + lane] : 0;
      for (int j = 0; j < n; j += NS * kUnroll) {
        Raw<float, VEC> gr[kUnroll];
        float2 st[kUnroll];
        float art[kUnroll];
        bool ok[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const int jj = j + u * NS + slot;
          ok[u] = (jj < n) && active;
          const int t = __shfl(my_col, jj & (kWave - 1));
          if (ok[u]) {
            gr[u] = load_raw<float, VEC>(g + static_cast<int64_t>(t) * ldg + c0);
            st[u] = *reinterpret_cast<const float2*>(stats + (static_cast<int64_t>(t) * H + h) * 2);
            art[u] = ar[static_cast<int64_t>(t) * H + h];
          }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          if (ok[u]) {
            const float e = al_s + art[u];
            const float p = __expf(leaky_relu(e, slope) - st[u].x);
            const float pp = e > 0.f ? p : 0.f;
            const FVec<VEC> gu = unpack<float, VEC>(gr[u]);
#pragma unroll
            for (int k = 0; k < VEC; ++k) { gv[k] = fmaf(p, gu.v[k], gv[k]); gvp[k] = fmaf(pp, gu.v[k], gvp[k]); }
            D = fmaf(p, st[u].y, D);
            Dp = fmaf(pp, st[u].y, Dp);
          }
        }
      }
    }
#pragma unroll
    for (int off = LPR; off < kWave; off <<= 1) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) { gv[k] += __shfl_xor(gv[k], off); gvp[k] += __shfl_xor(gvp[k], off); }
      D += __shfl_xor(D, off);
      Dp += __shfl_xor(Dp, off);
    }
    // sum_j w_j <x_s, g_j> = <x_s, sum_j w_j g_j> for w = p and w = p [e > 0]: no per-incidence dot product
    float S = 0.f, Sp = 0.f;
#pragma unroll
    for (int k = 0; k < VEC; ++k) { S = fmaf(vown.v[k], gv[k], S); Sp = fmaf(vown.v[k], gvp[k], Sp); }
    if (slot == 0 && active) {
      FVec<VEC> r;
#pragma unroll
      for (int k = 0; k < VEC; ++k) r.v[k] = gv[k];
      store_vec<float, VEC>(gx + static_cast<int64_t>(row) * ldgx + c0, r);
    }
    // per head: the lanes' dot-product parts summed, the (lane-uniform) delta sums subtracted once, where the head begins
    const int n_act = min(LPR, (d - cb) / VEC);
    const int grp_end = min(li - q + G, n_act);
    float part = (slot == 0 && active) ? slope * S + (1.f - slope) * Sp : 0.f;
    part = head_group_reduce<LPR>(part, li, grp_end);
    // (one lane per head and chunk: the head's first lane, or lane 0 for a head continuing from the previous chunk)
    if (slot == 0 && active && (q == 0 || li == 0)) red[wave][h] += part - (q == 0 ? slope * D + (1.f - slope) * Dp : 0.f);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
  for (int h = lane; h < H; h += kWave) gal[static_cast<int64_t>(row) * H + h] = red[wave][h];
}

static int check_dims(const char* who, int64_t n_a, int64_t n_b, int64_t H, int64_t C) {
  ALLSET_REQUIRE(n_a >= 0 && n_b >= 0, "%s: negative size", who);
  ALLSET_REQUIRE(n_a < INT32_MAX && n_b < INT32_MAX, "%s: size exceeds int32", who);
  ALLSET_REQUIRE(H >= 1 && C >= 1, "%s: heads/channels must be >= 1", who);
  if (H > kMaxHeads || C > kMaxWidth || H * C > kMaxWidth) {
    set_error("%s: heads=%lld x channels=%lld exceeds the built maximum (heads <= %d, heads * channels <= %d)", who,
              static_cast<long long>(H), static_cast<long long>(C), kMaxHeads, kMaxWidth);
    return ALLSET_ERR_UNSUPPORTED;
  }
  return ALLSET_OK;
}

#define ALLSET_GAT_DISPATCH(LAUNCH)                        \
  do {                                                     \
    if (wide_ok) {                                         \
      switch (pick_lpr(d, 4)) {                            \
        case 8:  LAUNCH(4, 8); break;                      \
        case 16: LAUNCH(4, 16); break;                     \
        case 32: LAUNCH(4, 32); break;                     \
        default: LAUNCH(4, 64); break;                     \
      }                                                    \
    } else {                                               \
      switch (pick_lpr(d, 1)) {                            \
        case 8:  LAUNCH(1, 8); break;                      \
        case 16: LAUNCH(1, 16); break;                     \
        case 32: LAUNCH(1, 32); break;                     \
        default: LAUNCH(1, 64); break;                     \
      }                                                    \
    }                                                      \
  } while (0)

}  // namespace gat
}  // namespace allset

using namespace allset;
using namespace allset::gat;

extern "C" int allset_gat_supported(void) { return 1; }

extern "C" int allset_gat_fwd(int variant, int64_t nnz, const int32_t* row_order, const int32_t* rowptr, const int32_t* col,
                              const float* al, const float* ar, const float* x, int64_t ldx, float slope, const float* bias, int act,
                              float p, uint64_t seed, const uint64_t* seed_base, int concat, float* y, int64_t ldy, float* agg,
                              int64_t ldagg, float* aggpos, int64_t ldpos, float* ppos, float* m, float* l, int64_t n_t, int64_t n_s,
                              int64_t H, int64_t C, void* stream) {
  clear_error();
  ALLSET_REQUIRE(variant >= 0 && variant <= 2, "gat_fwd: bad variant %d", variant);
  ALLSET_REQUIRE(act == kActNone || act == kActRelu, "gat_fwd: act must be none (0) or relu (1), got %d", act);
  ALLSET_REQUIRE(p >= 0.f && p < 1.f, "gat_fwd: dropout p must be in [0,1)");
  ALLSET_REQUIRE(nnz >= 0, "gat_fwd: negative size");
  int rc = check_dims("gat_fwd", n_t, n_s, H, C);
  if (rc != ALLSET_OK) return rc;
  if (variant == 2) {
    set_error("gat_fwd: the short-row variant is not built; use 0 or 1 (one wavefront per row)");
    return ALLSET_ERR_UNSUPPORTED;
  }
  if (n_t == 0) return ALLSET_OK;
  const int64_t d = H * C, dy = concat ? d : C;
  ALLSET_REQUIRE(rowptr && y && m && l && ar, "gat_fwd: null rowptr/y/m/l/ar");
  ALLSET_REQUIRE(nnz == 0 || (col && x && al), "gat_fwd: null col/x/al with nnz > 0");
  ALLSET_REQUIRE((aggpos == nullptr) == (ppos == nullptr), "gat_fwd: aggpos and ppos go together");
  ALLSET_REQUIRE(ldx >= d && ldy >= dy && (!agg || ldagg >= d) && (!aggpos || ldpos >= d), "gat_fwd: leading dimension smaller than the row");
  const bool wide_ok = (C % 4 == 0) && (ldx % 4 == 0) && aligned16(x) && (!concat || (ldy % 4 == 0 && aligned16(y))) &&
                       (!agg || (ldagg % 4 == 0 && aligned16(agg))) && (!aggpos || (ldpos % 4 == 0 && aligned16(aggpos)));
  const RowEpi e = row_epi(bias, act, p, seed);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned grid = row_grid(n_t);
#define ALLSET_GAT_FWD(VEC, LPR)                                                                                                   \
  do {                                                                                                                             \
    if (aggpos) gat_fwd_kernel<VEC, LPR, true><<<grid, kBlock, 0, st>>>(rowptr, col, al, ar, x, ldx, slope, y, ldy, agg, ldagg, aggpos,    \
        ldpos, ppos, m, l, static_cast<int>(n_t), static_cast<int>(H), static_cast<int>(C), concat ? 1 : 0, row_order, e, seed_base);       \
    else gat_fwd_kernel<VEC, LPR, false><<<grid, kBlock, 0, st>>>(rowptr, col, al, ar, x, ldx, slope, y, ldy, agg, ldagg, aggpos,          \
        ldpos, ppos, m, l, static_cast<int>(n_t), static_cast<int>(H), static_cast<int>(C), concat ? 1 : 0, row_order, e, seed_base);       \
  } while (0)
  ALLSET_GAT_DISPATCH(ALLSET_GAT_FWD);
#undef ALLSET_GAT_FWD
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_gat_bwd_stats(const float* y, int64_t ldy, const float* bias, float p, const float* agg, int64_t ldagg,
                                    const float* aggpos, int64_t ldpos, const float* ppos, const float* g, int64_t ldg, const float* m,
                                    const float* l, float slope, float* stats, float* gar, int64_t n_t, int64_t H, int64_t C,
                                    void* stream) {
  clear_error();
  ALLSET_REQUIRE(p >= 0.f && p < 1.f, "gat_bwd_stats: dropout p must be in [0,1)");
  int rc = check_dims("gat_bwd_stats", n_t, 0, H, C);
  if (rc != ALLSET_OK) return rc;
  if (n_t == 0) return ALLSET_OK;
  const int64_t d = H * C;
  ALLSET_REQUIRE((agg || y) && aggpos && ppos && g && m && l && stats && gar, "gat_bwd_stats: null pointer");
  ALLSET_REQUIRE(ldg >= d && ldpos >= d && (agg ? ldagg >= d : ldy >= d), "gat_bwd_stats: leading dimension smaller than H*C");
  ALLSET_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 7u) == 0, "gat_bwd_stats: stats must be 8-byte aligned");
  int hp = 1;
  while (hp < H) hp <<= 1;
  gat_bwd_stats_kernel<<<row_grid(n_t), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      y, ldy, bias, 1.f - p, agg, ldagg, aggpos, ldpos, ppos, g, ldg, m, l, slope, stats, gar, static_cast<int>(n_t),
      static_cast<int>(H), static_cast<int>(C), kWave / hp);
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_gat_bwd_src(int variant, int64_t nnz, const int32_t* row_order, const int32_t* rowptrT, const int32_t* colT,
                                  const float* al, const float* ar, const float* x, int64_t ldx, const float* g, int64_t ldg,
                                  const float* stats, float slope, float* gx, int64_t ldgx, float* gal, int64_t n_s, int64_t n_t,
                                  int64_t H, int64_t C, void* stream) {
  clear_error();
  ALLSET_REQUIRE(variant >= 0 && variant <= 2, "gat_bwd_src: bad variant %d", variant);
  ALLSET_REQUIRE(nnz >= 0, "gat_bwd_src: negative size");
  int rc = check_dims("gat_bwd_src", n_s, n_t, H, C);
  if (rc != ALLSET_OK) return rc;
  if (variant == 2) {
    set_error("gat_bwd_src: the short-row variant is not built; use 0 or 1 (one wavefront per row)");
    return ALLSET_ERR_UNSUPPORTED;
  }
  if (n_s == 0) return ALLSET_OK;
  const int64_t d = H * C;
  ALLSET_REQUIRE(rowptrT && al && x && gx && gal, "gat_bwd_src: null pointer");
  ALLSET_REQUIRE(nnz == 0 || (colT && ar && g && stats), "gat_bwd_src: null colT/ar/g/stats with nnz > 0");
  ALLSET_REQUIRE(ldx >= d && ldg >= d && ldgx >= d, "gat_bwd_src: leading dimension smaller than H*C");
  ALLSET_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 7u) == 0, "gat_bwd_src: stats must be 8-byte aligned");
  const bool wide_ok = (C % 4 == 0) && (ldx % 4 == 0) && (ldg % 4 == 0) && (ldgx % 4 == 0) && aligned16(x) && aligned16(g) && aligned16(gx);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned grid = row_grid(n_s);
#define ALLSET_GAT_BWD(VEC, LPR)                                                                                                  \
  gat_bwd_src_kernel<VEC, LPR><<<grid, kBlock, 0, st>>>(rowptrT, colT, al, ar, x, ldx, g, ldg, stats, slope, gx, ldgx, gal,        \
                                                        static_cast<int>(n_s), static_cast<int>(H), static_cast<int>(C), row_order)
  ALLSET_GAT_DISPATCH(ALLSET_GAT_BWD);
#undef ALLSET_GAT_BWD
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}
