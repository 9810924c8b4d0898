// Hypergraph attention of HCHA's HypergraphConv(use_attention=True) (reference layers.py:405-490) for gfx950.  Incidences
// j = (v_j, e_j); Z [n_v, H*C]; av [n_v, H], ae [n_e, H] the per-row logit terms:
//   l_j      = leaky_relu(av[v_j,h] + ae[e_j,h])
//   alpha_j  = exp(l_j - m[v_j,h]) / (sum_{k: v_k = v_j} exp(l_k - m) + 1e-16)          softmax over the hyperedges OF A VERTEX
//   a_j      = alpha_j * keep_j / (1 - p)                                               one draw, used by both hops
//   Y[e,h,:] = B[e] * sum_{j: e_j = e} a_j * Z[v_j,h,:]                                  hop 1, grouped by hyperedge
//   U[v,h,:] = D[v] * sum_{j: v_j = v} a_j * Y[e_j,h,:]                                  hop 2, grouped by vertex
//   out      = drop_p(act(concat_h or mean_h U + bias))
// The coefficient is normalised over one grouping and consumed under both, so gat.hip's hop (softmax over the incidences of the
// row being written) does not apply: the coefficient is made once, vertex-major, as an [nnz, H] array in BOTH CSR orders (the
// position map between the two orders comes from the CSRs' perm), and each hop is a gather with a per-(incidence, head) weight.
//
//   hattn_coef        vertex-major CSR, one wavefront per vertex: m, l per (v, h), then a_j written in vertex-major order and, through
//                     the position map, in hyperedge-major order.  The dropout key is (edge-list position of the incidence) * H + h.
//   hattn_hop         y[t,h,:] = epilogue(s[t] * sum_j w[j,h] * r[col_j] * x[col_j,h,:]) over either CSR: hop 1 (w = a in
//                     hyperedge-major order, s = B), hop 2 (w = a in vertex-major order, s = D, the epilogue in the launch) and, in
//                     the backward, hop 2 transposed: gY[e,h,:] = sum_{j in e} a_j * D[v_j] * G[v_j,h,:].
//   hattn_bwd_vertex  vertex-major, one gather pass over the rows Y[e_j] and gY[e_j] of the vertex's hyperedges:
//                       gZ[v,h,:] = sum_j a_j B[e_j] gY[e_j,h,:]                                   (hop 1 transposed)
//                       t_j       = a_j * (D[v] <G[v,h], Y[e_j,h]> + B[e_j] <gY[e_j,h], Z[v,h]>)    (a_j * dL/da_j, both hops' terms)
//                     then, over the [deg, H] scalars only, with delta = sum_k t_k (kept in registers, one fixed order):
//                       gl_j = t_j - alpha_j * delta ;  ge_j = gl_j * (slope + (1 - slope) [pre_j > 0])
//                       gav[v,h] = sum_j ge_j ;  ge_j also written in hyperedge-major order
//   hattn_bwd_edge    gae[e,h] = sum_{j in e} ge_j: a segment sum of the [nnz, H] array in its own order.
// No float atomics, every reduction is a segment sum over one of the two CSR orientations in a fixed order; nothing of shape
// [nnz, H*C] exists.  Lanes: a wavefront per row; a lane group of GW = Hp * LH lanes per incidence (Hp = H rounded up to a power of
// two, LH lanes per head, each lane NPL packets of VEC floats, c = (k * LH + sub) * VEC), NS = 64 / GW incidences per wave-wide
// gather; a head's dot product is an xor-shuffle reduction over its LH lanes, the head mean one over the Hp groups.
// Algorithmic bytes per launch (d = H*C): coef nnz * (8 + 12H) + n_v * 12H ; hop nnz * (4d + 4H + 4 [+4 r]) + n_t * 4d ;
// bwd_vertex nnz * (8d + 12H + 16) + n_v * (12d + 8H) ; bwd_edge nnz * 4H + n_e * 4H.  fp32 only.  Vector stores only.
#include <float.h>

#include "common.h"
#include "row_epilogue.h"

namespace allset {
namespace hattn {

constexpr int kUnroll = 4;
constexpr int kMaxHeads = 64;
constexpr int kMaxWidth = 512;
constexpr float kSoftmaxEps = 1e-16f;    // torch_geometric.utils.softmax denominator guard

struct Geo {
  int H, C;
  int LH;     // lanes per head (power of two)
  int GW;     // lanes per incidence slot = Hp * LH (power of two, <= 64)
};

// One wavefront per vertex; lanes stride the vertex's incidences, heads in turn.
__global__ __launch_bounds__(kBlock) void hattn_coef_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int32_t* __restrict__ perm,
    const int32_t* __restrict__ pos, const float* __restrict__ av, const float* __restrict__ ae, float slope, float p, uint64_t seed,
    const uint64_t* __restrict__ seed_base, uint32_t thr, float inv_keep, float* __restrict__ a_v, float* __restrict__ a_e,
    float* __restrict__ m_out, float* __restrict__ l_out, int n_v, int H) {
  const int row = static_cast<int>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  if (row >= n_v) return;
  seed = resolve_seed(seed_base, seed);
  const int lane = lane_id();
  const int start = rowptr[row], end = rowptr[row + 1];
  for (int h = 0; h < H; ++h) {
    const float av_h = av[static_cast<int64_t>(row) * H + h];
    float mx = -FLT_MAX;
    for (int j = start + lane; j < end; j += kWave)
      mx = fmaxf(mx, leaky_relu(av_h + ae[static_cast<int64_t>(col[j]) * H + h], slope));
    mx = wave_max(mx);
    float sum = 0.f;
    for (int j = start + lane; j < end; j += kWave)
      sum += __expf(leaky_relu(av_h + ae[static_cast<int64_t>(col[j]) * H + h], slope) - mx);
    sum = wave_sum(sum);
    if (lane == 0) {
      m_out[static_cast<int64_t>(row) * H + h] = end > start ? mx : 0.f;
      l_out[static_cast<int64_t>(row) * H + h] = sum;
    }
    const float inv = 1.f / (sum + kSoftmaxEps);
    for (int j = start + lane; j < end; j += kWave) {
      float a = __expf(leaky_relu(av_h + ae[static_cast<int64_t>(col[j]) * H + h], slope) - mx) * inv;
      if (p > 0.f) a *= keep_scale(seed, static_cast<int64_t>(perm[j]) * H + h, thr, inv_keep);
      a_v[static_cast<int64_t>(j) * H + h] = a;
      a_e[static_cast<int64_t>(pos[j]) * H + h] = a;
    }
  }
}

template <int VEC, int NPL>
__global__ __launch_bounds__(kBlock) void hattn_hop_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ w, const float* __restrict__ r,
    const float* __restrict__ s, const float* __restrict__ x, int64_t ldx, float* __restrict__ y, int64_t ldy, int n_t, Geo g,
    int concat, const int32_t* __restrict__ row_order, RowEpi epi, const uint64_t* __restrict__ seed_base) {
  const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int slot_row = static_cast<int>(blk) * kWavesPerBlock + (threadIdx.x >> 6);
  if (slot_row >= n_t) return;  // whole wave exits together
  const int row = row_order ? row_order[slot_row] : slot_row;
  epi.seed = resolve_seed(seed_base, epi.seed);
  const int lane = lane_id();
  const int slot = lane / g.GW, h = (lane % g.GW) / g.LH, sub = lane % g.LH;
  const int NS = kWave / g.GW;
  const bool hact = h < g.H;
  const int start = rowptr[row], end = rowptr[row + 1];
  bool on[NPL];
  int cofs[NPL];
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    const int c = (k * g.LH + sub) * VEC;
    on[k] = hact && c < g.C;
    cofs[k] = h * g.C + c;
  }
  float acc[NPL][VEC];
#pragma unroll
  for (int k = 0; k < NPL; ++k)
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[k][i] = 0.f;

  for (int base = start; base < end; base += kWave) {
    const int n = min(kWave, end - base);
    int my_col = 0;
    float my_r = 1.f;
    if (lane < n) {
      my_col = col[base + lane];
      if (r) my_r = r[my_col];
    }
    for (int j = 0; j < n; j += NS * kUnroll) {
      Raw<float, VEC> raw[kUnroll][NPL];
      float ww[kUnroll];
      bool ok[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int jj = j + u * NS + slot;
        ok[u] = (jj < n) && hact;
        const int src = __shfl(my_col, jj & (kWave - 1));
        const float rr = __shfl(my_r, jj & (kWave - 1));
        ww[u] = 0.f;
        if (ok[u]) {
          ww[u] = w[static_cast<int64_t>(base + jj) * g.H + h] * rr;
#pragma unroll
          for (int k = 0; k < NPL; ++k)
            if (on[k]) raw[u][k] = load_raw<float, VEC>(x + static_cast<int64_t>(src) * ldx + cofs[k]);
        }
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        if (ok[u]) {
#pragma unroll
          for (int k = 0; k < NPL; ++k) {
            if (on[k]) {
              const FVec<VEC> v = unpack<float, VEC>(raw[u][k]);
#pragma unroll
              for (int i = 0; i < VEC; ++i) acc[k][i] = fmaf(ww[u], v.v[i], acc[k][i]);
            }
          }
        }
      }
    }
  }
  // merge the NS slots, then (head-mean form) the Hp head groups: lanes of a head beyond H hold zeros
  const float sc = s ? s[row] : 1.f;
  const int red_to = concat ? g.GW : g.LH;
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      float v = acc[k][i];
      for (int off = kWave / 2; off >= red_to; off >>= 1) v += __shfl_xor(v, off);
      acc[k][i] = v * sc;
    }
  }
  if (slot != 0) return;
  if (concat) {
    const int d = g.H * g.C;
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      if (on[k]) {
        FVec<VEC> o;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const int c = cofs[k] + i;
          o.v[i] = row_epilogue<true>(epi, acc[k][i], c, [=] { return static_cast<int64_t>(row) * d + c; });
        }
        store_vec<float, VEC>(y + static_cast<int64_t>(row) * ldy + cofs[k], o);
      }
    }
  } else if (h == 0) {
    const float inv_h = 1.f / static_cast<float>(g.H);
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      if (on[k]) {
        FVec<VEC> o;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const int c = cofs[k] + i;
          o.v[i] = row_epilogue<true>(epi, acc[k][i] * inv_h, c, [=] { return static_cast<int64_t>(row) * g.C + c; });
        }
        store_vec<float, VEC>(y + static_cast<int64_t>(row) * ldy + cofs[k], o);
      }
    }
  }
}

template <int VEC, int NPL>
__global__ __launch_bounds__(kBlock) void hattn_bwd_vertex_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int32_t* __restrict__ pos,
    const float* __restrict__ a_v, const float* __restrict__ av, const float* __restrict__ ae, const float* __restrict__ m,
    const float* __restrict__ l, float slope, const float* __restrict__ z, int64_t ldz, const float* __restrict__ gu, int64_t ldg,
    const float* __restrict__ yv, int64_t ldy, const float* __restrict__ gy, int64_t ldgy, const float* __restrict__ D,
    const float* __restrict__ B, float* __restrict__ gz, int64_t ldgz, float* __restrict__ t, float* __restrict__ gav,
    float* __restrict__ ge_e, int n_v, Geo g) {
  constexpr int kU = 2;
  const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int row = static_cast<int>(blk) * kWavesPerBlock + (threadIdx.x >> 6);
  if (row >= n_v) return;
  const int lane = lane_id();
  const int slot = lane / g.GW, h = (lane % g.GW) / g.LH, sub = lane % g.LH;
  const int NS = kWave / g.GW;
  const bool hact = h < g.H;
  const int start = rowptr[row], end = rowptr[row + 1];
  const float d_v = D[row];
  bool on[NPL];
  int cofs[NPL];
  float zv[NPL][VEC], gv[NPL][VEC], gz1[NPL][VEC];
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    const int c = (k * g.LH + sub) * VEC;
    on[k] = hact && c < g.C;
    cofs[k] = h * g.C + c;
#pragma unroll
    for (int i = 0; i < VEC; ++i) { zv[k][i] = 0.f; gv[k][i] = 0.f; gz1[k][i] = 0.f; }
    if (on[k]) {
      const FVec<VEC> a = load_vec<float, VEC>(z + static_cast<int64_t>(row) * ldz + cofs[k]);
      const FVec<VEC> b = load_vec<float, VEC>(gu + static_cast<int64_t>(row) * ldg + cofs[k]);
#pragma unroll
      for (int i = 0; i < VEC; ++i) { zv[k][i] = a.v[i]; gv[k][i] = b.v[i] * d_v; }
    }
  }
  float delta = 0.f;

  for (int base = start; base < end; base += kWave) {
    const int n = min(kWave, end - base);
    int my_col = 0;
    float my_b = 0.f;
    if (lane < n) {
      my_col = col[base + lane];
      my_b = B[my_col];
    }
    for (int j = 0; j < n; j += NS * kU) {
      Raw<float, VEC> ry[kU][NPL], rg[kU][NPL];
      float ww[kU], be[kU];
      bool ok[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int jj = j + u * NS + slot;
        ok[u] = (jj < n) && hact;
        const int e = __shfl(my_col, jj & (kWave - 1));
        be[u] = __shfl(my_b, jj & (kWave - 1));
        ww[u] = 0.f;
        if (ok[u]) {
          ww[u] = a_v[static_cast<int64_t>(base + jj) * g.H + h];
#pragma unroll
          for (int k = 0; k < NPL; ++k) {
            if (on[k]) {
              ry[u][k] = load_raw<float, VEC>(yv + static_cast<int64_t>(e) * ldy + cofs[k]);
              rg[u][k] = load_raw<float, VEC>(gy + static_cast<int64_t>(e) * ldgy + cofs[k]);
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        float dot_y = 0.f, dot_g = 0.f;
        if (ok[u]) {
          const float wb = ww[u] * be[u];
#pragma unroll
          for (int k = 0; k < NPL; ++k) {
            if (on[k]) {
              const FVec<VEC> vy = unpack<float, VEC>(ry[u][k]);
              const FVec<VEC> vg = unpack<float, VEC>(rg[u][k]);
#pragma unroll
              for (int i = 0; i < VEC; ++i) {
                dot_y = fmaf(gv[k][i], vy.v[i], dot_y);
                dot_g = fmaf(zv[k][i], vg.v[i], dot_g);
                gz1[k][i] = fmaf(wb, vg.v[i], gz1[k][i]);
              }
            }
          }
        }
        float dot = ok[u] ? fmaf(be[u], dot_g, dot_y) : 0.f;
        for (int off = 1; off < g.LH; off <<= 1) dot += __shfl_xor(dot, off);     // (every lane takes part: no shuffle under a branch)
        if (ok[u]) {
          const float tj = ww[u] * dot;
          delta += tj;
          if (sub == 0) t[static_cast<int64_t>(base + j + u * NS + slot) * g.H + h] = tj;
        }
      }
    }
  }
  for (int off = g.GW; off < kWave; off <<= 1) {
    delta += __shfl_xor(delta, off);
#pragma unroll
    for (int k = 0; k < NPL; ++k)
#pragma unroll
      for (int i = 0; i < VEC; ++i) gz1[k][i] += __shfl_xor(gz1[k][i], off);
  }
  if (slot == 0) {
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      if (on[k]) {
        FVec<VEC> o;
#pragma unroll
        for (int i = 0; i < VEC; ++i) o.v[i] = gz1[k][i];
        store_vec<float, VEC>(gz + static_cast<int64_t>(row) * ldgz + cofs[k], o);
      }
    }
  }
  // t[] written above by this wavefront's head lanes is read below by its incidence-striding lanes: workgroup scope orders the two
  // through the CU's own L1 (an agent-scope fence would write the whole L2 back, once per row)
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");

  for (int hh = 0; hh < g.H; ++hh) {
    const float delta_h = __shfl(delta, hh * g.LH);
    const int64_t vh = static_cast<int64_t>(row) * g.H + hh;
    const float av_h = av[vh], m_h = m[vh];
    const float inv = 1.f / (l[vh] + kSoftmaxEps);
    float sum = 0.f;
    for (int j = start + lane; j < end; j += kWave) {
      const float pre = av_h + ae[static_cast<int64_t>(col[j]) * g.H + hh];
      const float alpha = __expf(leaky_relu(pre, slope) - m_h) * inv;
      const float gl = t[static_cast<int64_t>(j) * g.H + hh] - alpha * delta_h;
      const float ge = pre > 0.f ? gl : gl * slope;
      ge_e[static_cast<int64_t>(pos[j]) * g.H + hh] = ge;
      sum += ge;
    }
    sum = wave_sum(sum);
    if (lane == 0) gav[vh] = sum;
  }
}

// One wavefront per hyperedge: gae[e,h] = sum of ge[j,h] over the row's own (contiguous) positions.
__global__ __launch_bounds__(kBlock) void hattn_bwd_edge_kernel(const int32_t* __restrict__ rowptr, const float* __restrict__ ge,
                                                                 float* __restrict__ gae, int n_e, int H) {
  const int row = static_cast<int>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  if (row >= n_e) return;
  const int lane = lane_id();
  const int start = rowptr[row], end = rowptr[row + 1];
  for (int h = 0; h < H; ++h) {
    float sum = 0.f;
    for (int j = start + lane; j < end; j += kWave) sum += ge[static_cast<int64_t>(j) * H + h];
    sum = wave_sum(sum);
    if (lane == 0) gae[static_cast<int64_t>(row) * H + h] = sum;
  }
}

static int check_dims(const char* who, int64_t n_a, int64_t n_b, int64_t nnz, int64_t H, int64_t C) {
  ALLSET_REQUIRE(n_a >= 0 && n_b >= 0 && nnz >= 0, "%s: negative size", who);
  ALLSET_REQUIRE(n_a < INT32_MAX && n_b < INT32_MAX && nnz < INT32_MAX, "%s: size exceeds int32", who);
  ALLSET_REQUIRE(H >= 1 && C >= 1, "%s: heads/channels must be >= 1", who);
  if (H > kMaxHeads || C > kMaxWidth || H * C > kMaxWidth) {
    set_error("%s: heads=%lld x channels=%lld exceeds the built maximum (heads <= %d, heads * channels <= %d)", who,
              static_cast<long long>(H), static_cast<long long>(C), kMaxHeads, kMaxWidth);
    return ALLSET_ERR_UNSUPPORTED;
  }
  return ALLSET_OK;
}

// lanes per head / per slot and packets per lane (rounded up to a built count) for H heads of C channels in VEC-float packets
static inline int geometry(int64_t H, int64_t C, int vec, Geo* g) {
  int hp = 1;
  while (hp < H) hp <<= 1;
  const int per = static_cast<int>((C + vec - 1) / vec);
  int lh = 1;
  while (lh < per && lh * hp < kWave) lh <<= 1;
  *g = Geo{static_cast<int>(H), static_cast<int>(C), lh, hp * lh};
  const int need = (per + lh - 1) / lh;
  int npl = 1;
  while (npl < need) npl <<= 1;
  return npl;
}

#define ALLSET_HATTN_DISPATCH(LAUNCH)                                \
  do {                                                               \
    if (wide_ok) {                                                   \
      switch (npl) {                                                 \
        case 1: LAUNCH(4, 1); break;                                 \
        case 2: LAUNCH(4, 2); break;                                 \
        default: LAUNCH(4, 4); break;                                \
      }                                                              \
    } else {                                                         \
      switch (npl) {                                                 \
        case 1: LAUNCH(1, 1); break;                                 \
        case 2: LAUNCH(1, 2); break;                                 \
        case 4: LAUNCH(1, 4); break;                                 \
        case 8: LAUNCH(1, 8); break;                                 \
        default: LAUNCH(1, 16); break;                               \
      }                                                              \
    }                                                                \
  } while (0)

}  // namespace hattn
}  // namespace allset

using namespace allset;
using namespace allset::hattn;

extern "C" int allset_hattn_supported(void) { return 1; }

extern "C" int allset_hattn_coef(int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm, const int32_t* pos,
                                 const float* av, const float* ae, float slope, float p, uint64_t seed, const uint64_t* seed_base,
                                 float* a_v, float* a_e, float* m, float* l, int64_t n_v, int64_t n_e, int64_t H, void* stream) {
  clear_error();
  ALLSET_REQUIRE(p >= 0.f && p < 1.f, "hattn_coef: dropout p must be in [0,1)");
  int rc = check_dims("hattn_coef", n_v, n_e, nnz, H, 1);
  if (rc != ALLSET_OK) return rc;
  if (n_v == 0) return ALLSET_OK;
  ALLSET_REQUIRE(rowptr && av && m && l, "hattn_coef: null rowptr/av/m/l");
  ALLSET_REQUIRE(nnz == 0 || (col && perm && pos && ae && a_v && a_e), "hattn_coef: null col/perm/pos/ae/a_v/a_e with nnz > 0");
  hattn_coef_kernel<<<row_grid(n_v), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      rowptr, col, perm, pos, av, ae, slope, p, seed, seed_base, drop_threshold(p), drop_inv_keep(p), a_v, a_e, m, l,
      static_cast<int>(n_v), static_cast<int>(H));
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_hattn_hop(int64_t nnz, const int32_t* row_order, const int32_t* rowptr, const int32_t* col, const float* w,
                                const float* r, const float* s, const float* x, int64_t ldx, const float* bias, int act, float p,
                                uint64_t seed, const uint64_t* seed_base, int concat, float* y, int64_t ldy, int64_t n_t, int64_t n_s,
                                int64_t H, int64_t C, void* stream) {
  clear_error();
  ALLSET_REQUIRE(act >= kActNone && act <= kActElu, "hattn_hop: bad act %d", act);
  ALLSET_REQUIRE(p >= 0.f && p < 1.f, "hattn_hop: dropout p must be in [0,1)");
  int rc = check_dims("hattn_hop", n_t, n_s, nnz, H, C);
  if (rc != ALLSET_OK) return rc;
  if (n_t == 0) return ALLSET_OK;
  const int64_t d = H * C, dy = concat ? d : C;
  ALLSET_REQUIRE(rowptr && y, "hattn_hop: null rowptr/y");
  ALLSET_REQUIRE(nnz == 0 || (col && w && x), "hattn_hop: null col/w/x with nnz > 0");
  ALLSET_REQUIRE(ldx >= d && ldy >= dy, "hattn_hop: leading dimension smaller than the row");
  const bool wide_ok = (C % 4 == 0) && (ldx % 4 == 0) && (ldy % 4 == 0) && aligned16(x) && aligned16(y);
  Geo g;
  const int npl = geometry(H, C, wide_ok ? 4 : 1, &g);
  const RowEpi e = row_epi(bias, act, p, seed);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned grid = row_grid(n_t);
#define ALLSET_HATTN_HOP(VEC, NPL)                                                                                               \
  hattn_hop_kernel<VEC, NPL><<<grid, kBlock, 0, st>>>(rowptr, col, w, r, s, x, ldx, y, ldy, static_cast<int>(n_t), g, concat ? 1 : 0, \
                                                      row_order, e, seed_base)
  ALLSET_HATTN_DISPATCH(ALLSET_HATTN_HOP);
#undef ALLSET_HATTN_HOP
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_hattn_bwd_vertex(int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* pos, const float* a_v,
                                       const float* av, const float* ae, const float* m, const float* l, float slope, const float* z,
                                       int64_t ldz, const float* g_u, int64_t ldg, const float* y, int64_t ldy, const float* gy,
                                       int64_t ldgy, const float* D, const float* B, float* gz, int64_t ldgz, float* t, float* gav,
                                       float* ge_e, int64_t n_v, int64_t n_e, int64_t H, int64_t C, void* stream) {
  clear_error();
  int rc = check_dims("hattn_bwd_vertex", n_v, n_e, nnz, H, C);
  if (rc != ALLSET_OK) return rc;
  if (n_v == 0) return ALLSET_OK;
  const int64_t d = H * C;
  ALLSET_REQUIRE(rowptr && av && m && l && z && g_u && D && gz && gav, "hattn_bwd_vertex: null pointer");
  ALLSET_REQUIRE(nnz == 0 || (col && pos && a_v && ae && y && gy && B && t && ge_e), "hattn_bwd_vertex: null pointer with nnz > 0");
  ALLSET_REQUIRE(ldz >= d && ldg >= d && ldy >= d && ldgy >= d && ldgz >= d, "hattn_bwd_vertex: leading dimension smaller than H*C");
  const bool wide_ok = (C % 4 == 0) && (ldz % 4 == 0) && (ldg % 4 == 0) && (ldy % 4 == 0) && (ldgy % 4 == 0) && (ldgz % 4 == 0) &&
                       aligned16(z) && aligned16(g_u) && aligned16(y) && aligned16(gy) && aligned16(gz);
  Geo g;
  const int npl = geometry(H, C, wide_ok ? 4 : 1, &g);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned grid = row_grid(n_v);
#define ALLSET_HATTN_BWD(VEC, NPL)                                                                                                  \
  hattn_bwd_vertex_kernel<VEC, NPL><<<grid, kBlock, 0, st>>>(rowptr, col, pos, a_v, av, ae, m, l, slope, z, ldz, g_u, ldg, y, ldy, gy, \
                                                             ldgy, D, B, gz, ldgz, t, gav, ge_e, static_cast<int>(n_v), g)
  ALLSET_HATTN_DISPATCH(ALLSET_HATTN_BWD);
#undef ALLSET_HATTN_BWD
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_hattn_bwd_edge(int64_t nnz, const int32_t* rowptr, const float* ge_e, float* gae, int64_t n_e, int64_t H,
                                     void* stream) {
  clear_error();
  int rc = check_dims("hattn_bwd_edge", n_e, 0, nnz, H, 1);
  if (rc != ALLSET_OK) return rc;
  if (n_e == 0) return ALLSET_OK;
  ALLSET_REQUIRE(rowptr && gae, "hattn_bwd_edge: null rowptr/gae");
  ALLSET_REQUIRE(nnz == 0 || ge_e, "hattn_bwd_edge: null ge_e with nnz > 0");
  hattn_bwd_edge_kernel<<<row_grid(n_e), kBlock, 0, static_cast<hipStream_t>(stream)>>>(rowptr, ge_e, gae, static_cast<int>(n_e),
                                                                                         static_cast<int>(H));
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}
