// HAN baseline (reference DGL_HAN/model.py: one DGL 0.7.1 GATConv per metapath graph, then SemanticAttention) for gfx950.
//
// ---- the attention hop -------------------------------------------------------------------------------------------------------
// Over a target-major CSR of a multigraph (slot j of the CSR is the edge's identity; duplicates are separate slots), per head h:
//   e_j        = leaky_relu(el[s_j,h] + er[t,h], slope)
//   p_j        = exp(e_j - m) / l,  m = max_j e_j,  l = sum_j exp(e_j - m)                    (no epsilon; a row without edges: out = 0)
//   a_j        = p_j * k_j,  k_j = keep_j / (1 - p_att),  keep_j = hash(seed, j * H + h)     (the library's counter-hash dropout)
//   out[t,h,:] = sum_j a_j x[s_j,h,:]
//   y[t,h,:]   = elu(out[t,h,:] + bias[h,:])                                                   (alpha = 1)
// y is written through a row pitch, so the caller points it at column block m of the stacked [N, M*H*C] buffer.
//
// Backward, with g = gy * elu'(.) = gy * (y > 0 ? 1 : y + 1) the gradient at out and d_j = <x[s_j,h,:], g[t,h,:]>:
//   dL/da_j = d_j,  dL/dp_j = k_j d_j,  and through the softmax
//   dL/de_j = p_j (k_j d_j - sum_i p_i k_i d_i) = a_j d_j - p_j delta,   delta[t,h] = sum_i a_i d_i = <out[t,h,:], g[t,h,:]>
// so the delta identity of gat.hip holds with the mask INSIDE the aggregate.  With lrelu' = slope + (1 - slope) [e > 0]:
//   ger[t,h] = sum_j lrelu'_j (a_j d_j - p_j delta)
//            = slope (delta - delta * sum_j p_j) + (1 - slope) (<outpos[t,h,:], g[t,h,:]> - delta * ppos[t,h])
//            = (1 - slope) (<outpos, g> - delta * ppos)          outpos = sum_{e_j > 0} a_j x_j (MASKED),  ppos = sum_{e_j > 0} p_j (NOT)
//   gx[s,h,:] = sum_j a_j g[t_j,h,:]                                                            (j over the edges leaving s)
//   gel[s,h]  = slope (<x_s, gx_s> - sum_j p_j delta_j) + (1 - slope) (<x_s, sum_{e_j > 0} a_j g_j> - sum_{e_j > 0} p_j delta_j)
//   forward  : one wavefront per target row (gat.hip's skeleton: LPR lanes x VEC floats per row, NS = 64 / LPR edges per gather,
//              an online softmax per lane, slots merged at the end), elu epilogue in the same launch; outpos / ppos on demand.
//   stats    : one pass over the rows, no edges: g (dense, also the bias gradient's operand), {m + log l, delta} and ger.  out is
//              rebuilt from y wherever g != 0: out = (y > 0 ? y : log1p(y)) - bias (the error of log1p near y = -1 is
//              ulp / (1 + y), and g carries the factor 1 + y).
//   source   : one gather pass over the source-major CSR; slotT[j] is the target-major slot of entry j, from which the same
//              keep_j is regenerated.  Dot products once per ROW on the accumulated vectors.
// Algorithmic bytes: forward nnz (4d + 4H + 4) + n (4d [+ 4d outpos] + 12H); stats n (5 * 4d + 16H); source nnz (4d + 12H + 8) + n 8d.
//
// ---- semantic attention ------------------------------------------------------------------------------------------------------
//   s[n,m] = q . tanh(W1 z[n,m,:] + b1)     w_m = mean_n s[n,m]     beta = softmax_m w     out[n,:] = sum_m beta_m z[n,m,:]
// The projection is [N*M, D] x [D, 128] with D <= 128: LDS-tiled fp32 FMA (32 rows per tile, W1 resident in LDS for the
// block's whole life, a 2 x 8 register tile per thread).  The split-precision MFMA helpers of this tree are built around
// pre-split weight planes and 128-row tiles of K >= 64; here K = D (64 by default), and the tanh, the reductions and the two further
// products of the backward want the hidden in registers in exactly this layout.  Measured share of the training step (DESIGN
// section 15): sem_score 2 % (Cora-shaped) / 6 % (10^6 edges per graph), sem_bwd 4 % / 14 %.
//   forward : sem_score (persistent blocks; hidden in registers; per-block, per-metapath partial sums of s in a fixed order),
//             sem_stage2 (one block: w, beta), sem_combine.
//   backward: gbeta_m = sum_n <gout[n], z[n,m]> (sem_dot, same partial scheme), stage2: gs_m = beta_m (gbeta_m - sum_k beta_k gbeta_k) / N
//             (s enters only through the mean, so ds is one number per metapath), then sem_bwd recomputes the hidden and, per tile,
//             gpre = gs_m q (1 - h^2) -> LDS; gz = beta_m gout[n] + gpre W1; register partials of gW1 = gpre^T z, gb1 = sum gpre,
//             gq = sum gs_m h; per-block partials, reduced in block order by sem_reduce.  No atomics anywhere.
// Algorithmic bytes: forward 2 * 4NMD + 4ND; backward 3 * 4NMD + 2 * 4ND + blocks * 4 (128 D + 256).
#include <float.h>

#include "common.h"

namespace allset {
namespace han {

constexpr int kUnroll = 8;
constexpr int kMaxHeads = 64;
constexpr int kMaxWidth = 512;

__device__ __forceinline__ float elu1(float v) { return v > 0.f ? v : expm1f(v); }

template <int VEC, int LPR, bool POS>
__global__ __launch_bounds__(kBlock) void hop_fwd_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ el, const float* __restrict__ er,
    const float* __restrict__ x, int64_t ldx, float slope, const float* __restrict__ bias, uint64_t seed,
    const uint64_t* __restrict__ seed_base, uint32_t thr, float inv_keep, int drop, float* __restrict__ y, int64_t ldy,
    float* __restrict__ outpos, int64_t ldp, float* __restrict__ ppos, float* __restrict__ lse, int n, int H, int C) {
  constexpr int NS = kWave / LPR;
  const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int row = static_cast<int>(blk) * kWavesPerBlock + (threadIdx.x >> 6);
  if (row >= n) return;  // whole wave exits together
  seed = resolve_seed(seed_base, seed);
  const int lane = lane_id();
  const int slot = lane / LPR, li = lane % LPR;
  const int start = rowptr[row], end = rowptr[row + 1];
  const int d = H * C;

  for (int cb = 0; cb < d; cb += LPR * VEC) {
    const int c0 = cb + li * VEC;
    const bool active = c0 < d;
    const int h = active ? c0 / C : 0;
    const float er_t = active ? er[static_cast<int64_t>(row) * H + h] : 0.f;
    float m = -FLT_MAX, l = 0.f, lp = 0.f;
    float acc[VEC], accp[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) { acc[k] = 0.f; accp[k] = 0.f; }

    for (int base = start; base < end; base += kWave) {
      const int cnt = min(kWave, end - base);
      const int my_col = (lane < cnt) ? col[base + lane] : 0;
      for (int j = 0; j < cnt; j += NS * kUnroll) {
        Raw<float, VEC> raw[kUnroll];
        float a[kUnroll];
        bool ok[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const int jj = j + u * NS + slot;
          ok[u] = (jj < cnt) && active;
          const int src = __shfl(my_col, jj & (kWave - 1));
          if (ok[u]) {
            a[u] = el[static_cast<int64_t>(src) * H + h];
            raw[u] = load_raw<float, VEC>(x + static_cast<int64_t>(src) * ldx + c0);
          }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          if (ok[u]) {
            const FVec<VEC> vu = unpack<float, VEC>(raw[u]);
            const float e = a[u] + er_t;
            const float av = leaky_relu(e, slope);
            const float m_new = fmaxf(m, av);
            const float sc = __expf(m - m_new);       // 0 on the first edge (m = -FLT_MAX)
            const float pe = __expf(av - m_new);
            const int64_t eid = static_cast<int64_t>(base + j + u * NS + slot) * H + h;
            const float pk = drop ? pe * keep_scale(seed, eid, thr, inv_keep) : pe;
            l = fmaf(l, sc, pe);
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = fmaf(acc[k], sc, pk * vu.v[k]);
            if constexpr (POS) {
              const bool pos = e > 0.f;
              lp = fmaf(lp, sc, pos ? pe : 0.f);
              const float ppk = pos ? pk : 0.f;
#pragma unroll
              for (int k = 0; k < VEC; ++k) accp[k] = fmaf(accp[k], sc, ppk * vu.v[k]);
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
      // a row without edges (han_hetero's graphs allow one): acc = 0, inv = 0 -> y = elu(bias); lse = FLT_MAX, outpos = ppos = 0, so
      // the stats pass gives ger = 0 and no edge ever reads its stats (tests/test_gpu_han_hetero.py)
      const float inv = l > 0.f ? 1.f / l : 0.f;
      FVec<VEC> r;
#pragma unroll
      for (int k = 0; k < VEC; ++k) r.v[k] = elu1(acc[k] * inv + (bias ? bias[c0 + k] : 0.f));
      store_vec<float, VEC>(y + static_cast<int64_t>(row) * ldy + c0, r);
      if constexpr (POS) {
        FVec<VEC> rp;
#pragma unroll
        for (int k = 0; k < VEC; ++k) rp.v[k] = accp[k] * inv;
        store_vec<float, VEC>(outpos + static_cast<int64_t>(row) * ldp + c0, rp);
      }
      if (c0 % C == 0) {
        const int64_t th = static_cast<int64_t>(row) * H + h;
        lse[th] = l > 0.f ? m + logf(l) : FLT_MAX;
        if constexpr (POS) ppos[th] = lp * inv;
      }
    }
  }
}

// One wavefront per target row; LH = 64 / Hp lanes per head (Hp = H rounded up to a power of two), each striding its head's C
// channels.  Writes g = gy * elu'(y), stats[t,h] = {m + log l, delta} and ger[t,h].
__global__ __launch_bounds__(kBlock) void hop_bwd_stats_kernel(
    const float* __restrict__ y, int64_t ldy, const float* __restrict__ bias, const float* __restrict__ gy, int64_t ldgy,
    const float* __restrict__ outpos, int64_t ldp, const float* __restrict__ ppos, const float* __restrict__ lse, float slope,
    float* __restrict__ g, int64_t ldg, float* __restrict__ stats, float* __restrict__ ger, int n, int H, int C, int LH) {
  const int row = static_cast<int>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  if (row >= n) return;
  const int lane = lane_id();
  const int h = lane / LH, sub = lane % LH;
  float delta = 0.f, dpos = 0.f;
  if (h < H) {
    for (int c = sub; c < C; c += LH) {
      const int cc = h * C + c;
      const float yv = y[static_cast<int64_t>(row) * ldy + cc];
      const float gv = gy[static_cast<int64_t>(row) * ldgy + cc] * (yv > 0.f ? 1.f : yv + 1.f);
      g[static_cast<int64_t>(row) * ldg + cc] = gv;
      if (gv != 0.f) {
        const float a = (yv > 0.f ? yv : log1pf(yv)) - (bias ? bias[cc] : 0.f);
        delta = fmaf(a, gv, delta);
        dpos = fmaf(outpos[static_cast<int64_t>(row) * ldp + cc], gv, dpos);
      }
    }
  }
  for (int off = 1; off < LH; off <<= 1) {
    delta += __shfl_xor(delta, off);
    dpos += __shfl_xor(dpos, off);
  }
  if (h < H && sub == 0) {
    const int64_t th = static_cast<int64_t>(row) * H + h;
    float2 s;
    s.x = lse[th];
    s.y = delta;
    *reinterpret_cast<float2*>(stats + th * 2) = s;
    ger[th] = (1.f - slope) * (dpos - delta * ppos[th]);
  }
}

template <int VEC, int LPR>
__global__ __launch_bounds__(kBlock) void hop_bwd_src_kernel(
    const int32_t* __restrict__ rowptrT, const int32_t* __restrict__ colT, const int32_t* __restrict__ slotT,
    const float* __restrict__ el, const float* __restrict__ er, const float* __restrict__ x, int64_t ldx, const float* __restrict__ g,
    int64_t ldg, const float* __restrict__ stats, float slope, uint64_t seed, const uint64_t* __restrict__ seed_base, uint32_t thr,
    float inv_keep, int drop, float* __restrict__ gx, int64_t ldgx, float* __restrict__ gel, int n, int H, int C) {
  constexpr int NS = kWave / LPR;
  __shared__ float red[kWavesPerBlock][kMaxHeads];
  const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int wave = threadIdx.x >> 6;
  const int row = static_cast<int>(blk) * kWavesPerBlock + wave;
  if (row >= n) return;
  seed = resolve_seed(seed_base, seed);
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
    float el_s = 0.f;
    if (active) {
      vown = load_vec<float, VEC>(x + static_cast<int64_t>(row) * ldx + c0);
      el_s = el[static_cast<int64_t>(row) * H + h];
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) vown.v[k] = 0.f;
    }
    float gv[VEC], gvp[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) { gv[k] = 0.f; gvp[k] = 0.f; }
    float D = 0.f, Dp = 0.f;

    for (int base = start; base < end; base += kWave) {
      const int cnt = min(kWave, end - base);
      const int my_col = (lane < cnt) ? colT[base + lane] : 0;
      const int my_slot = (lane < cnt) ? slotT[base + lane] : 0;
      for (int j = 0; j < cnt; j += NS * kUnroll) {
        Raw<float, VEC> gr[kUnroll];
        float2 st[kUnroll];
        float ert[kUnroll];
        int es[kUnroll];
        bool ok[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const int jj = j + u * NS + slot;
          ok[u] = (jj < cnt) && active;
          const int t = __shfl(my_col, jj & (kWave - 1));
          es[u] = __shfl(my_slot, jj & (kWave - 1));
          if (ok[u]) {
            gr[u] = load_raw<float, VEC>(g + static_cast<int64_t>(t) * ldg + c0);
            st[u] = *reinterpret_cast<const float2*>(stats + (static_cast<int64_t>(t) * H + h) * 2);
            ert[u] = er[static_cast<int64_t>(t) * H + h];
          }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          if (ok[u]) {
            const float e = el_s + ert[u];
            const float p = __expf(leaky_relu(e, slope) - st[u].x);
            const float a = drop ? p * keep_scale(seed, static_cast<int64_t>(es[u]) * H + h, thr, inv_keep) : p;
            const bool pos = e > 0.f;
            const float ap = pos ? a : 0.f;
            const FVec<VEC> gu = unpack<float, VEC>(gr[u]);
#pragma unroll
            for (int k = 0; k < VEC; ++k) { gv[k] = fmaf(a, gu.v[k], gv[k]); gvp[k] = fmaf(ap, gu.v[k], gvp[k]); }
            D = fmaf(p, st[u].y, D);
            Dp = fmaf(pos ? p : 0.f, st[u].y, Dp);
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
    // sum_j w_j <x_s, g_j> = <x_s, sum_j w_j g_j> for w = a and w = a [e > 0]: no per-edge dot product
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
    if (slot == 0 && active && (q == 0 || li == 0)) red[wave][h] += part - (q == 0 ? slope * D + (1.f - slope) * Dp : 0.f);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
  for (int h = lane; h < H; h += kWave) gel[static_cast<int64_t>(row) * H + h] = red[wave][h];
}

// ---- semantic attention --------------------------------------------------------------------------------------------------------
constexpr int kHid = 128;                 // SemanticAttention's hidden width (the reference's default, the only one built)
constexpr int kRows = 32;                 // rows of z (one row = one (node, metapath) pair) per tile
constexpr int kSemMaxD = 128;
constexpr int kSemMaxM = 32;
constexpr int kSemMaxBlocks = 256;        // persistent blocks: the partial buffers' first dimension
constexpr int kGp = kHid + 1;             // LDS pitch of the gpre tile

static inline int sem_blocks(int64_t rows) {
  const int64_t tiles = (rows + kRows - 1) / kRows;
  return static_cast<int>(tiles < kSemMaxBlocks ? (tiles > 0 ? tiles : 1) : kSemMaxBlocks);
}

template <int DMAX>
__device__ __forceinline__ void sem_load_w(float* Ws, const float* __restrict__ W1, int D) {
  for (int i = threadIdx.x; i < kHid * D; i += kBlock) Ws[(i / D) * (DMAX + 1) + (i % D)] = W1[i];
}

template <int DMAX>
__device__ __forceinline__ void sem_load_z(float* zt, const float* __restrict__ z, int64_t r0, int64_t rows, int D) {
  for (int i = threadIdx.x; i < kRows * D; i += kBlock) {
    const int r = i / D, k = i % D;
    zt[r * (DMAX + 1) + k] = (r0 + r < rows) ? z[(r0 + r) * D + k] : 0.f;
  }
}

// thread (tr = tid / 16, tc = tid % 16): rows 2 tr, 2 tr + 1 of the tile, hidden units tc + 16 i
template <int DMAX>
__device__ __forceinline__ void sem_hidden(const float* Ws, const float* zt, const float* __restrict__ b1, int D, int tr, int tc,
                                           float (&h)[2][8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) { h[0][i] = 0.f; h[1][i] = 0.f; }
  const float* z0 = zt + (2 * tr) * (DMAX + 1);
  const float* z1 = z0 + (DMAX + 1);
  for (int k = 0; k < D; ++k) {
    const float a0 = z0[k], a1 = z1[k];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float w = Ws[(tc + 16 * i) * (DMAX + 1) + k];
      h[0][i] = fmaf(a0, w, h[0][i]);
      h[1][i] = fmaf(a1, w, h[1][i]);
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float b = b1[tc + 16 * i];
    h[0][i] = tanhf(h[0][i] + b);
    h[1][i] = tanhf(h[1][i] + b);
  }
}

// per-row scalars of one tile (in LDS) -> this thread's metapath (thread m < M), rows in order
__device__ __forceinline__ float sem_by_metapath(const float* srow, int64_t r0, int64_t rows, int M, float sum) {
  const int m = threadIdx.x;
  if (m < M) {
    for (int r = 0; r < kRows; ++r) {
      const int64_t row = r0 + r;
      if (row < rows && row % M == m) sum += srow[r];
    }
  }
  return sum;
}

template <int DMAX>
__global__ __launch_bounds__(kBlock) void sem_score_kernel(const float* __restrict__ z, const float* __restrict__ W1,
                                                           const float* __restrict__ b1, const float* __restrict__ q,
                                                           float* __restrict__ part, int64_t rows, int M, int D) {
  __shared__ float Ws[kHid * (DMAX + 1)];
  __shared__ float zt[kRows * (DMAX + 1)];
  __shared__ float srow[kRows];
  const int tr = threadIdx.x >> 4, tc = threadIdx.x & 15;
  sem_load_w<DMAX>(Ws, W1, D);
  float qv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) qv[i] = q[tc + 16 * i];
  const int64_t tiles = (rows + kRows - 1) / kRows;
  float msum = 0.f;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * kRows;
    __syncthreads();
    sem_load_z<DMAX>(zt, z, r0, rows, D);
    __syncthreads();
    float h[2][8];
    sem_hidden<DMAX>(Ws, zt, b1, D, tr, tc, h);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) s = fmaf(qv[i], h[a][i], s);
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) s += __shfl_xor(s, off);
      if (tc == 0) srow[2 * tr + a] = s;
    }
    __syncthreads();
    msum = sem_by_metapath(srow, r0, rows, M, msum);
  }
  if (threadIdx.x < M) part[static_cast<int64_t>(blockIdx.x) * M + threadIdx.x] = msum;
}

// per-block, per-metapath partial sums of <gout[n,:], z[n,m,:]>
__global__ __launch_bounds__(kBlock) void sem_dot_kernel(const float* __restrict__ z, const float* __restrict__ gout,
                                                         float* __restrict__ part, int64_t rows, int M, int D) {
  __shared__ float srow[kRows];
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const int64_t tiles = (rows + kRows - 1) / kRows;
  float msum = 0.f;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * kRows;
    __syncthreads();
    for (int r = wave; r < kRows; r += kWavesPerBlock) {
      const int64_t row = r0 + r;
      float v = 0.f;
      if (row < rows)
        for (int c = lane; c < D; c += kWave) v = fmaf(gout[(row / M) * D + c], z[row * D + c], v);
#pragma unroll
      for (int off = 1; off < kWave; off <<= 1) v += __shfl_xor(v, off);
      if (lane == 0) srow[r] = v;
    }
    __syncthreads();
    msum = sem_by_metapath(srow, r0, rows, M, msum);
  }
  if (threadIdx.x < M) part[static_cast<int64_t>(blockIdx.x) * M + threadIdx.x] = msum;
}

// One block.  mode 0: wbeta[0..M) = w = column sums of part / N, wbeta[M..2M) = softmax(w).  mode 1: gbeta = column sums,
// gsm[m] = beta_m (gbeta_m - sum_k beta_k gbeta_k) / N.
__global__ __launch_bounds__(kBlock) void sem_stage2_kernel(const float* __restrict__ part, int nb, int M, float inv_n, int mode,
                                                            float* __restrict__ wbeta, float* __restrict__ gsm) {
  __shared__ float red[kBlock];
  __shared__ float tot[kSemMaxM];
  for (int m = 0; m < M; ++m) {
    float v = 0.f;
    for (int b = threadIdx.x; b < nb; b += kBlock) v += part[static_cast<int64_t>(b) * M + m];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int off = kBlock / 2; off > 0; off >>= 1) {
      if (static_cast<int>(threadIdx.x) < off) red[threadIdx.x] += red[threadIdx.x + off];
      __syncthreads();
    }
    if (threadIdx.x == 0) tot[m] = red[0];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  if (mode == 0) {
    float mx = -FLT_MAX, den = 0.f;
    for (int m = 0; m < M; ++m) { tot[m] *= inv_n; mx = fmaxf(mx, tot[m]); }
    for (int m = 0; m < M; ++m) den += expf(tot[m] - mx);
    for (int m = 0; m < M; ++m) { wbeta[m] = tot[m]; wbeta[M + m] = expf(tot[m] - mx) / den; }
  } else {
    float dot = 0.f;
    for (int m = 0; m < M; ++m) dot = fmaf(wbeta[M + m], tot[m], dot);
    for (int m = 0; m < M; ++m) gsm[m] = wbeta[M + m] * (tot[m] - dot) * inv_n;
  }
}

__global__ __launch_bounds__(kBlock) void sem_combine_kernel(const float* __restrict__ z, const float* __restrict__ wbeta,
                                                             float* __restrict__ out, int64_t total, int M, int D) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int64_t nrow = idx / D;
  const int c = static_cast<int>(idx % D);
  float v = 0.f;
  for (int m = 0; m < M; ++m) v = fmaf(wbeta[M + m], z[(nrow * M + m) * D + c], v);
  out[idx] = v;
}

template <int DMAX>
__global__ __launch_bounds__(kBlock) void sem_bwd_kernel(const float* __restrict__ z, const float* __restrict__ W1,
                                                         const float* __restrict__ b1, const float* __restrict__ q,
                                                         const float* __restrict__ wbeta, const float* __restrict__ gsm,
                                                         const float* __restrict__ gout, float* __restrict__ gz,
                                                         float* __restrict__ ppart, int64_t rows, int M, int D) {
  constexpr int NI = DMAX / 16;
  __shared__ float Ws[kHid * (DMAX + 1)];
  __shared__ float zt[kRows * (DMAX + 1)];
  __shared__ float gp[kRows * kGp];
  const int tr = threadIdx.x >> 4, tc = threadIdx.x & 15;
  sem_load_w<DMAX>(Ws, W1, D);
  float qv[8], accq[8], accb[8], accW[8][NI];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    qv[i] = q[tc + 16 * i];
    accq[i] = 0.f;
    accb[i] = 0.f;
#pragma unroll
    for (int b = 0; b < NI; ++b) accW[i][b] = 0.f;
  }
  const int64_t tiles = (rows + kRows - 1) / kRows;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * kRows;
    __syncthreads();
    sem_load_z<DMAX>(zt, z, r0, rows, D);
    __syncthreads();
    float h[2][8];
    sem_hidden<DMAX>(Ws, zt, b1, D, tr, tc, h);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int64_t row = r0 + 2 * tr + a;
      const float gs = row < rows ? gsm[row % M] : 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float hv = h[a][i];
        const float gpv = gs * qv[i] * (1.f - hv * hv);
        accq[i] = fmaf(gs, hv, accq[i]);
        accb[i] += gpv;
        gp[(2 * tr + a) * kGp + tc + 16 * i] = gpv;
      }
    }
    __syncthreads();
    // gz[row, c] = beta_m gout[n, c] + sum_j gpre[row, j] W1[j, c]: rows 2 tr, 2 tr + 1, columns tc + 16 i
    float acc[2][NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) { acc[0][i] = 0.f; acc[1][i] = 0.f; }
    const float* g0 = gp + (2 * tr) * kGp;
    const float* g1 = g0 + kGp;
    for (int j = 0; j < kHid; ++j) {
      const float a0 = g0[j], a1 = g1[j];
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int c = tc + 16 * i;
        const float w = c < D ? Ws[j * (DMAX + 1) + c] : 0.f;
        acc[0][i] = fmaf(a0, w, acc[0][i]);
        acc[1][i] = fmaf(a1, w, acc[1][i]);
      }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int64_t row = r0 + 2 * tr + a;
      if (row < rows) {
        const float beta = wbeta[M + row % M];
        const int64_t nrow = row / M;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int c = tc + 16 * i;
          if (c < D) gz[row * D + c] = fmaf(beta, gout[nrow * D + c], acc[a][i]);
        }
      }
    }
    // gW1[j, k] += sum_r gpre[r, j] z[r, k]: j = 8 tr + a, k = tc + 16 b (rows past the end carry gpre = 0 and z = 0)
    for (int r = 0; r < kRows; ++r) {
      float zk[NI];
#pragma unroll
      for (int b = 0; b < NI; ++b) {
        const int k = tc + 16 * b;
        zk[b] = k < D ? zt[r * (DMAX + 1) + k] : 0.f;
      }
#pragma unroll
      for (int a = 0; a < 8; ++a) {
        const float gj = gp[r * kGp + 8 * tr + a];
#pragma unroll
        for (int b = 0; b < NI; ++b) accW[a][b] = fmaf(gj, zk[b], accW[a][b]);
      }
    }
  }
  // this block's partials: [128 * D] gW1, [128] gb1, [128] gq
  float* pp = ppart + static_cast<int64_t>(blockIdx.x) * (kHid * D + 2 * kHid);
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int b = 0; b < NI; ++b) {
      const int k = tc + 16 * b;
      if (k < D) pp[(8 * tr + a) * D + k] = accW[a][b];
    }
  for (int pass = 0; pass < 2; ++pass) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) gp[tr * kHid + tc + 16 * i] = pass == 0 ? accb[i] : accq[i];
    __syncthreads();
    if (threadIdx.x < kHid) {
      float v = 0.f;
      for (int t = 0; t < 16; ++t) v += gp[t * kHid + threadIdx.x];
      pp[kHid * D + pass * kHid + threadIdx.x] = v;
    }
  }
}

__global__ __launch_bounds__(kBlock) void sem_reduce_kernel(const float* __restrict__ ppart, int nb, int64_t P, float* __restrict__ out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= P) return;
  float v = 0.f;
  for (int b = 0; b < nb; ++b) v += ppart[static_cast<int64_t>(b) * P + i];
  out[i] = v;
}

static int check_dims(const char* who, int64_t n, int64_t nnz, int64_t H, int64_t C) {
  ALLSET_REQUIRE(n >= 0 && nnz >= 0, "%s: negative size", who);
  ALLSET_REQUIRE(n < INT32_MAX && nnz < INT32_MAX, "%s: size exceeds int32", who);
  ALLSET_REQUIRE(H >= 1 && C >= 1, "%s: heads/channels must be >= 1", who);
  if (H > kMaxHeads || C > kMaxWidth || H * C > kMaxWidth) {
    set_error("%s: heads=%lld x channels=%lld exceeds the built maximum (heads <= %d, heads * channels <= %d)", who,
              static_cast<long long>(H), static_cast<long long>(C), kMaxHeads, kMaxWidth);
    return ALLSET_ERR_UNSUPPORTED;
  }
  return ALLSET_OK;
}

static int check_sem(const char* who, int64_t N, int64_t M, int64_t D, int64_t hidden) {
  ALLSET_REQUIRE(N >= 1 && M >= 1 && D >= 1, "%s: sizes must be >= 1", who);
  ALLSET_REQUIRE(N * M < INT32_MAX, "%s: size exceeds int32", who);
  if (hidden != kHid || D > kSemMaxD || M > kSemMaxM) {
    set_error("%s: hidden=%lld, width=%lld, metapaths=%lld: built for hidden == %d, width <= %d, metapaths <= %d", who,
              static_cast<long long>(hidden), static_cast<long long>(D), static_cast<long long>(M), kHid, kSemMaxD, kSemMaxM);
    return ALLSET_ERR_UNSUPPORTED;
  }
  return ALLSET_OK;
}

#define ALLSET_HAN_DISPATCH(LAUNCH)                        \
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

}  // namespace han
}  // namespace allset

using namespace allset;
using namespace allset::han;

extern "C" int allset_han_supported(void) { return 1; }

extern "C" int allset_han_hop_fwd(int64_t nnz, const int32_t* rowptr, const int32_t* col, const float* el, const float* er,
                                  const float* x, int64_t ldx, float slope, const float* bias, float p_att, uint64_t seed,
                                  const uint64_t* seed_base, float* y, int64_t ldy, float* outpos, int64_t ldpos, float* ppos,
                                  float* lse, int64_t n, int64_t H, int64_t C, void* stream) {
  clear_error();
  ALLSET_REQUIRE(p_att >= 0.f && p_att < 1.f, "han_hop_fwd: dropout p must be in [0,1)");
  int rc = check_dims("han_hop_fwd", n, nnz, H, C);
  if (rc != ALLSET_OK) return rc;
  if (n == 0) return ALLSET_OK;
  const int64_t d = H * C;
  ALLSET_REQUIRE(rowptr && y && lse && er, "han_hop_fwd: null rowptr/y/lse/er");
  ALLSET_REQUIRE(nnz == 0 || (col && x && el), "han_hop_fwd: null col/x/el with nnz > 0");
  ALLSET_REQUIRE((outpos == nullptr) == (ppos == nullptr), "han_hop_fwd: outpos and ppos go together");
  ALLSET_REQUIRE(ldx >= d && ldy >= d && (!outpos || ldpos >= d), "han_hop_fwd: leading dimension smaller than the row");
  const bool wide_ok = (C % 4 == 0) && (ldx % 4 == 0) && aligned16(x) && (ldy % 4 == 0) && aligned16(y) &&
                       (!outpos || (ldpos % 4 == 0 && aligned16(outpos)));
  const uint32_t thr = drop_threshold(p_att);
  const float inv_keep = drop_inv_keep(p_att);
  const int drop = p_att > 0.f ? 1 : 0;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned grid = row_grid(n);
#define ALLSET_HAN_FWD(VEC, LPR)                                                                                                  \
  do {                                                                                                                            \
    if (outpos) hop_fwd_kernel<VEC, LPR, true><<<grid, kBlock, 0, st>>>(rowptr, col, el, er, x, ldx, slope, bias, seed, seed_base, thr, \
        inv_keep, drop, y, ldy, outpos, ldpos, ppos, lse, static_cast<int>(n), static_cast<int>(H), static_cast<int>(C));         \
    else hop_fwd_kernel<VEC, LPR, false><<<grid, kBlock, 0, st>>>(rowptr, col, el, er, x, ldx, slope, bias, seed, seed_base, thr,  \
        inv_keep, drop, y, ldy, outpos, ldpos, ppos, lse, static_cast<int>(n), static_cast<int>(H), static_cast<int>(C));         \
  } while (0)
  ALLSET_HAN_DISPATCH(ALLSET_HAN_FWD);
#undef ALLSET_HAN_FWD
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_han_hop_bwd_stats(const float* y, int64_t ldy, const float* bias, const float* gy, int64_t ldgy,
                                        const float* outpos, int64_t ldpos, const float* ppos, const float* lse, float slope,
                                        float* g, int64_t ldg, float* stats, float* ger, int64_t n, int64_t H, int64_t C,
                                        void* stream) {
  clear_error();
  int rc = check_dims("han_hop_bwd_stats", n, 0, H, C);
  if (rc != ALLSET_OK) return rc;
  if (n == 0) return ALLSET_OK;
  const int64_t d = H * C;
  ALLSET_REQUIRE(y && gy && outpos && ppos && lse && g && stats && ger, "han_hop_bwd_stats: null pointer");
  ALLSET_REQUIRE(ldy >= d && ldgy >= d && ldpos >= d && ldg >= d, "han_hop_bwd_stats: leading dimension smaller than H*C");
  ALLSET_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 7u) == 0, "han_hop_bwd_stats: stats must be 8-byte aligned");
  int hp = 1;
  while (hp < H) hp <<= 1;
  hop_bwd_stats_kernel<<<row_grid(n), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      y, ldy, bias, gy, ldgy, outpos, ldpos, ppos, lse, slope, g, ldg, stats, ger, static_cast<int>(n), static_cast<int>(H),
      static_cast<int>(C), kWave / hp);
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_han_hop_bwd_src(int64_t nnz, const int32_t* rowptrT, const int32_t* colT, const int32_t* slotT, const float* el,
                                      const float* er, const float* x, int64_t ldx, const float* g, int64_t ldg, const float* stats,
                                      float slope, float p_att, uint64_t seed, const uint64_t* seed_base, float* gx, int64_t ldgx,
                                      float* gel, int64_t n, int64_t H, int64_t C, void* stream) {
  clear_error();
  ALLSET_REQUIRE(p_att >= 0.f && p_att < 1.f, "han_hop_bwd_src: dropout p must be in [0,1)");
  int rc = check_dims("han_hop_bwd_src", n, nnz, H, C);
  if (rc != ALLSET_OK) return rc;
  if (n == 0) return ALLSET_OK;
  const int64_t d = H * C;
  ALLSET_REQUIRE(rowptrT && el && x && gx && gel, "han_hop_bwd_src: null pointer");
  ALLSET_REQUIRE(nnz == 0 || (colT && slotT && er && g && stats), "han_hop_bwd_src: null colT/slotT/er/g/stats with nnz > 0");
  ALLSET_REQUIRE(ldx >= d && ldg >= d && ldgx >= d, "han_hop_bwd_src: leading dimension smaller than H*C");
  ALLSET_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 7u) == 0, "han_hop_bwd_src: stats must be 8-byte aligned");
  const bool wide_ok = (C % 4 == 0) && (ldx % 4 == 0) && (ldg % 4 == 0) && (ldgx % 4 == 0) && aligned16(x) && aligned16(g) && aligned16(gx);
  const uint32_t thr = drop_threshold(p_att);
  const float inv_keep = drop_inv_keep(p_att);
  const int drop = p_att > 0.f ? 1 : 0;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned grid = row_grid(n);
#define ALLSET_HAN_BWD(VEC, LPR)                                                                                                \
  hop_bwd_src_kernel<VEC, LPR><<<grid, kBlock, 0, st>>>(rowptrT, colT, slotT, el, er, x, ldx, g, ldg, stats, slope, seed, seed_base, \
                                                        thr, inv_keep, drop, gx, ldgx, gel, static_cast<int>(n), static_cast<int>(H), \
                                                        static_cast<int>(C))
  ALLSET_HAN_DISPATCH(ALLSET_HAN_BWD);
#undef ALLSET_HAN_BWD
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_han_sem_blocks(int64_t N, int64_t M, int64_t* blocks) {
  clear_error();
  ALLSET_REQUIRE(blocks != nullptr, "han_sem_blocks: null pointer");
  ALLSET_REQUIRE(N >= 0 && M >= 0, "han_sem_blocks: negative size");
  *blocks = sem_blocks(N * M);
  return ALLSET_OK;
}

extern "C" int allset_han_sem_fwd(const float* z, const float* W1, const float* b1, const float* q, float* part, float* wbeta,
                                  float* out, int64_t N, int64_t M, int64_t D, int64_t hidden, void* stream) {
  clear_error();
  int rc = check_sem("han_sem_fwd", N, M, D, hidden);
  if (rc != ALLSET_OK) return rc;
  ALLSET_REQUIRE(z && W1 && b1 && q && part && wbeta && out, "han_sem_fwd: null pointer");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t rows = N * M;
  const int nb = sem_blocks(rows);
  if (D <= 64) sem_score_kernel<64><<<nb, kBlock, 0, st>>>(z, W1, b1, q, part, rows, static_cast<int>(M), static_cast<int>(D));
  else sem_score_kernel<128><<<nb, kBlock, 0, st>>>(z, W1, b1, q, part, rows, static_cast<int>(M), static_cast<int>(D));
  sem_stage2_kernel<<<1, kBlock, 0, st>>>(part, nb, static_cast<int>(M), 1.f / static_cast<float>(N), 0, wbeta, nullptr);
  const int64_t total = N * D;
  sem_combine_kernel<<<static_cast<unsigned>((total + kBlock - 1) / kBlock), kBlock, 0, st>>>(z, wbeta, out, total, static_cast<int>(M),
                                                                                               static_cast<int>(D));
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_han_sem_bwd(const float* z, const float* W1, const float* b1, const float* q, const float* wbeta,
                                  const float* gout, float* part, float* gsm, float* gz, float* ppart, float* gparams, int64_t N,
                                  int64_t M, int64_t D, int64_t hidden, void* stream) {
  clear_error();
  int rc = check_sem("han_sem_bwd", N, M, D, hidden);
  if (rc != ALLSET_OK) return rc;
  ALLSET_REQUIRE(z && W1 && b1 && q && wbeta && gout && part && gsm && gz && ppart && gparams, "han_sem_bwd: null pointer");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t rows = N * M;
  const int nb = sem_blocks(rows);
  sem_dot_kernel<<<nb, kBlock, 0, st>>>(z, gout, part, rows, static_cast<int>(M), static_cast<int>(D));
  sem_stage2_kernel<<<1, kBlock, 0, st>>>(part, nb, static_cast<int>(M), 1.f / static_cast<float>(N), 1, const_cast<float*>(wbeta), gsm);
  if (D <= 64) sem_bwd_kernel<64><<<nb, kBlock, 0, st>>>(z, W1, b1, q, wbeta, gsm, gout, gz, ppart, rows, static_cast<int>(M), static_cast<int>(D));
  else sem_bwd_kernel<128><<<nb, kBlock, 0, st>>>(z, W1, b1, q, wbeta, gsm, gout, gz, ppart, rows, static_cast<int>(M), static_cast<int>(D));
  const int64_t P = kHid * D + 2 * kHid;
  sem_reduce_kernel<<<static_cast<unsigned>((P + kBlock - 1) / kBlock), kBlock, 0, st>>>(ppart, nb, P, gparams);
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}
