// Leave-one-out softmax for gfx950 (exclude-self AllSetTransformer without the k^2 expansion).
// For every position i of every CSR segment of k rows and every head h (a_j = leaky_relu(alpha[idx(j), h]), v_j = V[idx(j), h, :],
// idx(q) = col ? col[q] : q):
//   forward   o_i = sum_{j != i} exp(a_j) v_j / Z_i,   L_i = log Z_i,   Z_i = sum_{j != i} exp(a_j)      (k == 1: o = v, L = a)
//   backward  g_v,j = sum_{i != j} p_ij g_o,i,   g_a,j = <g_v,j, v_j> + sum_{i != j} p_ij (g_L,i - <g_o,i, o_i>),   p_ij = exp(a_j - L_i)
// Both are ONE shape: a leave-one-out reduction of rows that carry a log-weight w, a scalar x and a vector y,
//   S_i = (m, l, acc) = (max_{j != i} w_j,  sum_{j != i} exp(w_j - m) x_j,  sum_{j != i} exp(w_j - m) y_j)
//   forward:  w = a, x = 1, y = v:              o_i = acc / l,  L_i = m + log l
//   backward: w = -L, x = g_L - <g_o, o>, y = g_o:  g_v,j = exp(a_j + m) acc,  g_a,j = <g_v,j, v_j> + exp(a_j + m) l
// and S_i is the online-softmax merge of three states: the rows of i's run in front of i, those behind it, the other runs' totals --
// the prefix / suffix / other-runs traversal of loo.hip with sums replaced by merges.
//
// Numerics.  A state's reference m is the maximum of the rows IT holds, so every exp is taken at an argument <= 0 and every state
// that holds a row has a term exp(0) = 1: no overflow and no 0 / 0 however the logits are spread (one logit 100 above the rest:
// the position that omits it is a state of the OTHER rows, with their own maximum).  Nothing is ever "segment total minus own
// term".  Backward: L_i >= a_j for every j != i, so a_j + m = a_j - min_{i != j} L_i <= 0.  Empty state: m = -FLT_MAX, l = acc = 0
// (exp(-FLT_MAX - m) = 0; two empty states merge to an empty one).
//
// Mapping.  Heads are independent: a lane owns 16 B of ONE head; LH = pow2 >= C / 4 lanes (at most 64) cover a head, HP = LPR / LH heads
// sit side by side in a slot of LPR lanes (d = 128: the whole 512-B row per half-wave, as in loo.hip), further heads and the column
// chunks of a head wider than 256 are taken one after the other.  All per-head reductions (<g_o, o>, <g_v, v>) are xor butterflies
// over the LH lanes of the head.  Runs, the wave kernel, the workgroup kernel for segments longer than kLsmLong (the loo.hip
// threshold; long_seg lists them) and the two sweeps of a run longer than kLsmRows are those of loo.hip.  The suffix sweep parks the
// running suffix state of each position in the outputs: forward normalised (o, L) in out / lse; backward acc in gV and (m, l) in
// `scratch`.  The per-head scalars of a parked state are written by EVERY lane of the head (same value, same address) so that each
// lane reads back what it wrote itself; final per-head results are written by the head's first lane, which also adds up the column
// chunks of a wide head (the same lane in every chunk).  No atomics, no allocation, no sync; fixed order of operations.
#include <float.h>

#include "common.h"

namespace allset {

constexpr int kLsmRows = 8;                       // rows of a run a slot holds in registers
constexpr int kLsmLong = 64;                      // == kLooLong (allset_loo_long_threshold): one long_seg list serves both files
constexpr int kLsmBlock = 512;
constexpr int kLsmMaxD = 512;

struct LsmArgs {
  const int32_t* rowptr;
  const int32_t* col;        // null: rows are the positions themselves
  const float* alpha;        // [n_src, H] pre-activation logits
  const float* V;            // [n_src, ldv]
  int64_t ldv;
  float slope;
  float* out;                // forward: o [nnz, ldo];  backward: gV [nnz, ldo]
  int64_t ldo;
  float* sc;                 // forward: lse [nnz, H];  backward: galpha [nnz, H]
  // backward only
  const float* o;            // saved forward output [nnz, ldso]
  int64_t ldso;
  const float* lse;          // saved [nnz, H]
  const float* gout;         // [nnz, ldg]
  int64_t ldg;
  const float* glse;         // [nnz, H] or null (zeros)
  float* scratch;            // [nnz, H, 2]: (m, l) of parked suffix states
  int H, C, LH;
};

struct LsmState {
  float m, l, acc[4];
};

__device__ __forceinline__ void lsm_clear(LsmState& s) {
  s.m = -FLT_MAX;
  s.l = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) s.acc[c] = 0.f;
}

__device__ __forceinline__ void lsm_add_row(LsmState& s, float w, float x, const float (&y)[4]) {
  const float mn = fmaxf(s.m, w);
  const float a = __expf(s.m - mn), b = __expf(w - mn);
  s.l = fmaf(s.l, a, b * x);
#pragma unroll
  for (int c = 0; c < 4; ++c) s.acc[c] = fmaf(s.acc[c], a, b * y[c]);
  s.m = mn;
}

__device__ __forceinline__ void lsm_merge(LsmState& s, const LsmState& t) {
  const float mn = fmaxf(s.m, t.m);
  const float a = __expf(s.m - mn), b = __expf(t.m - mn);
  s.l = fmaf(s.l, a, b * t.l);
#pragma unroll
  for (int c = 0; c < 4; ++c) s.acc[c] = fmaf(s.acc[c], a, b * t.acc[c]);
  s.m = mn;
}

// where a lane works: head h, columns [c0, c0 + 4) of the row, cc = the first of them inside the head
struct LsmLane {
  int h, c0, li;             // (h clamped into [0, H) for lanes beyond the last head: they index nothing out of range)
  bool head_on, active;      // the lane's head exists; ... and so do its columns
};

__device__ __forceinline__ float lsm_head_sum(float v, int LH) {
  for (int off = LH >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__device__ __forceinline__ void lsm_load4(const float* p, bool on, float (&r)[4]) {
  const float4 t = on ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
  r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
}

__device__ __forceinline__ void lsm_store4(float* p, const float (&r)[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(r[0], r[1], r[2], r[3]);
}

// rows q0 .. q0 + n of a run as (w, x, y); rows beyond n are empty (w = -FLT_MAX, x = 0, y = 0) and change no state they are added to
template <bool BWD>
__device__ __forceinline__ void lsm_load(const LsmArgs& a, const LsmLane& ln, int q0, int n, float (&w)[kLsmRows], float (&x)[kLsmRows],
                                         float (&y)[kLsmRows][4]) {
  if constexpr (!BWD) {
    int idx[kLsmRows];
#pragma unroll
    for (int u = 0; u < kLsmRows; ++u) idx[u] = (u < n && a.col != nullptr) ? a.col[q0 + u] : q0 + u;
#pragma unroll
    for (int u = 0; u < kLsmRows; ++u) {
      const bool on = u < n && ln.active;
      lsm_load4(a.V + static_cast<int64_t>(idx[u]) * a.ldv + ln.c0, on, y[u]);
      w[u] = on ? leaky_relu(a.alpha[static_cast<int64_t>(idx[u]) * a.H + ln.h], a.slope) : -FLT_MAX;
      x[u] = on ? 1.f : 0.f;
    }
  } else {
    const bool single = a.C <= a.LH * 4;                          // the head's columns are one chunk: y is the g_o of <g_o, o>
#pragma unroll
    for (int u = 0; u < kLsmRows; ++u) {
      const bool on = u < n && ln.active;
      const int64_t q = q0 + u;
      lsm_load4(a.gout + q * a.ldg + ln.c0, on, y[u]);
      float part = 0.f;
      if (single) {
        float ov[4];
        lsm_load4(a.o + q * a.ldso + ln.c0, on, ov);
#pragma unroll
        for (int c = 0; c < 4; ++c) part = fmaf(ov[c], y[u][c], part);
      } else {
        for (int c2 = ln.li * 4; c2 < a.C; c2 += a.LH * 4) {      // (a head wider than 256 columns: every chunk needs the whole dot)
          float ov[4], gv[4];
          const bool on2 = u < n && ln.head_on;
          lsm_load4(a.o + q * a.ldso + ln.h * a.C + c2, on2, ov);
          lsm_load4(a.gout + q * a.ldg + ln.h * a.C + c2, on2, gv);
#pragma unroll
          for (int c = 0; c < 4; ++c) part = fmaf(ov[c], gv[c], part);
        }
      }
      const float delta = lsm_head_sum(part, a.LH);
      w[u] = on ? -a.lse[q * a.H + ln.h] : -FLT_MAX;
      x[u] = on ? (a.glse != nullptr ? a.glse[q * a.H + ln.h] : 0.f) - delta : 0.f;
    }
  }
}

// the result of position p from its leave-one-out state; `first` = the first column chunk of the head
template <bool BWD>
__device__ __forceinline__ void lsm_finish(const LsmArgs& a, const LsmLane& ln, int p, const LsmState& s, bool first) {
  if constexpr (!BWD) {
    if (!ln.active) return;
    const float inv = 1.f / s.l;
    float r[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) r[c] = s.acc[c] * inv;
    lsm_store4(a.out + static_cast<int64_t>(p) * a.ldo + ln.c0, r);
    if (ln.li == 0) a.sc[static_cast<int64_t>(p) * a.H + ln.h] = s.m + __logf(s.l);
  } else {
    const int64_t j = a.col != nullptr ? a.col[p] : p;
    float vj[4], r[4];
    lsm_load4(a.V + j * a.ldv + ln.c0, ln.active, vj);
    const float al = ln.active ? a.alpha[j * a.H + ln.h] : 0.f;
    const float f = ln.active ? __expf(leaky_relu(al, a.slope) + s.m) : 0.f;
    float part = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      r[c] = f * s.acc[c];
      part = fmaf(r[c], vj[c], part);
    }
    part = lsm_head_sum(part, a.LH);
    if (!ln.active) return;
    lsm_store4(a.out + static_cast<int64_t>(p) * a.ldo + ln.c0, r);
    if (ln.li == 0) {
      const float dact = al > 0.f ? 1.f : a.slope;
      float* g = a.sc + static_cast<int64_t>(p) * a.H + ln.h;
      *g = first ? dact * (part + f * s.l) : *g + dact * part;   // (the same lane in every chunk of a wide head)
    }
  }
}

// a singleton keeps its row: o = v, L = a, bit for bit; backward g_v = g_o, g_a = g_L * leaky_relu'
template <bool BWD>
__device__ __forceinline__ void lsm_singleton(const LsmArgs& a, const LsmLane& ln, int p, bool first) {
  if (!ln.active) return;
  const int64_t j = a.col != nullptr ? a.col[p] : p;
  float r[4];
  if constexpr (!BWD) {
    lsm_load4(a.V + j * a.ldv + ln.c0, true, r);
    lsm_store4(a.out + static_cast<int64_t>(p) * a.ldo + ln.c0, r);
    if (ln.li == 0 && first) a.sc[static_cast<int64_t>(p) * a.H + ln.h] = leaky_relu(a.alpha[j * a.H + ln.h], a.slope);
  } else {
    lsm_load4(a.gout + static_cast<int64_t>(p) * a.ldg + ln.c0, true, r);
    lsm_store4(a.out + static_cast<int64_t>(p) * a.ldo + ln.c0, r);
    if (ln.li == 0 && first) {
      const float gl = a.glse != nullptr ? a.glse[static_cast<int64_t>(p) * a.H + ln.h] : 0.f;
      a.sc[static_cast<int64_t>(p) * a.H + ln.h] = gl * (a.alpha[j * a.H + ln.h] > 0.f ? 1.f : a.slope);
    }
  }
}

// park / fetch the suffix state of position p (two-sweep path; see the header)
template <bool BWD>
__device__ __forceinline__ void lsm_park(const LsmArgs& a, const LsmLane& ln, int p, const LsmState& s) {
  if (!ln.active) return;
  float r[4];
  if constexpr (!BWD) {
    const float inv = s.l > 0.f ? 1.f / s.l : 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) r[c] = s.acc[c] * inv;
    a.sc[static_cast<int64_t>(p) * a.H + ln.h] = s.l > 0.f ? s.m + __logf(s.l) : -FLT_MAX;
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) r[c] = s.acc[c];
    *reinterpret_cast<float2*>(a.scratch + (static_cast<int64_t>(p) * a.H + ln.h) * 2) = make_float2(s.m, s.l);
  }
  lsm_store4(a.out + static_cast<int64_t>(p) * a.ldo + ln.c0, r);
}

template <bool BWD>
__device__ __forceinline__ void lsm_fetch(const LsmArgs& a, const LsmLane& ln, int p, LsmState& s) {
  lsm_clear(s);
  if (!ln.active) return;
  lsm_load4(a.out + static_cast<int64_t>(p) * a.ldo + ln.c0, true, s.acc);
  if constexpr (!BWD) {
    s.m = a.sc[static_cast<int64_t>(p) * a.H + ln.h];
    s.l = s.m > -FLT_MAX ? 1.f : 0.f;
  } else {
    const float2 t = *reinterpret_cast<const float2*>(a.scratch + (static_cast<int64_t>(p) * a.H + ln.h) * 2);
    s.m = t.x;
    s.l = t.y;
  }
}

// One (head group, column chunk) of one segment [start, end) of k >= 2 rows for the slot `s` of `nslots`.  exchange(total, others):
// others = the merge of the other slots' totals; called exactly once, by every lane of the group, at a point all of them reach together.
template <bool BWD, typename Exchange>
__device__ __forceinline__ void lsm_segment(const LsmArgs& a, const LsmLane& ln, int start, int end, int s, int nslots, bool first,
                                            Exchange exchange) {
  const int k = end - start;
  const int per = (k + nslots - 1) / nslots;                    // run length (the last runs may be shorter or empty)
  const int ra = min(start + s * per, end), rb = min(ra + per, end);
  const int len = rb - ra;
  float w[kLsmRows], x[kLsmRows], y[kLsmRows][4];
  LsmState total, others, pre;

  if (per <= kLsmRows) {                                        // (uniform over the group) every run fits in registers
    lsm_load<BWD>(a, ln, ra, len, w, x, y);
    LsmState suf[kLsmRows];                                     // exclusive suffix inside the run (rows beyond len are empty)
    lsm_clear(suf[kLsmRows - 1]);
#pragma unroll
    for (int u = kLsmRows - 2; u >= 0; --u) {
      suf[u] = suf[u + 1];
      lsm_add_row(suf[u], w[u + 1], x[u + 1], y[u + 1]);
    }
    total = suf[0];
    lsm_add_row(total, w[0], x[0], y[0]);
    exchange(total, others);
    lsm_clear(pre);
#pragma unroll
    for (int u = 0; u < kLsmRows; ++u) {
      if (u < len) {                                            // (uniform over the slot: the head sums inside stay among its lanes)
        LsmState st = pre;
        lsm_merge(st, suf[u]);
        lsm_merge(st, others);
        lsm_finish<BWD>(a, ln, ra + u, st, first);
      }
      lsm_add_row(pre, w[u], x[u], y[u]);
    }
    return;
  }

  // long runs: two sweeps over the run in tiles of kLsmRows rows
  const int ntile = (len + kLsmRows - 1) / kLsmRows;
  lsm_clear(total);
  for (int t = ntile - 1; t >= 0; --t) {                        // backward: park the state of the run's rows behind p
    const int q0 = ra + t * kLsmRows, n = min(kLsmRows, rb - q0);
    lsm_load<BWD>(a, ln, q0, n, w, x, y);
#pragma unroll
    for (int u = kLsmRows - 1; u >= 0; --u) {
      if (u < n) lsm_park<BWD>(a, ln, q0 + u, total);
      lsm_add_row(total, w[u], x[u], y[u]);
    }
  }
  exchange(total, others);
  lsm_clear(pre);
  for (int t = 0; t < ntile; ++t) {                             // forward: merge the rows in front of p and the other runs
    const int q0 = ra + t * kLsmRows, n = min(kLsmRows, rb - q0);
    lsm_load<BWD>(a, ln, q0, n, w, x, y);
#pragma unroll
    for (int u = 0; u < kLsmRows; ++u) {
      if (u < n) {
        LsmState st;                                            // (position q0 + u's own parked state: no other position's result
        lsm_fetch<BWD>(a, ln, q0 + u, st);                      //  has been written over it)
        lsm_merge(st, pre);
        lsm_merge(st, others);
        lsm_finish<BWD>(a, ln, q0 + u, st, first);
      }
      lsm_add_row(pre, w[u], x[u], y[u]);
    }
  }
}

__device__ __forceinline__ LsmLane lsm_lane(const LsmArgs& a, int lr, int hb, int cb) {
  LsmLane ln;
  ln.li = lr % a.LH;
  const int h = hb + lr / a.LH, cc = cb + ln.li * 4;
  ln.head_on = h < a.H;
  ln.active = ln.head_on && cc < a.C;
  ln.h = min(h, a.H - 1);
  ln.c0 = ln.active ? ln.h * a.C + cc : 0;
  return ln;
}

template <bool BWD, int LPR>
__global__ __launch_bounds__(kBlock) void lsm_wave_kernel(LsmArgs a, int n_seg, int skip_long) {
  constexpr int NS = kWave / LPR;
  const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int seg = static_cast<int>(blk) * kWavesPerBlock + (threadIdx.x >> 6);
  if (seg >= n_seg) return;                                     // whole wave exits together
  const int start = a.rowptr[seg], end = a.rowptr[seg + 1];
  if (end <= start || (skip_long && end - start > kLsmLong)) return;
  const int lane = lane_id();
  const int s = lane / LPR, lr = lane % LPR;
  auto exchange = [](const LsmState& total, LsmState& others) {
    lsm_clear(others);
#pragma unroll
    for (int m = 1; m < NS; ++m) {
      LsmState t;
      t.m = __shfl_xor(total.m, m * LPR);
      t.l = __shfl_xor(total.l, m * LPR);
#pragma unroll
      for (int c = 0; c < 4; ++c) t.acc[c] = __shfl_xor(total.acc[c], m * LPR);
      lsm_merge(others, t);
    }
  };
  const int HP = LPR / a.LH;
  for (int hb = 0; hb < a.H; hb += HP)
    for (int cb = 0; cb < a.C; cb += a.LH * 4) {
      const LsmLane ln = lsm_lane(a, lr, hb, cb);
      if (end - start == 1) {
        if (s == 0) lsm_singleton<BWD>(a, ln, start, cb == 0);
      } else {
        lsm_segment<BWD>(a, ln, start, end, s, NS, cb == 0, exchange);
      }
    }
}

template <bool BWD, int LPR>
__global__ __launch_bounds__(kLsmBlock) void lsm_block_kernel(LsmArgs a, const int32_t* __restrict__ long_seg, int n_seg) {
  constexpr int NSLOT = kLsmBlock / LPR;
  __shared__ float totals[kLsmBlock * 6];
  const int seg = long_seg != nullptr ? long_seg[blockIdx.x] : static_cast<int>(blockIdx.x);
  if (seg < 0 || seg >= n_seg) return;                          // (uniform over the workgroup, as every exit here)
  const int start = a.rowptr[seg], end = a.rowptr[seg + 1];
  if (end - start <= kLsmLong) return;                          // the wave kernel's
  const int tid = threadIdx.x;
  const int s = tid / LPR, lr = tid % LPR;
  auto exchange = [&](const LsmState& total, LsmState& others) {
    totals[tid * 6 + 0] = total.m;
    totals[tid * 6 + 1] = total.l;
#pragma unroll
    for (int c = 0; c < 4; ++c) totals[tid * 6 + 2 + c] = total.acc[c];
    __syncthreads();
    lsm_clear(others);
    for (int m = 0; m < NSLOT; ++m) {                           // fixed order; the own run enters as an empty state
      const float* p = &totals[(m * LPR + lr) * 6];
      LsmState t;
      t.m = m != s ? p[0] : -FLT_MAX;
      t.l = m != s ? p[1] : 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) t.acc[c] = m != s ? p[2 + c] : 0.f;
      lsm_merge(others, t);
    }
    __syncthreads();                                            // before the next chunk overwrites the totals
  };
  const int HP = LPR / a.LH;
  for (int hb = 0; hb < a.H; hb += HP)
    for (int cb = 0; cb < a.C; cb += a.LH * 4) {
      const LsmLane ln = lsm_lane(a, lr, hb, cb);
      lsm_segment<BWD>(a, ln, start, end, s, NSLOT, cb == 0, exchange);
    }
}

static inline int lsm_lanes_per_head(int64_t C) {
  int lh = 1;
  while (lh * 4 < C && lh < 64) lh <<= 1;
  return lh;
}

static inline int lsm_lpr(int64_t H, int lh) {
  int lpr = 8;
  while (lpr < H * lh && lpr < 64) lpr <<= 1;
  return lpr;
}

template <bool BWD>
static int lsm_launch(const char* who, LsmArgs a, const int32_t* long_seg, int64_t n_long, int64_t n_seg, int64_t n_src, int64_t nnz,
                      int64_t d, int64_t heads, void* stream) {
  ALLSET_REQUIRE(n_seg >= 0 && n_src >= 0 && nnz >= 0 && d >= 0, "%s: negative size", who);
  ALLSET_REQUIRE(n_seg < INT32_MAX && n_src < INT32_MAX && nnz < INT32_MAX, "%s: size exceeds int32", who);
  if (n_seg == 0 || nnz == 0 || d == 0) return ALLSET_OK;
  if (!allset_loo_softmax_supported(d, heads)) {
    set_error("%s: d = %lld with %lld heads is not built (heads 1 | 2 | 4 | 8, (d / heads) %% 4 == 0, d <= %d)", who,
              static_cast<long long>(d), static_cast<long long>(heads), kLsmMaxD);
    return ALLSET_ERR_UNSUPPORTED;
  }
  ALLSET_REQUIRE(a.rowptr && a.alpha && a.V && a.out && a.sc, "%s: null rowptr/alpha/V/output", who);
  ALLSET_REQUIRE(n_src > 0, "%s: an empty source table with nnz > 0", who);
  ALLSET_REQUIRE(a.col != nullptr || n_src >= nnz, "%s: null col (contiguous rows) needs n_src >= nnz", who);
  ALLSET_REQUIRE(a.ldv >= d && a.ldo >= d, "%s: leading dimension smaller than d", who);
  ALLSET_REQUIRE(a.ldv % 4 == 0 && a.ldo % 4 == 0 && aligned16(a.V) && aligned16(a.out), "%s: rows must be 16-byte aligned", who);
  ALLSET_REQUIRE(static_cast<const void*>(a.V) != static_cast<const void*>(a.out), "%s: the output may not alias V", who);
  if (BWD) {
    ALLSET_REQUIRE(a.o && a.lse && a.gout && a.scratch, "%s: null out/lse/gout/scratch", who);
    ALLSET_REQUIRE(a.ldso >= d && a.ldg >= d && a.ldso % 4 == 0 && a.ldg % 4 == 0 && aligned16(a.o) && aligned16(a.gout),
                   "%s: out / gout rows must be 16-byte aligned and at least d wide", who);
    ALLSET_REQUIRE((reinterpret_cast<uintptr_t>(a.scratch) & 7u) == 0, "%s: scratch must be 8-byte aligned", who);
    ALLSET_REQUIRE(static_cast<const void*>(a.gout) != static_cast<const void*>(a.out) &&
                       static_cast<const void*>(a.o) != static_cast<const void*>(a.out),
                   "%s: gV may not alias gout or out", who);
    ALLSET_REQUIRE(static_cast<const void*>(a.glse) != static_cast<const void*>(a.sc) &&
                       static_cast<const void*>(a.lse) != static_cast<const void*>(a.sc),
                   "%s: galpha may not alias glse or lse", who);
  }
  ALLSET_REQUIRE(n_long <= n_seg, "%s: n_long exceeds n_seg", who);
  ALLSET_REQUIRE(n_long <= 0 || long_seg != nullptr, "%s: null long_seg with n_long > 0", who);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  a.H = static_cast<int>(heads);
  a.C = static_cast<int>(d / heads);
  a.LH = lsm_lanes_per_head(a.C);
  const int ns = static_cast<int>(n_seg);
  // n_long < 0: long segments unknown -- one workgroup per segment looks (and leaves at once unless its segment is long);
  // n_long == 0: the caller states there is none -- the wave kernel takes every segment; n_long > 0: the list.
  const unsigned wave_grid = static_cast<unsigned>((n_seg + kWavesPerBlock - 1) / kWavesPerBlock);
  const unsigned block_grid = n_long < 0 ? static_cast<unsigned>(n_seg) : static_cast<unsigned>(n_long);
  const int32_t* list = n_long > 0 ? long_seg : nullptr;
  const int skip_long = n_long != 0;
#define ALLSET_LSM(LPR_)                                                                                   \
  do {                                                                                                     \
    lsm_wave_kernel<BWD, LPR_><<<wave_grid, kBlock, 0, st>>>(a, ns, skip_long);                            \
    if (block_grid > 0) lsm_block_kernel<BWD, LPR_><<<block_grid, kLsmBlock, 0, st>>>(a, list, ns);        \
  } while (0)
  switch (lsm_lpr(heads, a.LH)) {
    case 8:  ALLSET_LSM(8); break;
    case 16: ALLSET_LSM(16); break;
    case 32: ALLSET_LSM(32); break;
    default: ALLSET_LSM(64); break;
  }
#undef ALLSET_LSM
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

}  // namespace allset

using namespace allset;

extern "C" int allset_loo_softmax_supported(int64_t d, int64_t heads) {
  if (!(heads == 1 || heads == 2 || heads == 4 || heads == 8)) return 0;
  return d > 0 && d <= kLsmMaxD && d % heads == 0 && (d / heads) % 4 == 0;
}

extern "C" int allset_loo_softmax_fwd(const int32_t* rowptr, const int32_t* col, const float* alpha, const float* V, int64_t ldv,
                                      float slope, float* out, int64_t ldo, float* lse, const int32_t* long_seg, int64_t n_long,
                                      int64_t n_seg, int64_t n_src, int64_t nnz, int64_t d, int64_t heads, void* stream) {
  clear_error();
  LsmArgs a{};
  a.rowptr = rowptr; a.col = col; a.alpha = alpha; a.V = V; a.ldv = ldv; a.slope = slope;
  a.out = out; a.ldo = ldo; a.sc = lse;
  return lsm_launch<false>("loo_softmax_fwd", a, long_seg, n_long, n_seg, n_src, nnz, d, heads, stream);
}

extern "C" int allset_loo_softmax_bwd(const int32_t* rowptr, const int32_t* col, const float* alpha, const float* V, int64_t ldv,
                                      float slope, const float* out, int64_t ldo, const float* lse, const float* gout, int64_t ldg,
                                      const float* glse, float* gV, int64_t ldgv, float* galpha, float* scratch,
                                      const int32_t* long_seg, int64_t n_long, int64_t n_seg, int64_t n_src, int64_t nnz, int64_t d,
                                      int64_t heads, void* stream) {
  clear_error();
  LsmArgs a{};
  a.rowptr = rowptr; a.col = col; a.alpha = alpha; a.V = V; a.ldv = ldv; a.slope = slope;
  a.out = gV; a.ldo = ldgv; a.sc = galpha;
  a.o = out; a.ldso = ldo; a.lse = lse; a.gout = gout; a.ldg = ldg; a.glse = glse; a.scratch = scratch;
  return lsm_launch<true>("loo_softmax_bwd", a, long_seg, n_long, n_seg, n_src, nnz, d, heads, stream);
}
