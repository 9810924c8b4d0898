// Leave-one-out segmented sums for gfx950 (exclude-self Deep Sets without the k^2 expansion):
//   out[p,:] = s_seg[g] * sum_{q in segment g, q != p} s_src[idx(q)] * src[idx(q),:]      idx(q) = col ? col[q] : q
// for every position p of every CSR segment g (a segment of one position keeps its own row, as the reference keeps a
// singleton hyperedge).  One output row per incidence; the k rows of a segment share k inputs, so the traffic is that of
// one gather pass plus one write of [nnz, d] instead of the expansion's k - 1 gathers per output row.
//
// Every output is the sum of exactly the k - 1 terms it stands for -- an exclusive prefix plus an exclusive suffix, never
// "total minus own row" (accurate only relative to the total).  A segment is cut into contiguous RUNS, one per lane group:
//   out[p] = s_seg * ((prefix inside the run + suffix inside the run) + sum of the OTHER runs' totals).
//
// Mapping to the machine (the discipline of segreduce.hip): a feature row of d f32 is covered by LPR lanes x 16 B, so a
// wave holds NS = 64 / LPR lane groups ("slots"; d = 128: one 512-B row per half-wave); a slot keeps kLooRows rows of its
// run in registers as packed 16-byte loads issued back to back (8 KiB in flight per wave).  d > 256: column chunks.
//   * loo_wave_kernel: one wave per segment, 4 segments per workgroup, run totals exchanged by xor-shuffles.  A segment of
//     at most NS * kLooRows rows is read once and written once.
//   * loo_block_kernel: one 512-thread workgroup per segment longer than kLooLong (8 waves, 8 * NS runs; run totals
//     exchanged through LDS): the two-level scan -- runs in parallel, then the scan over run totals.
//   * a run longer than kLooRows takes two sweeps: backward, writing the exclusive suffix inside the run to `out` and
//     ending with the run's total; forward, re-reading the rows (from cache) and that suffix and writing the result.
// No atomics: every output has one writer and a fixed order of additions.
#include "common.h"
#include "seg_rows.h"

namespace allset {

// One column chunk of one segment [start, end) for the slot `s` of `nslots`.  exchange(total, others): others = the sum of
// the other slots' totals; called exactly once, by every lane of the group, at a point all of them reach together.
template <typename Exchange>
__device__ __forceinline__ void loo_segment(const LooArgs& a, int start, int end, int s, int nslots, int c0, bool active,
                                            float sseg, Exchange exchange) {
  const int k = end - start;
  const int per = (k + nslots - 1) / nslots;                    // run length (the last runs may be shorter or empty)
  const int ra = min(start + s * per, end), rb = min(ra + per, end);
  const int len = rb - ra;
  float total[4], others[4], v[kLooRows][4];

  if (per <= kLooRows) {                                        // (uniform over the group) every run fits in registers
    loo_load(a, ra, len, c0, active, v);
#pragma unroll
    for (int c = 0; c < 4; ++c) total[c] = 0.f;
#pragma unroll
    for (int u = 0; u < kLooRows; ++u)
#pragma unroll
      for (int c = 0; c < 4; ++c) total[c] += v[u][c];
    exchange(total, others);
    if (k == 1) {                                               // a singleton keeps its member
      if (len == 1 && active) {
        float r[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) r[c] = sseg * v[0][c];
        loo_store(a, ra, c0, r);
      }
      return;
    }
    float suf[kLooRows][4];                                     // exclusive suffix inside the run (rows beyond len are zero)
#pragma unroll
    for (int c = 0; c < 4; ++c) suf[kLooRows - 1][c] = 0.f;
#pragma unroll
    for (int u = kLooRows - 2; u >= 0; --u)
#pragma unroll
      for (int c = 0; c < 4; ++c) suf[u][c] = suf[u + 1][c] + v[u + 1][c];
    float pre[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < kLooRows; ++u) {
      if (u < len && active) {
        float r[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) r[c] = sseg * ((pre[c] + suf[u][c]) + others[c]);
        loo_store(a, ra + u, c0, r);
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) pre[c] += v[u][c];
    }
    return;
  }

  // long runs (k > nslots * kLooRows >= 8, never a singleton): two sweeps over the run in tiles of kLooRows rows
  const int ntile = (len + kLooRows - 1) / kLooRows;
#pragma unroll
  for (int c = 0; c < 4; ++c) total[c] = 0.f;
  for (int t = ntile - 1; t >= 0; --t) {                        // backward: out[p] = sum of the run's rows behind p
    const int q0 = ra + t * kLooRows, n = min(kLooRows, rb - q0);
    loo_load(a, q0, n, c0, active, v);
#pragma unroll
    for (int u = kLooRows - 1; u >= 0; --u) {
      if (u < n && active) loo_store(a, q0 + u, c0, total);
#pragma unroll
      for (int c = 0; c < 4; ++c) total[c] += v[u][c];
    }
  }
  exchange(total, others);
  float pre[4] = {0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < ntile; ++t) {                             // forward: + the rows in front of p + the other runs
    const int q0 = ra + t * kLooRows, n = min(kLooRows, rb - q0);
    loo_load(a, q0, n, c0, active, v);
    float o[kLooRows][4];
#pragma unroll
    for (int u = 0; u < kLooRows; ++u) {
      if (u < n && active) {
        const float4 w = *reinterpret_cast<const float4*>(a.out + static_cast<int64_t>(q0 + u) * a.ldo + c0);
        o[u][0] = w.x; o[u][1] = w.y; o[u][2] = w.z; o[u][3] = w.w;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) o[u][c] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < kLooRows; ++u) {
      if (u < n && active) {
        float r[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) r[c] = sseg * ((pre[c] + o[u][c]) + others[c]);
        loo_store(a, q0 + u, c0, r);
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) pre[c] += v[u][c];
    }
  }
}

template <int LPR>
__global__ __launch_bounds__(kBlock) void loo_wave_kernel(LooArgs a, int n_seg, int skip_long) {
  constexpr int NS = kWave / LPR;
  const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int seg = static_cast<int>(blk) * kWavesPerBlock + (threadIdx.x >> 6);
  if (seg >= n_seg) return;                                     // whole wave exits together
  const int start = a.rowptr[seg], end = a.rowptr[seg + 1];
  if (end <= start || (skip_long && end - start > kLooLong)) return;
  const int lane = lane_id();
  const int s = lane / LPR, li = lane % LPR;
  const float sseg = a.s_seg != nullptr ? a.s_seg[seg] : 1.f;
  auto exchange = [](const float (&total)[4], float (&others)[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      others[c] = 0.f;
#pragma unroll
      for (int m = 1; m < NS; ++m) others[c] += __shfl_xor(total[c], m * LPR);
    }
  };
  for (int cb = 0; cb < a.d; cb += LPR * 4) {
    const int c0 = cb + li * 4;
    loo_segment(a, start, end, s, NS, c0, c0 < a.d, sseg, exchange);
  }
}

template <int LPR>
__global__ __launch_bounds__(kLooBlock) void loo_block_kernel(LooArgs a, const int32_t* __restrict__ long_seg, int n_seg) {
  constexpr int NSLOT = kLooBlock / LPR;
  __shared__ float totals[kLooBlock * 4];
  const int seg = long_seg != nullptr ? long_seg[blockIdx.x] : static_cast<int>(blockIdx.x);
  if (seg < 0 || seg >= n_seg) return;                          // (uniform over the workgroup, as every exit here)
  const int start = a.rowptr[seg], end = a.rowptr[seg + 1];
  if (end - start <= kLooLong) return;                          // the wave kernel's
  const int tid = threadIdx.x;
  const int s = tid / LPR, li = tid % LPR;
  const float sseg = a.s_seg != nullptr ? a.s_seg[seg] : 1.f;
  auto exchange = [&](const float (&total)[4], float (&others)[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) totals[tid * 4 + c] = total[c];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) others[c] = 0.f;
    for (int m = 0; m < NSLOT; ++m) {                           // fixed order; the own run contributes an exact zero
      const float4 w = *reinterpret_cast<const float4*>(&totals[(m * LPR + li) * 4]);
      const bool other = m != s;
      others[0] += other ? w.x : 0.f; others[1] += other ? w.y : 0.f;
      others[2] += other ? w.z : 0.f; others[3] += other ? w.w : 0.f;
    }
    __syncthreads();                                            // before the next column chunk overwrites the totals
  };
  for (int cb = 0; cb < a.d; cb += LPR * 4) {
    const int c0 = cb + li * 4;
    loo_segment(a, start, end, s, NSLOT, c0, c0 < a.d, sseg, exchange);
  }
}

}  // namespace allset

using namespace allset;

extern "C" int allset_loo_supported(int64_t d) { return d > 0 && d % 4 == 0 && d <= kLooMaxD; }

extern "C" int allset_loo_long_threshold(void) { return kLooLong; }

extern "C" int allset_loo_rows(const int32_t* rowptr, const int32_t* col, const float* src, int64_t lds, const float* s_src,
                               const float* s_seg, float* out, int64_t ldo, const int32_t* long_seg, int64_t n_long,
                               int64_t n_seg, int64_t n_src, int64_t nnz, int64_t d, void* stream) {
  clear_error();
  ALLSET_REQUIRE(n_seg >= 0 && n_src >= 0 && nnz >= 0 && d >= 0, "loo_rows: negative size");
  ALLSET_REQUIRE(n_seg < INT32_MAX && n_src < INT32_MAX && nnz < INT32_MAX, "loo_rows: size exceeds int32");
  if (n_seg == 0 || nnz == 0 || d == 0) return ALLSET_OK;
  if (!allset_loo_supported(d)) {
    set_error("loo_rows: width %lld is not built (d %% 4 == 0, d <= %d)", static_cast<long long>(d), kLooMaxD);
    return ALLSET_ERR_UNSUPPORTED;
  }
  ALLSET_REQUIRE(rowptr && src && out, "loo_rows: null rowptr/src/out");
  ALLSET_REQUIRE(n_src > 0, "loo_rows: an empty source table with nnz > 0");
  ALLSET_REQUIRE(col != nullptr || n_src >= nnz, "loo_rows: null col (contiguous rows) needs n_src >= nnz");
  ALLSET_REQUIRE(lds >= d && ldo >= d, "loo_rows: leading dimension smaller than d");
  ALLSET_REQUIRE(lds % 4 == 0 && ldo % 4 == 0 && aligned16(src) && aligned16(out), "loo_rows: rows must be 16-byte aligned");
  ALLSET_REQUIRE(static_cast<const void*>(src) != static_cast<const void*>(out), "loo_rows: out may not alias src");
  ALLSET_REQUIRE(n_long <= n_seg, "loo_rows: n_long exceeds n_seg");
  ALLSET_REQUIRE(n_long <= 0 || long_seg != nullptr, "loo_rows: null long_seg with n_long > 0");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const LooArgs a{rowptr, col, src, lds, s_src, s_seg, out, ldo, static_cast<int>(d)};
  const int ns = static_cast<int>(n_seg);
  // n_long < 0: long segments unknown -- one workgroup per segment looks (and leaves at once unless its segment is long);
  // n_long == 0: the caller states there is none -- the wave kernel takes every segment; n_long > 0: the list.
  const unsigned wave_grid = static_cast<unsigned>((n_seg + kWavesPerBlock - 1) / kWavesPerBlock);
  const unsigned block_grid = n_long < 0 ? static_cast<unsigned>(n_seg) : static_cast<unsigned>(n_long);
  const int32_t* list = n_long > 0 ? long_seg : nullptr;
  const int skip_long = n_long != 0;
#define ALLSET_LOO(LPR_)                                                                              \
  do {                                                                                                \
    loo_wave_kernel<LPR_><<<wave_grid, kBlock, 0, st>>>(a, ns, skip_long);                            \
    if (block_grid > 0) loo_block_kernel<LPR_><<<block_grid, kLooBlock, 0, st>>>(a, list, ns);        \
  } while (0)
  switch (loo_lpr(d)) {
    case 8:  ALLSET_LOO(8); break;
    case 16: ALLSET_LOO(16); break;
    case 32: ALLSET_LOO(32); break;
    default: ALLSET_LOO(64); break;
  }
#undef ALLSET_LOO
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}
