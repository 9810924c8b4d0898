// CEGCN's GCN hop without the clique expansion, for gfx950.  Two launches per pass:
//
// (1) allset_scan_rows -- segmented EXCLUSIVE scan of gathered, scaled rows:
//   out[p,:] = sum_{q in the segment of p, q before p (reverse = 0) | q behind p (reverse = 1)} s_src[idx(q)] * src[idx(q),:]
//   idx(q) = col ? col[q] : q
// One output row per CSR position; the first position of a segment (reverse: the last) and every position of a segment of one get
// zeros.  Every output is the sum of exactly the terms it names: the totals of the RUNS in front of (behind) its own plus the rows in
// front of (behind) it inside its run -- never "segment total minus the rest".
// Mapping: loo.hip's (seg_rows.h): LPR lanes x 16 B per feature row, NS = 64 / LPR lane groups per wave, each keeping kLooRows rows of
// its contiguous run in registers; d > 256: column chunks.
//   * scan_wave_kernel: one wave per segment, 4 segments per workgroup, run totals exchanged by shuffles.
//   * scan_block_kernel: one 512-thread workgroup per segment longer than kLooLong, run totals exchanged through LDS.
//   * a run longer than kLooRows takes two sweeps: the first sums the run, the second re-reads its rows (from cache) and writes the
//     running sum that starts at the total of the runs in front (behind).  `out` is written once and never read.
// Algorithmic bytes: nnz * (2 * 4d + 4 [col] + 4 [s_src]) + (n_seg + 1) * 4.
//
// (2) allset_scan_collect -- the per-vertex sum of those rows plus the vertex's own row, with hconv.hip's row epilogue:
//   y[j,:] = drop_p( act( s[j] * ( sum_{p in row j} t[col_p,:] + r_self[j] * x[j,:] ) + bias ) )
// One wave per CSR row (hconv.hip's skeleton, without a per-incidence scale): the row's ids in one coalesced load, broadcast with
// shuffles, kUnroll gathers in flight per lane group.  The self term is read where it lies (no appended rows, no copy of x).
// Algorithmic bytes: nnz * (4d + 4) + (n_t + 1) * 4 + n_t * (2 * 4d + 8).
// No atomics: every output has one writer and a fixed order of additions.
#include "common.h"
#include "row_epilogue.h"
#include "seg_rows.h"

namespace allset {
namespace scan {

// One column chunk of one segment [start, end) for the slot `s` of `nslots`.  exchange(total, base): base = the sum of the totals of
// the slots in front of s (reverse: behind); called exactly once, by every lane of the group, at a point all of them reach together.
template <bool REV, typename Exchange>
__device__ __forceinline__ void scan_segment(const LooArgs& a, int start, int end, int s, int nslots, int c0, bool active,
                                             Exchange exchange) {
  const int k = end - start;
  const int per = (k + nslots - 1) / nslots;                    // run length (the last runs may be shorter or empty)
  const int ra = min(start + s * per, end), rb = min(ra + per, end);
  const int len = rb - ra;
  float total[4], run[4], v[kLooRows][4];
#pragma unroll
  for (int c = 0; c < 4; ++c) total[c] = 0.f;

  if (per <= kLooRows) {                                        // (uniform over the group) every run fits in registers
    loo_load(a, ra, len, c0, active, v);
#pragma unroll
    for (int u = 0; u < kLooRows; ++u)
#pragma unroll
      for (int c = 0; c < 4; ++c) total[c] += v[u][c];
    exchange(total, run);
    if constexpr (!REV) {
#pragma unroll
      for (int u = 0; u < kLooRows; ++u) {
        if (u < len && active) loo_store(a, ra + u, c0, run);
#pragma unroll
        for (int c = 0; c < 4; ++c) run[c] += v[u][c];
      }
    } else {
#pragma unroll
      for (int u = kLooRows - 1; u >= 0; --u) {                 // (rows beyond len are zero)
        if (u < len && active) loo_store(a, ra + u, c0, run);
#pragma unroll
        for (int c = 0; c < 4; ++c) run[c] += v[u][c];
      }
    }
    return;
  }

  // long runs: two sweeps over the run in tiles of kLooRows rows
  const int ntile = (len + kLooRows - 1) / kLooRows;
  for (int t = 0; t < ntile; ++t) {                             // the run's total
    const int q0 = ra + t * kLooRows;
    loo_load(a, q0, min(kLooRows, rb - q0), c0, active, v);
#pragma unroll
    for (int u = 0; u < kLooRows; ++u)
#pragma unroll
      for (int c = 0; c < 4; ++c) total[c] += v[u][c];
  }
  exchange(total, run);
  for (int i = 0; i < ntile; ++i) {                             // the running sum, from the runs in front (behind) on
    const int t = REV ? ntile - 1 - i : i;
    const int q0 = ra + t * kLooRows, n = min(kLooRows, rb - q0);
    loo_load(a, q0, n, c0, active, v);
#pragma unroll
    for (int j = 0; j < kLooRows; ++j) {
      const int u = REV ? kLooRows - 1 - j : j;
      if (u < n && active) loo_store(a, q0 + u, c0, run);
#pragma unroll
      for (int c = 0; c < 4; ++c) run[c] += v[u][c];
    }
  }
}

template <int LPR, bool REV>
__global__ __launch_bounds__(kBlock) void scan_wave_kernel(LooArgs a, int n_seg, int skip_long) {
  constexpr int NS = kWave / LPR;
  const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int seg = static_cast<int>(blk) * kWavesPerBlock + (threadIdx.x >> 6);
  if (seg >= n_seg) return;                                     // whole wave exits together
  const int start = a.rowptr[seg], end = a.rowptr[seg + 1];
  if (end <= start || (skip_long && end - start > kLooLong)) return;
  const int lane = lane_id();
  const int s = lane / LPR, li = lane % LPR;
  auto exchange = [=](const float (&total)[4], float (&base)[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      base[c] = 0.f;
#pragma unroll
      for (int m = 0; m < NS; ++m) {                            // fixed order; the other side contributes exact zeros
        const float t = __shfl(total[c], m * LPR + li);
        base[c] += (REV ? m > s : m < s) ? t : 0.f;
      }
    }
  };
  for (int cb = 0; cb < a.d; cb += LPR * 4) {
    const int c0 = cb + li * 4;
    scan_segment<REV>(a, start, end, s, NS, c0, c0 < a.d, exchange);
  }
}

template <int LPR, bool REV>
__global__ __launch_bounds__(kLooBlock) void scan_block_kernel(LooArgs a, const int32_t* __restrict__ long_seg, int n_seg) {
  constexpr int NSLOT = kLooBlock / LPR;
  __shared__ float totals[kLooBlock * 4];
  const int seg = long_seg != nullptr ? long_seg[blockIdx.x] : static_cast<int>(blockIdx.x);
  if (seg < 0 || seg >= n_seg) return;                          // (uniform over the workgroup, as every exit here)
  const int start = a.rowptr[seg], end = a.rowptr[seg + 1];
  if (end - start <= kLooLong) return;                          // the wave kernel's
  const int tid = threadIdx.x;
  const int s = tid / LPR, li = tid % LPR;
  auto exchange = [&](const float (&total)[4], float (&base)[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) totals[tid * 4 + c] = total[c];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) base[c] = 0.f;
    for (int m = 0; m < NSLOT; ++m) {                           // fixed order; the other side contributes exact zeros
      const float4 w = *reinterpret_cast<const float4*>(&totals[(m * LPR + li) * 4]);
      const bool take = REV ? m > s : m < s;
      base[0] += take ? w.x : 0.f; base[1] += take ? w.y : 0.f;
      base[2] += take ? w.z : 0.f; base[3] += take ? w.w : 0.f;
    }
    __syncthreads();                                            // before the next column chunk overwrites the totals
  };
  for (int cb = 0; cb < a.d; cb += LPR * 4) {
    const int c0 = cb + li * 4;
    scan_segment<REV>(a, start, end, s, NSLOT, c0, c0 < a.d, exchange);
  }
}

constexpr int kUnroll = 8;

struct CollectEpi {
  const float* s;         // per output row, or NULL
  const float* r_self;    // per output row: the scale of the row's own x, or NULL (no self term)
  int width;              // columns that carry the epilogue (the mask index is row * width + column); the rest are written as zeros
  RowEpi row;
};

template <int LPR>
__global__ __launch_bounds__(kBlock) void scan_collect_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ t, int64_t ldt,
    const float* __restrict__ x, int64_t ldx, float* __restrict__ y, int64_t ldy, int n_t, int d, CollectEpi e,
    const uint64_t* __restrict__ seed_base) {
  constexpr int NS = kWave / LPR;
  const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int row = static_cast<int>(blk) * kWavesPerBlock + (threadIdx.x >> 6);
  if (row >= n_t) return;                                       // whole wave exits together
  e.row.seed = resolve_seed(seed_base, e.row.seed);
  const int lane = lane_id();
  const int slot = lane / LPR, li = lane % LPR;
  const int start = rowptr[row], end = rowptr[row + 1];
  const float sc = e.s ? e.s[row] : 1.f;
  const float rs = e.r_self ? e.r_self[row] : 0.f;

  for (int cb = 0; cb < d; cb += LPR * 4) {
    const int c0 = cb + li * 4;
    const bool active = c0 < d;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int base = start; base < end; base += kWave) {
      const int n = min(kWave, end - base);
      const int my_col = lane < n ? col[base + lane] : 0;
      for (int j = 0; j < n; j += NS * kUnroll) {
        Raw<float, 4> raw[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const int jj = j + u * NS + slot;
          const int src = __shfl(my_col, jj & (kWave - 1));
          if (jj < n && active) raw[u] = load_raw<float, 4>(t + static_cast<int64_t>(src) * ldt + c0);
          else raw[u] = zero_raw<float, 4>();
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const FVec<4> f = unpack<float, 4>(raw[u]);
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] += f.v[k];
        }
      }
    }
#pragma unroll
    for (int off = LPR; off < kWave; off <<= 1)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] += __shfl_xor(acc[k], off);

    if (slot == 0 && active) {
      if (rs != 0.f) {                                          // (a vertex without a loop never touches its x)
        const FVec<4> own = load_vec<float, 4>(x + static_cast<int64_t>(row) * ldx + c0);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = fmaf(rs, own.v[k], acc[k]);
      }
      FVec<4> o;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = c0 + k;
        o.v[k] = c < e.width
                     ? row_epilogue<true>(e.row, acc[k] * sc, c, [=] { return static_cast<int64_t>(row) * e.width + c; })
                     : 0.f;
      }
      store_vec<float, 4>(y + static_cast<int64_t>(row) * ldy + c0, o);
    }
  }
}

}  // namespace scan
}  // namespace allset

using namespace allset;
using namespace allset::scan;

extern "C" int allset_scan_rows_supported(int64_t d) { return d > 0 && d % 4 == 0 && d <= kLooMaxD; }

extern "C" int allset_scan_rows(const int32_t* rowptr, const int32_t* col, const float* src, int64_t lds, const float* s_src, float* out,
                                int64_t ldo, const int32_t* long_seg, int64_t n_long, int reverse, int64_t n_seg, int64_t n_src,
                                int64_t nnz, int64_t d, void* stream) {
  clear_error();
  ALLSET_REQUIRE(n_seg >= 0 && n_src >= 0 && nnz >= 0 && d >= 0, "scan_rows: negative size");
  ALLSET_REQUIRE(n_seg < INT32_MAX && n_src < INT32_MAX && nnz < INT32_MAX, "scan_rows: size exceeds int32");
  ALLSET_REQUIRE(reverse == 0 || reverse == 1, "scan_rows: reverse must be 0 or 1, got %d", reverse);
  if (n_seg == 0 || nnz == 0 || d == 0) return ALLSET_OK;
  if (!allset_scan_rows_supported(d)) {
    set_error("scan_rows: width %lld is not built (d %% 4 == 0, d <= %d)", static_cast<long long>(d), kLooMaxD);
    return ALLSET_ERR_UNSUPPORTED;
  }
  ALLSET_REQUIRE(rowptr && src && out, "scan_rows: null rowptr/src/out");
  ALLSET_REQUIRE(n_src > 0, "scan_rows: an empty source table with nnz > 0");
  ALLSET_REQUIRE(col != nullptr || n_src >= nnz, "scan_rows: null col (contiguous rows) needs n_src >= nnz");
  ALLSET_REQUIRE(lds >= d && ldo >= d, "scan_rows: leading dimension smaller than d");
  ALLSET_REQUIRE(lds % 4 == 0 && ldo % 4 == 0 && aligned16(src) && aligned16(out), "scan_rows: rows must be 16-byte aligned");
  ALLSET_REQUIRE(static_cast<const void*>(src) != static_cast<const void*>(out), "scan_rows: out may not alias src");
  ALLSET_REQUIRE(n_long <= n_seg, "scan_rows: n_long exceeds n_seg");
  ALLSET_REQUIRE(n_long <= 0 || long_seg != nullptr, "scan_rows: null long_seg with n_long > 0");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const LooArgs a{rowptr, col, src, lds, s_src, nullptr, out, ldo, static_cast<int>(d)};
  const int ns = static_cast<int>(n_seg);
  // n_long as for allset_loo_rows: < 0 unknown (one workgroup per segment looks), 0 none (one wave each), > 0 the list
  const unsigned wave_grid = static_cast<unsigned>((n_seg + kWavesPerBlock - 1) / kWavesPerBlock);
  const unsigned block_grid = n_long < 0 ? static_cast<unsigned>(n_seg) : static_cast<unsigned>(n_long);
  const int32_t* list = n_long > 0 ? long_seg : nullptr;
  const int skip_long = n_long != 0;
#define ALLSET_SCAN(LPR_, REV_)                                                                               \
  do {                                                                                                        \
    scan_wave_kernel<LPR_, REV_><<<wave_grid, kBlock, 0, st>>>(a, ns, skip_long);                             \
    if (block_grid > 0) scan_block_kernel<LPR_, REV_><<<block_grid, kLooBlock, 0, st>>>(a, list, ns);         \
  } while (0)
#define ALLSET_SCAN_DIR(LPR_)                 \
  do {                                        \
    if (reverse) ALLSET_SCAN(LPR_, true);     \
    else ALLSET_SCAN(LPR_, false);            \
  } while (0)
  switch (loo_lpr(d)) {
    case 8:  ALLSET_SCAN_DIR(8); break;
    case 16: ALLSET_SCAN_DIR(16); break;
    case 32: ALLSET_SCAN_DIR(32); break;
    default: ALLSET_SCAN_DIR(64); break;
  }
#undef ALLSET_SCAN_DIR
#undef ALLSET_SCAN
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_scan_collect(const int32_t* rowptr, const int32_t* col, const float* t, int64_t ldt, const float* r_self,
                                   const float* x, int64_t ldx, const float* s, const float* bias, int act, float p, uint64_t seed,
                                   const uint64_t* seed_base, float* y, int64_t ldy, int64_t n_t, int64_t n_pos, int64_t d,
                                   int64_t width, void* stream) {
  clear_error();
  ALLSET_REQUIRE(act >= kActNone && act <= kActElu, "scan_collect: bad act %d", act);
  ALLSET_REQUIRE(p >= 0.f && p < 1.f, "scan_collect: dropout p must be in [0,1)");
  ALLSET_REQUIRE(n_t >= 0 && n_pos >= 0 && d >= 0, "scan_collect: negative size");
  ALLSET_REQUIRE(n_t < INT32_MAX && n_pos < INT32_MAX, "scan_collect: size exceeds int32");
  if (n_t == 0 || d == 0) return ALLSET_OK;
  if (!allset_scan_rows_supported(d)) {
    set_error("scan_collect: width %lld is not built (d %% 4 == 0, d <= %d)", static_cast<long long>(d), kLooMaxD);
    return ALLSET_ERR_UNSUPPORTED;
  }
  ALLSET_REQUIRE(width > d - 4 && width <= d, "scan_collect: width %lld outside (d - 4, d]", static_cast<long long>(width));
  ALLSET_REQUIRE(rowptr && y, "scan_collect: null rowptr/y");
  ALLSET_REQUIRE(n_pos == 0 || (col && t), "scan_collect: null col/t with rows to collect");
  ALLSET_REQUIRE(r_self == nullptr || x != nullptr, "scan_collect: r_self without x");
  ALLSET_REQUIRE(ldy >= d && ldy % 4 == 0 && aligned16(y), "scan_collect: y rows must be 16-byte aligned, ldy >= d");
  ALLSET_REQUIRE(t == nullptr || (ldt >= d && ldt % 4 == 0 && aligned16(t)), "scan_collect: t rows must be 16-byte aligned, ldt >= d");
  ALLSET_REQUIRE(x == nullptr || (ldx >= d && ldx % 4 == 0 && aligned16(x)), "scan_collect: x rows must be 16-byte aligned, ldx >= d");
  ALLSET_REQUIRE(static_cast<const void*>(y) != static_cast<const void*>(t) && static_cast<const void*>(y) != static_cast<const void*>(x),
                 "scan_collect: y may alias neither t nor x");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const CollectEpi e{s, r_self, static_cast<int>(width), row_epi(bias, act, p, seed)};
  const unsigned grid = row_grid(n_t);
  const int nt = static_cast<int>(n_t), di = static_cast<int>(d);
  switch (loo_lpr(d)) {
    case 8:  scan_collect_kernel<8><<<grid, kBlock, 0, st>>>(rowptr, col, t, ldt, x, ldx, y, ldy, nt, di, e, seed_base); break;
    case 16: scan_collect_kernel<16><<<grid, kBlock, 0, st>>>(rowptr, col, t, ldt, x, ldx, y, ldy, nt, di, e, seed_base); break;
    case 32: scan_collect_kernel<32><<<grid, kBlock, 0, st>>>(rowptr, col, t, ldt, x, ldx, y, ldy, nt, di, e, seed_base); break;
    default: scan_collect_kernel<64><<<grid, kBlock, 0, st>>>(rowptr, col, t, ldt, x, ldx, y, ldy, nt, di, e, seed_base); break;
  }
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}
