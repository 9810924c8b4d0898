// Metapath reachability (dgl.metapath_reachable_graph of the reference's `main.py --hetero`) for gfx950: C = pattern(A B), a boolean
// sparse matrix product.  A [n_a, n_b] and B [n_b, n_c] are int32 CSR (duplicate entries allowed, they count once); C is int32 CSR
// whose columns are strictly increasing inside every row, so the result is unique: the insertion order inside a kernel cannot show.
//
// count pass -> (the caller scans the row counts and reads nnz_c: the one host sync) -> fill pass.  Nothing global is proportional to
// the candidate count sum_i sum_{k in A[i,:]} deg_B(k): a row's distinct-column set lives in LDS.
//
//   bin_kernel     one thread per row of A: cand_i = sum_{k in A[i,:]} deg_B(k) (int64, an upper bound of the row's result), and the
//                  row appended to the list of its bin (wave-aggregated atomic counters: the ORDER of a list is arbitrary, every
//                  row's result and position are not).  cand_i = 0: the count is written here.
//   hash_kernel    <16 lanes, 64 slots>:   cand <= 32, sixteen rows per workgroup (four per wavefront);
//                  <64 lanes, 1024 slots>: cand <= 512, one wavefront per row.
//                  Open addressing with LDS compare-and-swap, linear probing.  The bin bound is half the table, so a table can never
//                  fill: a row that could overflow one is in the next bin BY CONSTRUCTION and nothing is ever truncated.  Fill: the
//                  table is rebuilt, (compacted for the 1024-slot table,) and every entry written at its rank -- the number of
//                  smaller entries (broadcast LDS reads) -- which is the in-LDS sort.
//   bitmap_kernel  cand > 512: one workgroup per row, a 32 KiB LDS bitmap over a window of 262144 columns, one pass per window
//                  (n_c <= 262144: one pass; beyond, the row's candidates are re-read per window -- exact for any n_c, no global
//                  workspace).  Rows of A with >= 256 entries give every thread its own entries (short B rows: a field's papers);
//                  shorter ones put the whole workgroup on each B row (a hub's 3000 neighbours).  Counting is a popcount, the fill
//                  a block scan of per-thread popcounts and an in-order emission: sorted for free.
// All three are persistent: a fixed grid strides over its bin's list, whose length it reads from the workspace (the host never
// learns it).  LDS: 4 KiB / 24 KiB / 33 KiB per workgroup, so at least four workgroups stay resident per CU (160 KiB) on every path.
// Ids are trusted to be in range (han_hetero.HeteroGraph checks them); an id outside [0, n_b) / [0, n_c) is skipped, never dereferenced.
//
// Workspace (bytes): 16 (three list lengths) + 3 * 4 n_a (the lists) -- O(n_a).  The fill pass reads what the count pass left there.
#include <limits.h>

#include "common.h"

namespace allset {
namespace metapath {

constexpr int kCand16 = 32, kTab16 = 64;
constexpr int kCand64 = 512, kTab64 = 1024;
constexpr int kBitWords = 8192;                      // 32 KiB of LDS
constexpr int64_t kBitCols = static_cast<int64_t>(kBitWords) * 32;
constexpr int kWideRow = kBlock;                     // entries of an A row from which every thread takes its own
constexpr int kEmpty = INT_MAX;                      // (n_c <= INT_MAX, so no column equals it)
constexpr int kMaxGrid = 2048;

__device__ __forceinline__ int append(int* counter, bool mine) {
  const unsigned long long mask = __ballot(mine);
  if (mask == 0ull) return 0;
  const int lane = lane_id();
  const int leader = __ffsll(static_cast<long long>(mask)) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(counter, __popcll(mask));
  base = __shfl(base, leader);
  return base + __popcll(mask & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(kBlock) void bin_kernel(const int32_t* __restrict__ rowptrA, const int32_t* __restrict__ colA,
                                                     const int32_t* __restrict__ rowptrB, int n_a, int n_b, int* __restrict__ hdr,
                                                     int* __restrict__ list16, int* __restrict__ list64, int* __restrict__ listB,
                                                     int32_t* __restrict__ cnt) {
  const int i = static_cast<int>(blockIdx.x) * kBlock + threadIdx.x;
  int64_t cand = -1;
  if (i < n_a) {
    cand = 0;
    for (int k = rowptrA[i]; k < rowptrA[i + 1]; ++k) {
      const int j = colA[k];
      if (static_cast<unsigned>(j) < static_cast<unsigned>(n_b)) cand += rowptrB[j + 1] - rowptrB[j];
    }
    if (cand == 0) cnt[i] = 0;
  }
  const bool s = cand > 0 && cand <= kCand16, m = cand > kCand16 && cand <= kCand64, b = cand > kCand64;
  const int ps = append(hdr + 0, s), pm = append(hdr + 1, m), pb = append(hdr + 2, b);
  if (s) list16[ps] = i;
  if (m) list64[pm] = i;
  if (b) listB[pb] = i;
}

template <int TAB>
__device__ __forceinline__ int insert(int* tab, int v) {     // 1 when v is new
  unsigned slot = (static_cast<unsigned>(v) * 0x9E3779B1u) >> (32 - __builtin_ctz(TAB));
  for (int probe = 0; probe < TAB; ++probe) {                // (bounded: the bin keeps the table at most half full)
    const int old = atomicCAS(&tab[slot], kEmpty, v);
    if (old == kEmpty) return 1;
    if (old == v) return 0;
    slot = (slot + 1) & (TAB - 1);
  }
  return 0;
}

template <int LANES, int TAB, bool FILL>
__global__ __launch_bounds__(kBlock) void hash_kernel(const int32_t* __restrict__ rowptrA, const int32_t* __restrict__ colA,
                                                      const int32_t* __restrict__ rowptrB, const int32_t* __restrict__ colB, int n_b,
                                                      int n_c, const int* __restrict__ n_rows, const int* __restrict__ list,
                                                      int32_t* __restrict__ cnt, const int32_t* __restrict__ rowptrC,
                                                      int32_t* __restrict__ colC) {
  constexpr int GPB = kBlock / LANES;                        // rows per workgroup; a group never straddles a wavefront
  constexpr int DENSE = (FILL && LANES == kWave) ? TAB / 2 : 1;
  __shared__ int tab[GPB][TAB];
  __shared__ int dense[GPB][DENSE];
  const int grp = threadIdx.x / LANES, li = threadIdx.x % LANES;
  const int total = *n_rows;
  int* t = tab[grp];
  for (int r0 = static_cast<int>(blockIdx.x) * GPB; r0 < total; r0 += static_cast<int>(gridDim.x) * GPB) {   // (uniform per workgroup)
    const bool live = r0 + grp < total;
    const int row = live ? list[r0 + grp] : 0;
    for (int s = li; s < TAB; s += LANES) t[s] = kEmpty;
    __syncthreads();
    int mine = 0;
    if (live) {
      for (int k = rowptrA[row]; k < rowptrA[row + 1]; ++k) {
        const int j = colA[k];
        if (static_cast<unsigned>(j) >= static_cast<unsigned>(n_b)) continue;
        for (int q = rowptrB[j] + li; q < rowptrB[j + 1]; q += LANES) {
          const int c = colB[q];
          if (static_cast<unsigned>(c) < static_cast<unsigned>(n_c)) mine += insert<TAB>(t, c);
        }
      }
    }
    __syncthreads();
    if constexpr (!FILL) {
#pragma unroll
      for (int off = 1; off < LANES; off <<= 1) mine += __shfl_xor(mine, off);
      if (live && li == 0) cnt[row] = mine;
    } else if constexpr (LANES == kWave) {
      // compact the table (ballot prefix, the whole wavefront is one group), then rank within the compact list
      int n = 0;
      for (int s0 = 0; s0 < TAB; s0 += kWave) {
        const int v = t[s0 + li];
        const unsigned long long mask = __ballot(v != kEmpty);
        if (v != kEmpty) dense[grp][n + __popcll(mask & ((1ull << li) - 1ull))] = v;
        n += __popcll(mask);
      }
      __syncthreads();
      if (live) {
        int32_t* out = colC + rowptrC[row];
        for (int s = li; s < n; s += kWave) {
          const int v = dense[grp][s];
          int rank = 0;
          for (int u = 0; u < n; ++u) rank += dense[grp][u] < v;
          out[rank] = v;
        }
      }
    } else {
      if (live) {
        int32_t* out = colC + rowptrC[row];
        for (int s = li; s < TAB; s += LANES) {
          const int v = t[s];
          if (v == kEmpty) continue;
          int rank = 0;
          for (int u = 0; u < TAB; ++u) rank += t[u] < v;      // (kEmpty is larger than every column)
          out[rank] = v;
        }
      }
    }
    __syncthreads();
  }
}

template <bool FILL>
__global__ __launch_bounds__(kBlock) void bitmap_kernel(const int32_t* __restrict__ rowptrA, const int32_t* __restrict__ colA,
                                                        const int32_t* __restrict__ rowptrB, const int32_t* __restrict__ colB, int n_b,
                                                        int n_c, const int* __restrict__ n_rows, const int* __restrict__ list,
                                                        int32_t* __restrict__ cnt, const int32_t* __restrict__ rowptrC,
                                                        int32_t* __restrict__ colC) {
  __shared__ unsigned bits[kBitWords];
  __shared__ int wsum[kWavesPerBlock];
  const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  const int total = *n_rows;
  for (int r = blockIdx.x; r < total; r += gridDim.x) {
    const int row = list[r];
    const int a0 = rowptrA[row], a1 = rowptrA[row + 1];
    int found = 0;                                           // (uniform) columns found in the windows before this one
    for (int64_t base = 0; base < n_c; base += kBitCols) {
      const int words = static_cast<int>((min(kBitCols, static_cast<int64_t>(n_c) - base) + 31) / 32);
      for (int w = tid; w < words; w += kBlock) bits[w] = 0u;
      __syncthreads();
      auto mark = [&](int c) {
        const int64_t rel = static_cast<int64_t>(c) - base;
        if (static_cast<unsigned>(c) < static_cast<unsigned>(n_c) && rel >= 0 && rel < kBitCols)
          atomicOr(&bits[rel >> 5], 1u << (rel & 31));
      };
      if (a1 - a0 >= kWideRow) {
        for (int k = a0 + tid; k < a1; k += kBlock) {
          const int j = colA[k];
          if (static_cast<unsigned>(j) >= static_cast<unsigned>(n_b)) continue;
          for (int q = rowptrB[j]; q < rowptrB[j + 1]; ++q) mark(colB[q]);
        }
      } else {
        for (int k = a0; k < a1; ++k) {
          const int j = colA[k];
          if (static_cast<unsigned>(j) >= static_cast<unsigned>(n_b)) continue;
          for (int q = rowptrB[j] + tid; q < rowptrB[j + 1]; q += kBlock) mark(colB[q]);
        }
      }
      __syncthreads();
      // every thread owns a contiguous run of words: popcount, scan over the workgroup, emit in order
      const int per = (words + kBlock - 1) / kBlock;
      const int w0 = min(tid * per, words), w1 = min(w0 + per, words);
      int c = 0;
      for (int w = w0; w < w1; ++w) c += __popc(bits[w]);
      int inc = c;
#pragma unroll
      for (int off = 1; off < kWave; off <<= 1) {
        const int o = __shfl_up(inc, off);
        if (lane >= off) inc += o;
      }
      if (lane == kWave - 1) wsum[wave] = inc;
      __syncthreads();
      int before = 0, all = 0;
#pragma unroll
      for (int w = 0; w < kWavesPerBlock; ++w) {
        if (w < wave) before += wsum[w];
        all += wsum[w];
      }
      if constexpr (FILL) {
        int32_t* out = colC + rowptrC[row] + found + before + inc - c;
        for (int w = w0; w < w1; ++w) {
          unsigned m = bits[w];
          while (m) {
            *out++ = static_cast<int32_t>(base + static_cast<int64_t>(w) * 32 + (__ffs(m) - 1));
            m &= m - 1u;
          }
        }
      }
      found += all;
      __syncthreads();
    }
    if constexpr (!FILL) {
      if (tid == 0) cnt[row] = found;
    }
  }
}

struct Workspace {
  int* hdr;
  int* list16;
  int* list64;
  int* listB;
};

static inline size_t workspace_bytes(int64_t n_a) { return 16 + 3 * sizeof(int) * static_cast<size_t>(n_a); }

static inline Workspace carve(void* ws, int64_t n_a) {
  Workspace w;
  w.hdr = static_cast<int*>(ws);
  w.list16 = w.hdr + 4;
  w.list64 = w.list16 + n_a;
  w.listB = w.list64 + n_a;
  return w;
}

static inline unsigned grid_for(int64_t rows, int per_block) {
  const int64_t g = (rows + per_block - 1) / per_block;
  return static_cast<unsigned>(g < kMaxGrid ? (g > 0 ? g : 1) : kMaxGrid);
}

static int check_args(const char* who, const void* rowptrA, const void* colA, const void* rowptrB, const void* colB, int64_t n_a,
                      int64_t n_b, int64_t n_c, const void* ws, size_t ws_bytes) {
  ALLSET_REQUIRE(n_a >= 0 && n_b >= 0 && n_c >= 0, "%s: negative size", who);
  ALLSET_REQUIRE(n_a < INT32_MAX && n_b < INT32_MAX, "%s: n_a = %lld / n_b = %lld rows exceed int32", who, static_cast<long long>(n_a),
                 static_cast<long long>(n_b));
  ALLSET_REQUIRE(n_c <= INT32_MAX, "%s: n_c = %lld columns exceed int32 (the result's column ids are int32)", who,
                 static_cast<long long>(n_c));
  if (n_a == 0) return ALLSET_OK;
  ALLSET_REQUIRE(rowptrA && rowptrB, "%s: null rowptr", who);
  (void)colA;
  (void)colB;
  ALLSET_REQUIRE(ws != nullptr && ws_bytes >= workspace_bytes(n_a), "%s: workspace of %zu bytes, %zu needed", who, ws_bytes,
                 workspace_bytes(n_a));
  ALLSET_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3u) == 0, "%s: workspace must be 4-byte aligned", who);
  return ALLSET_OK;
}

}  // namespace metapath
}  // namespace allset

using namespace allset;
using namespace allset::metapath;

extern "C" int allset_spgemm_bool_bins(int64_t* bins) {
  clear_error();
  ALLSET_REQUIRE(bins != nullptr, "spgemm_bool_bins: null pointer");
  bins[0] = kCand16;
  bins[1] = kCand64;
  bins[2] = kBitCols;
  bins[3] = kWideRow;
  return ALLSET_OK;
}

extern "C" int allset_spgemm_bool_workspace_bytes(int64_t n_a, size_t* bytes) {
  clear_error();
  ALLSET_REQUIRE(bytes != nullptr, "spgemm_bool_workspace_bytes: null pointer");
  ALLSET_REQUIRE(n_a >= 0 && n_a < INT32_MAX, "spgemm_bool_workspace_bytes: n_a = %lld outside int32", static_cast<long long>(n_a));
  *bytes = workspace_bytes(n_a);
  return ALLSET_OK;
}

extern "C" int allset_spgemm_bool_count(const int32_t* rowptrA, const int32_t* colA, const int32_t* rowptrB, const int32_t* colB,
                                        int64_t n_a, int64_t n_b, int64_t n_c, int32_t* cnt, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  clear_error();
  int rc = check_args("spgemm_bool_count", rowptrA, colA, rowptrB, colB, n_a, n_b, n_c, workspace, workspace_bytes);
  if (rc != ALLSET_OK || n_a == 0) return rc;
  ALLSET_REQUIRE(cnt != nullptr, "spgemm_bool_count: null cnt");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const Workspace w = carve(workspace, n_a);
  ALLSET_HIP_CHECK(hipMemsetAsync(w.hdr, 0, 16, st));
  const int na = static_cast<int>(n_a), nb = static_cast<int>(n_b), nc = static_cast<int>(n_c);
  bin_kernel<<<static_cast<unsigned>((n_a + kBlock - 1) / kBlock), kBlock, 0, st>>>(rowptrA, colA, rowptrB, na, nb, w.hdr, w.list16,
                                                                                    w.list64, w.listB, cnt);
  hash_kernel<16, kTab16, false><<<grid_for(n_a, kBlock / 16), kBlock, 0, st>>>(rowptrA, colA, rowptrB, colB, nb, nc, w.hdr + 0, w.list16,
                                                                               cnt, nullptr, nullptr);
  hash_kernel<kWave, kTab64, false><<<grid_for(n_a, kWavesPerBlock), kBlock, 0, st>>>(rowptrA, colA, rowptrB, colB, nb, nc, w.hdr + 1,
                                                                                      w.list64, cnt, nullptr, nullptr);
  bitmap_kernel<false><<<grid_for(n_a, 1), kBlock, 0, st>>>(rowptrA, colA, rowptrB, colB, nb, nc, w.hdr + 2, w.listB, cnt, nullptr,
                                                           nullptr);
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_spgemm_bool_fill(const int32_t* rowptrA, const int32_t* colA, const int32_t* rowptrB, const int32_t* colB,
                                       int64_t n_a, int64_t n_b, int64_t n_c, const int32_t* rowptrC, int64_t nnz_c, int32_t* colC,
                                       const void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  ALLSET_REQUIRE(nnz_c >= 0, "spgemm_bool_fill: negative nnz_c");
  ALLSET_REQUIRE(nnz_c <= INT32_MAX, "spgemm_bool_fill: the result has %lld entries, more than an int32 rowptr can index (%d)",
                 static_cast<long long>(nnz_c), INT32_MAX);
  int rc = check_args("spgemm_bool_fill", rowptrA, colA, rowptrB, colB, n_a, n_b, n_c, workspace, workspace_bytes);
  if (rc != ALLSET_OK || n_a == 0 || nnz_c == 0) return rc;
  ALLSET_REQUIRE(rowptrC && colC, "spgemm_bool_fill: null rowptrC / colC");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const Workspace w = carve(const_cast<void*>(workspace), n_a);
  const int nb = static_cast<int>(n_b), nc = static_cast<int>(n_c);
  hash_kernel<16, kTab16, true><<<grid_for(n_a, kBlock / 16), kBlock, 0, st>>>(rowptrA, colA, rowptrB, colB, nb, nc, w.hdr + 0, w.list16,
                                                                              nullptr, rowptrC, colC);
  hash_kernel<kWave, kTab64, true><<<grid_for(n_a, kWavesPerBlock), kBlock, 0, st>>>(rowptrA, colA, rowptrB, colB, nb, nc, w.hdr + 1,
                                                                                     w.list64, nullptr, rowptrC, colC);
  bitmap_kernel<true><<<grid_for(n_a, 1), kBlock, 0, st>>>(rowptrA, colA, rowptrB, colB, nb, nc, w.hdr + 2, w.listB, nullptr, rowptrC, colC);
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}
