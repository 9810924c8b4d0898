// Mini-batch HAN (reference DGL_HAN/train_sampling.py: HANSampler over DGL's RandomWalkNeighborSampler, then dgl.to_block) for
// gfx950: the metapath random walk, the per-seed neighbour rows, the block's local relabelling, and the bipartite entry points of
// the attention hop.
//
// ---- the walk ----------------------------------------------------------------------------------------------------------------
// Nodes are the "appended" id space n = n_v + n_e (vertices, then hyperedges).  A metapath is two hops over the BINARISED incidence:
// CSR A (n_a rows -> ids of the other kind) then CSR B (back).  VEV: A = vertex -> hyperedges, B = hyperedge -> vertices, id_base 0;
// EVE: A = hyperedge -> vertices, B = vertex -> hyperedges, id_base n_v.  A seed outside [id_base, id_base + n_a) or with an empty
// row has no out-edge: the walk terminates and its endpoint is -1 (DGL writes -1 too).  Such a seed is never dereferenced.
//   one lane per (seed, walk): four dependent loads (rowptrA, colA, rowptrB, colB) per lane and nothing else -- a pointer chase
//   whose only lever is how many chases are in flight.  B * k lanes is 640 at the reference's defaults and 20 480 at B = 1024,
//   k = 20: far fewer than the machine holds, so every walk gets its own lane, blocks of 4 waves spread over the CUs, and the
//   cost is ONE chain latency (4 misses) whatever B is.  Rows are tiny (a hyperedge has a few members), so there is nothing to
//   coalesce or stage in LDS.
// Random numbers are counter-based, two rounds of common.h's pair_hash:
//   key = (counter * golden + seed) ^ (metapath + 1) * odd constant;   ctr = ((GLOBAL seed-node id) * 64 + walk) * 2 + hop
//   u32 = pair_hash(swap32(key), pair_hash(key, ctr))                   (the second round is a bijection of the first's 32 bits)
// keyed on the seed NODE, not on its position in the batch: a node's walks are the same whatever batch it is in.
// The uniform pick is multiply-shift, index = (u32 * degree) >> 32: every index is taken by floor(2^32 / degree) or one more of the
// 2^32 values, so its probability is within degree / 2^32 (relative) of 1 / degree -- 2.4e-7 for a row of 1000.
//
// ---- the typed walk ----------------------------------------------------------------------------------------------------------
// A typed graph's metapath is a chain of L <= kMaxHops relation CSRs (rows = source ids of the hop's source type, int32 columns =
// ids of its destination type, duplicate edges kept: a duplicated edge is twice as likely, DGL's multigraph walk).  Same mapping:
// one lane per (seed, walk), 2 L dependent loads.  The relation table (rowptr, col, n_rows per hop) is wave-uniform and travels by
// value as a kernel argument; the hop loop is unrolled over kMaxHops so that every table access has a constant offset (scalar
// loads, no scratch).  An id is range-checked against the hop's n_rows BEFORE it indexes that hop's rowptr: a seed outside
// [0, n_rows[0]), an empty row, or an intermediate id outside the next hop's rows ends the walk with -1 and reads nothing further.
// Random numbers: hop h of a walk draws walk_hash(key ^ (h >> 1) * odd constant, seed node, walk, h & 1).  For h < 2 that IS the
// two-hop walk's draw, so L = 2 over the same CSRs is bit-identical to allset_han_walk with id_base 0; hops 2 j and 2 j + 1 differ in
// the counter and hop pairs j != j' in the key, so the hops of one walk draw independently even where a metapath repeats a
// relation.  The key is still the seed NODE, never its position in the batch nor the node the walk currently stands on.
//
// ---- block rows --------------------------------------------------------------------------------------------------------------
// One wave per seed, one lane per walk (k <= 64): drop -1 and the seed itself, keep the first lane of every distinct endpoint, rank
// the survivors by global id (two 64-step shuffle passes, no LDS), write them ascending into row b of a B x (k + 1) slab, then the
// seed itself (the ONE self-loop) and -1 padding.  `extra` is the same slab with every seed-set member and the padding replaced by
// INT32_MAX: sorted and uniqued it lists the block's non-seed source nodes.
//
// ---- compaction / relabelling ------------------------------------------------------------------------------------------------
// One lane per slab entry: the block-local source id of a global id is its position in the seed list (binary search in the sorted
// seeds, then the sort's permutation) or B + its rank among the sorted distinct non-seed nodes; written at rowptr[b] + i of the
// target-major CSR together with the target b.  The row pointer is a prefix sum of the counts.
//
// ---- device-resident step counter ---------------------------------------------------------------------------------------------
// allset_han_walk_dc / allset_han_walk_typed_dc are the two walks with the step counter read from device memory: the key is formed in
// the kernel from *counter + counter_add (64-bit wrap) by the same walk_key() the host entries use, so equal effective counters give
// bit-identical endpoints and a captured graph whose counter another node advances draws new walks at every replay.
//
// ---- fixed-capacity block (no read-back) ---------------------------------------------------------------------------------------
// The block's arrays are sized by the slab, cap = B (k + 1) -- at most k + 1 slots per target and at most B k distinct non-seed
// nodes, so nothing can overflow -- and the real sizes {nnz, n_extra} stay on the device in `sizes`.
//   relabel:  ONE workgroup of kScanBlock lanes loops over chunks of kScanBlock entries, carrying the running total in a register:
//             the row pointer (prefix sum of the counts), then the distinct entries of the SORTED extra slab compacted to the front
//             of `uniq` (first-occurrence flags, their prefix sum), the tail filled with INT32_MAX, the two sizes, and the
//             duplicate-seed flag (equal neighbours in the sorted seeds) stored into a sticky status word.  No workgroup waits on
//             another: there is only one.  cap <= kMaxFixedSlab keeps the loop to 256 chunks.
//   compact:  block_compact_kernel's relabelling with nnz / n_extra read from `sizes`; lane t also writes padding slot t (t >= nnz:
//             col = dst = 0, sort key = cap), source id t (seeds, then uniq, then the first seed) -- every slot of every array is
//             written by exactly one lane.  The sort key of a real slot is its local source id (< cap).
//   transpose: from the stably sorted keys and their permutation, one lane per source row: rowptrT[j] = the first sorted position
//             whose key is >= j (j = 0 .. cap; the padding's key cap puts nnz into every row pointer past the real rows), colT =
//             dst[perm], slotT = perm, 0 for padding.
//
// ---- bipartite hop -----------------------------------------------------------------------------------------------------------
// han.hip's hop kernels already index sources (x, el: through col) and targets (er, y, lse: by row) separately; only their entry
// points tied the two row counts together.  allset_han_block_hop_* check the bipartite shapes and launch the same instantiations
// through the existing entry points: forward and stats over n_dst target rows, the source pass over n_src source rows.
#include <limits.h>

#include "common.h"

namespace allset {
namespace han_sample {

constexpr int kMaxWalks = 64;
constexpr int kMaxHeads = 64;
constexpr int kMaxWidth = 512;

__device__ __forceinline__ uint32_t walk_hash(uint64_t key, uint32_t node, uint32_t walk, uint32_t hop) {
  const int64_t ctr = (static_cast<int64_t>(node) * kMaxWalks + walk) * 2 + hop;
  const uint32_t h = pair_hash(key, ctr);
  return pair_hash((key >> 32) | (key << 32), static_cast<int64_t>(h));
}

__device__ __forceinline__ int uniform_pick(uint32_t h, int deg) {
  return static_cast<int>((static_cast<uint64_t>(h) * static_cast<uint32_t>(deg)) >> 32);
}

// the key of one (seed, step counter, metapath): host entries and the device-counter kernels form it with this one function
__host__ __device__ __forceinline__ uint64_t walk_key(uint64_t counter, uint64_t seed, int metapath) {
  return (counter * 0x9E3779B97F4A7C15ULL + seed) ^ (static_cast<uint64_t>(metapath + 1) * 0xD1B54A32D192ED03ULL);
}

__device__ __forceinline__ void walk_body(const int32_t* __restrict__ rpa, const int32_t* __restrict__ ca,
                                          const int32_t* __restrict__ rpb, const int32_t* __restrict__ cb, int n_a, int n_b, int id_base,
                                          const int32_t* __restrict__ seeds, int B, int k, uint64_t key, int32_t* __restrict__ out) {
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (tid >= static_cast<int64_t>(B) * k) return;
  const int b = static_cast<int>(tid / k), w = static_cast<int>(tid % k);
  const int s = seeds[b];
  const int64_t loc = static_cast<int64_t>(s) - id_base;
  int r = -1;
  if (loc >= 0 && loc < n_a) {
    const int a0 = rpa[loc], a1 = rpa[loc + 1];
    if (a1 > a0) {
      const int mid = ca[a0 + uniform_pick(walk_hash(key, static_cast<uint32_t>(s), w, 0), a1 - a0)];
      if (mid >= 0 && mid < n_b) {
        const int b0 = rpb[mid], b1 = rpb[mid + 1];
        if (b1 > b0) r = cb[b0 + uniform_pick(walk_hash(key, static_cast<uint32_t>(s), w, 1), b1 - b0)] + id_base;
      }
    }
  }
  out[tid] = r;
}

__global__ __launch_bounds__(kBlock) void walk_kernel(
    const int32_t* __restrict__ rpa, const int32_t* __restrict__ ca, const int32_t* __restrict__ rpb, const int32_t* __restrict__ cb,
    int n_a, int n_b, int id_base, const int32_t* __restrict__ seeds, int B, int k, uint64_t key, int32_t* __restrict__ out) {
  walk_body(rpa, ca, rpb, cb, n_a, n_b, id_base, seeds, B, k, key, out);
}

__global__ __launch_bounds__(kBlock) void walk_dc_kernel(
    const int32_t* __restrict__ rpa, const int32_t* __restrict__ ca, const int32_t* __restrict__ rpb, const int32_t* __restrict__ cb,
    int n_a, int n_b, int id_base, const int32_t* __restrict__ seeds, int B, int k, const uint64_t* __restrict__ counter,
    uint64_t counter_add, uint64_t seed, int metapath, int32_t* __restrict__ out) {
  walk_body(rpa, ca, rpb, cb, n_a, n_b, id_base, seeds, B, k, walk_key(*counter + counter_add, seed, metapath), out);
}

constexpr int kMaxHops = 8;
constexpr uint64_t kHopPairKey = 0xA0761D6478BD642FULL;

struct HopTable {
  const int32_t* rowptr[kMaxHops];
  const int32_t* col[kMaxHops];  // null only for a relation without edges: nothing is read through it
  int n_rows[kMaxHops];
};

__device__ __forceinline__ void walk_typed_body(const HopTable& t, int L, const int32_t* __restrict__ seeds, int B, int k, uint64_t key,
                                                int32_t* __restrict__ out) {
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (tid >= static_cast<int64_t>(B) * k) return;
  const int b = static_cast<int>(tid / k), w = static_cast<int>(tid % k);
  const int s = seeds[b];
  int cur = s;
#pragma unroll
  for (int h = 0; h < kMaxHops; ++h) {
    if (h < L) {
      int nxt = -1;
      if (cur >= 0 && cur < t.n_rows[h]) {
        const int r0 = t.rowptr[h][cur], r1 = t.rowptr[h][cur + 1];
        if (r1 > r0 && t.col[h] != nullptr) {
          const uint32_t u = walk_hash(key ^ (static_cast<uint64_t>(h >> 1) * kHopPairKey), static_cast<uint32_t>(s), w, h & 1);
          nxt = t.col[h][r0 + uniform_pick(u, r1 - r0)];
        }
      }
      cur = nxt;
    }
  }
  out[tid] = cur;
}

__global__ __launch_bounds__(kBlock) void walk_typed_kernel(const HopTable t, int L, const int32_t* __restrict__ seeds, int B, int k,
                                                            uint64_t key, int32_t* __restrict__ out) {
  walk_typed_body(t, L, seeds, B, k, key, out);
}

__global__ __launch_bounds__(kBlock) void walk_typed_dc_kernel(const HopTable t, int L, const int32_t* __restrict__ seeds, int B, int k,
                                                               const uint64_t* __restrict__ counter, uint64_t counter_add, uint64_t seed,
                                                               int metapath, int32_t* __restrict__ out) {
  walk_typed_body(t, L, seeds, B, k, walk_key(*counter + counter_add, seed, metapath), out);
}

// first index in sorted a[0, n) whose value is >= v
__device__ __forceinline__ int lower_bound(const int32_t* __restrict__ a, int n, int v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kBlock) void block_rows_kernel(
    const int32_t* __restrict__ endpoints, const int32_t* __restrict__ seeds, const int32_t* __restrict__ seeds_sorted, int B, int k,
    int32_t* __restrict__ rows, int32_t* __restrict__ extra, int32_t* __restrict__ counts) {
  const int b = static_cast<int>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  if (b >= B) return;  // whole wave exits together
  const int lane = lane_id();
  const int s = seeds[b];
  const int e = lane < k ? endpoints[static_cast<int64_t>(b) * k + lane] : -1;
  const int valid = (e >= 0 && e != s) ? 1 : 0;
  int first = valid;
  for (int j = 0; j < kWave; ++j) {
    const int ej = __shfl(e, j), vj = __shfl(valid, j);
    if (vj && ej == e && j < lane) first = 0;
  }
  int rank = 0;
  for (int j = 0; j < kWave; ++j) {
    const int ej = __shfl(e, j), fj = __shfl(first, j);
    if (fj && ej < e) ++rank;
  }
  const int cnt = __popcll(__ballot(first));
  const int64_t base = static_cast<int64_t>(b) * (k + 1);
  if (first) {
    rows[base + rank] = e;
    const int pos = lower_bound(seeds_sorted, B, e);
    extra[base + rank] = (pos < B && seeds_sorted[pos] == e) ? INT32_MAX : e;
  }
  for (int p = cnt + lane; p <= k; p += kWave) {
    rows[base + p] = p == cnt ? s : -1;
    extra[base + p] = INT32_MAX;
  }
  if (lane == 0) counts[b] = cnt + 1;
}

__global__ __launch_bounds__(kBlock) void block_compact_kernel(
    const int32_t* __restrict__ rows, const int32_t* __restrict__ counts, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ seeds_sorted, const int32_t* __restrict__ seed_perm, const int32_t* __restrict__ uniq, int n_extra,
    int B, int k, int nnz, int32_t* __restrict__ col, int32_t* __restrict__ dst) {
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (tid >= static_cast<int64_t>(B) * (k + 1)) return;
  const int b = static_cast<int>(tid / (k + 1)), i = static_cast<int>(tid % (k + 1));
  if (i >= counts[b]) return;
  const int slot = rowptr[b] + i;
  if (slot < 0 || slot >= nnz) return;
  const int g = rows[tid];
  const int pos = lower_bound(seeds_sorted, B, g);
  int local;
  if (pos < B && seeds_sorted[pos] == g) {
    local = seed_perm[pos];
  } else {
    const int q = lower_bound(uniq, n_extra, g);
    local = B + (q < n_extra ? q : max(n_extra - 1, 0));
  }
  col[slot] = local;
  dst[slot] = b;
}

// ---- fixed-capacity block --------------------------------------------------------------------------------------------------
constexpr int kScanBlock = 1024;                      // the relabel kernel's ONE workgroup, and the chunk it loops by
constexpr int kScanWaves = kScanBlock / kWave;
constexpr int64_t kMaxFixedSlab = 1 << 18;            // B (k + 1) up to 262 144: B = 4032 at k = 64 (256 chunks)

// Inclusive prefix sum of one int per lane over the workgroup (every lane calls it); `total` = the workgroup's sum.
__device__ __forceinline__ int scan_block(int v, int* __restrict__ wave_tot, int& total) {
  const int lane = lane_id(), wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int o = __shfl_up(v, off);
    if (lane >= off) v += o;
  }
  __syncthreads();                                    // the previous chunk's reads of wave_tot are over
  if (lane == kWave - 1) wave_tot[wave] = v;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kScanWaves; ++w) {
    const int t = wave_tot[w];
    before += w < wave ? t : 0;
    total += t;
  }
  return v + before;
}

__global__ __launch_bounds__(kScanBlock) void block_relabel_kernel(
    const int32_t* __restrict__ counts, const int32_t* __restrict__ flat, const int32_t* __restrict__ seeds_sorted, int B, int k,
    int32_t* __restrict__ rowptr, int32_t* __restrict__ uniq, int32_t* __restrict__ sizes, int32_t* __restrict__ status) {
  __shared__ int wave_tot[kScanWaves];
  const int t = threadIdx.x;
  const int cap = B * (k + 1);
  int nnz = 0;
  if (t == 0) rowptr[0] = 0;
  for (int base = 0; base < B; base += kScanBlock) {             // (uniform trip count: every lane reaches the barriers)
    const int b = base + t;
    const int c = b < B ? min(max(counts[b], 0), k + 1) : 0;
    int total;
    const int inc = scan_block(c, wave_tot, total);
    if (b < B) rowptr[b + 1] = nnz + inc;
    nnz += total;
  }
  int dup = 0;
  for (int b = 1 + t; b < B; b += kScanBlock) dup |= seeds_sorted[b] == seeds_sorted[b - 1] ? 1 : 0;
  if (dup && status != nullptr) *status = 1;                      // sticky: only ever set, every writer stores the same value
  int n_extra = 0;
  for (int base = 0; base < cap; base += kScanBlock) {
    const int i = base + t;
    const int v = i < cap ? flat[i] : INT32_MAX;
    const int first = (v != INT32_MAX && (i == 0 || flat[i - 1] != v)) ? 1 : 0;
    int total;
    const int inc = scan_block(first, wave_tot, total);
    if (first) uniq[n_extra + inc - 1] = v;                       // < cap: there are at most cap flags
    n_extra += total;
  }
  for (int i = n_extra + t; i < cap; i += kScanBlock) uniq[i] = INT32_MAX;
  if (t == 0) {
    sizes[0] = nnz;
    sizes[1] = n_extra;
  }
}

__global__ __launch_bounds__(kBlock) void block_compact_fixed_kernel(
    const int32_t* __restrict__ rows, const int32_t* __restrict__ counts, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ seeds, const int32_t* __restrict__ seeds_sorted, const int64_t* __restrict__ seed_order,
    const int32_t* __restrict__ uniq, const int32_t* __restrict__ sizes, int B, int k, int32_t* __restrict__ col,
    int32_t* __restrict__ dst, int32_t* __restrict__ key, int64_t* __restrict__ src_ids) {
  const int64_t tid64 = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int cap = B * (k + 1);
  if (tid64 >= cap) return;
  const int tid = static_cast<int>(tid64);
  const int nnz = min(max(sizes[0], 0), cap), n_extra = min(max(sizes[1], 0), B * k);
  if (tid >= nnz) {                                               // padding slot: in range, sorted behind every real slot
    col[tid] = 0;
    dst[tid] = 0;
    key[tid] = cap;
  }
  src_ids[tid] = tid < B ? seeds[tid] : (tid - B < n_extra ? uniq[tid - B] : seeds[0]);
  const int b = tid / (k + 1), i = tid % (k + 1);
  if (i >= counts[b]) return;
  const int slot = rowptr[b] + i;
  if (slot < 0 || slot >= nnz) return;
  const int g = rows[tid];
  const int pos = lower_bound(seeds_sorted, B, g);
  int local;
  if (pos < B && seeds_sorted[pos] == g) {
    const int64_t o = seed_order[pos];
    local = (o >= 0 && o < B) ? static_cast<int>(o) : 0;
  } else {
    const int q = lower_bound(uniq, n_extra, g);
    local = B + (q < n_extra ? q : max(n_extra - 1, 0));
  }
  col[slot] = local;
  dst[slot] = b;
  key[slot] = local;
}

__global__ __launch_bounds__(kBlock) void block_transpose_kernel(
    const int32_t* __restrict__ keys_sorted, const int64_t* __restrict__ perm, const int32_t* __restrict__ dst, int cap,
    int32_t* __restrict__ rowptrT, int32_t* __restrict__ colT, int32_t* __restrict__ slotT) {
  const int64_t tid64 = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (tid64 > cap) return;
  const int j = static_cast<int>(tid64);
  rowptrT[j] = lower_bound(keys_sorted, cap, j);
  if (j == cap) return;
  const int64_t p = perm[j];
  const bool real = keys_sorted[j] < cap && p >= 0 && p < cap;
  colT[j] = real ? dst[p] : 0;
  slotT[j] = real ? static_cast<int>(p) : 0;
}

static int check_block(const char* who, int64_t n_dst, int64_t n_src, int64_t nnz) {
  ALLSET_REQUIRE(n_dst >= 0 && n_src >= 0 && nnz >= 0, "%s: negative size", who);
  ALLSET_REQUIRE(n_src < INT32_MAX && nnz < INT32_MAX, "%s: size exceeds int32", who);
  ALLSET_REQUIRE(n_dst <= n_src, "%s: a block's targets are its first source rows (n_dst = %lld > n_src = %lld)", who,
                 static_cast<long long>(n_dst), static_cast<long long>(n_src));
  return ALLSET_OK;
}

static int check_heads(const char* who, int64_t H, int64_t C) {
  ALLSET_REQUIRE(H >= 1 && C >= 1, "%s: heads/channels must be >= 1", who);
  if (H > kMaxHeads || C > kMaxWidth || H * C > kMaxWidth) {
    set_error("%s: heads=%lld x channels=%lld exceeds the built maximum (heads <= %d, heads * channels <= %d)", who,
              static_cast<long long>(H), static_cast<long long>(C), kMaxHeads, kMaxWidth);
    return ALLSET_ERR_UNSUPPORTED;
  }
  return ALLSET_OK;
}

static int check_batch(const char* who, int64_t B, int64_t k) {
  ALLSET_REQUIRE(B >= 0 && k >= 1, "%s: need B >= 0 seeds and k >= 1 walks", who);
  if (k > kMaxWalks) {
    set_error("%s: %lld walks per seed exceeds the built maximum (%d)", who, static_cast<long long>(k), kMaxWalks);
    return ALLSET_ERR_UNSUPPORTED;
  }
  ALLSET_REQUIRE(B * (k + 1) < INT32_MAX, "%s: size exceeds int32", who);
  return ALLSET_OK;
}

static int check_fixed(const char* who, int64_t B, int64_t k) {
  int rc = check_batch(who, B, k);
  if (rc != ALLSET_OK) return rc;
  ALLSET_REQUIRE(B >= 1, "%s: a fixed-capacity block needs at least one seed", who);
  if (B * (k + 1) > kMaxFixedSlab) {
    set_error("%s: a slab of B * (k + 1) = %lld slots exceeds the built maximum (%lld)", who, static_cast<long long>(B * (k + 1)),
              static_cast<long long>(kMaxFixedSlab));
    return ALLSET_ERR_UNSUPPORTED;
  }
  return ALLSET_OK;
}

static inline unsigned lane_grid(int64_t lanes) { return static_cast<unsigned>((lanes + kBlock - 1) / kBlock); }

}  // namespace han_sample
}  // namespace allset

using namespace allset;
using namespace allset::han_sample;

extern "C" int allset_han_sampling_supported(void) { return 1; }

// counter_dev null: the step counter by value in `counter`; otherwise *counter_dev + counter (read by the kernel)
static int launch_walk(const char* who, int metapath, const int32_t* rowptr_a, const int32_t* col_a, const int32_t* rowptr_b,
                       const int32_t* col_b, int64_t n_a, int64_t n_b, int64_t id_base, const int32_t* seeds, int64_t B, int64_t k,
                       uint64_t seed, const uint64_t* counter_dev, bool dc, uint64_t counter, int32_t* endpoints, void* stream) {
  ALLSET_REQUIRE(metapath >= 0 && metapath < 256, "%s: metapath index must be in [0, 256)", who);
  int rc = check_batch(who, B, k);
  if (rc != ALLSET_OK) return rc;
  ALLSET_REQUIRE(n_a >= 0 && n_b >= 0 && id_base >= 0 && id_base + n_a < INT32_MAX && n_b < INT32_MAX, "%s: sizes must fit int32", who);
  if (B == 0) return ALLSET_OK;
  ALLSET_REQUIRE(rowptr_a && rowptr_b && seeds && endpoints, "%s: null rowptr/seeds/endpoints", who);
  ALLSET_REQUIRE(col_a && col_b, "%s: null col", who);
  ALLSET_REQUIRE(!dc || counter_dev, "%s: null counter", who);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (dc) {
    walk_dc_kernel<<<lane_grid(B * k), kBlock, 0, st>>>(rowptr_a, col_a, rowptr_b, col_b, static_cast<int>(n_a), static_cast<int>(n_b),
                                                       static_cast<int>(id_base), seeds, static_cast<int>(B), static_cast<int>(k),
                                                       counter_dev, counter, seed, metapath, endpoints);
  } else {
    walk_kernel<<<lane_grid(B * k), kBlock, 0, st>>>(rowptr_a, col_a, rowptr_b, col_b, static_cast<int>(n_a), static_cast<int>(n_b),
                                                    static_cast<int>(id_base), seeds, static_cast<int>(B), static_cast<int>(k),
                                                    walk_key(counter, seed, metapath), endpoints);
  }
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

static int launch_walk_typed(const char* who, int metapath, int64_t L, const int32_t* const* rowptrs, const int32_t* const* cols,
                             const int64_t* n_rows, const int32_t* seeds, int64_t B, int64_t k, uint64_t seed,
                             const uint64_t* counter_dev, bool dc, uint64_t counter, int32_t* endpoints, void* stream) {
  ALLSET_REQUIRE(metapath >= 0 && metapath < 256, "%s: metapath index must be in [0, 256)", who);
  ALLSET_REQUIRE(L >= 1 && L <= kMaxHops, "%s: a metapath has 1 to %d hops (HAN_MAX_HOPS), got %lld", who, kMaxHops,
                 static_cast<long long>(L));
  int rc = check_batch(who, B, k);
  if (rc != ALLSET_OK) return rc;
  ALLSET_REQUIRE(rowptrs && cols && n_rows, "%s: null relation table", who);
  HopTable t = {};
  for (int h = 0; h < L; ++h) {
    ALLSET_REQUIRE(n_rows[h] >= 0 && n_rows[h] < INT32_MAX, "%s: sizes must fit int32 (hop %d)", who, h);
    t.n_rows[h] = static_cast<int>(n_rows[h]);
  }
  if (B == 0) return ALLSET_OK;
  ALLSET_REQUIRE(seeds && endpoints, "%s: null seeds/endpoints", who);
  for (int h = 0; h < L; ++h) {
    ALLSET_REQUIRE(rowptrs[h], "%s: null rowptr (hop %d)", who, h);
    t.rowptr[h] = rowptrs[h];
    t.col[h] = cols[h];
  }
  ALLSET_REQUIRE(!dc || counter_dev, "%s: null counter", who);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (dc) {
    walk_typed_dc_kernel<<<lane_grid(B * k), kBlock, 0, st>>>(t, static_cast<int>(L), seeds, static_cast<int>(B), static_cast<int>(k),
                                                             counter_dev, counter, seed, metapath, endpoints);
  } else {
    walk_typed_kernel<<<lane_grid(B * k), kBlock, 0, st>>>(t, static_cast<int>(L), seeds, static_cast<int>(B), static_cast<int>(k),
                                                          walk_key(counter, seed, metapath), endpoints);
  }
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_han_walk(int metapath, const int32_t* rowptr_a, const int32_t* col_a, const int32_t* rowptr_b,
                               const int32_t* col_b, int64_t n_a, int64_t n_b, int64_t id_base, const int32_t* seeds, int64_t B,
                               int64_t k, uint64_t seed, uint64_t counter, int32_t* endpoints, void* stream) {
  clear_error();
  return launch_walk("han_walk", metapath, rowptr_a, col_a, rowptr_b, col_b, n_a, n_b, id_base, seeds, B, k, seed, nullptr, false, counter,
                     endpoints, stream);
}

extern "C" int allset_han_walk_dc(int metapath, const int32_t* rowptr_a, const int32_t* col_a, const int32_t* rowptr_b,
                                  const int32_t* col_b, int64_t n_a, int64_t n_b, int64_t id_base, const int32_t* seeds, int64_t B,
                                  int64_t k, uint64_t seed, const uint64_t* counter, uint64_t counter_add, int32_t* endpoints,
                                  void* stream) {
  clear_error();
  return launch_walk("han_walk_dc", metapath, rowptr_a, col_a, rowptr_b, col_b, n_a, n_b, id_base, seeds, B, k, seed, counter, true,
                     counter_add, endpoints, stream);
}

extern "C" int allset_han_walk_typed(int metapath, int64_t L, const int32_t* const* rowptrs, const int32_t* const* cols,
                                     const int64_t* n_rows, const int32_t* seeds, int64_t B, int64_t k, uint64_t seed,
                                     uint64_t counter, int32_t* endpoints, void* stream) {
  clear_error();
  return launch_walk_typed("han_walk_typed", metapath, L, rowptrs, cols, n_rows, seeds, B, k, seed, nullptr, false, counter, endpoints,
                           stream);
}

extern "C" int allset_han_walk_typed_dc(int metapath, int64_t L, const int32_t* const* rowptrs, const int32_t* const* cols,
                                        const int64_t* n_rows, const int32_t* seeds, int64_t B, int64_t k, uint64_t seed,
                                        const uint64_t* counter, uint64_t counter_add, int32_t* endpoints, void* stream) {
  clear_error();
  return launch_walk_typed("han_walk_typed_dc", metapath, L, rowptrs, cols, n_rows, seeds, B, k, seed, counter, true, counter_add,
                           endpoints, stream);
}

extern "C" int allset_han_block_rows(const int32_t* endpoints, const int32_t* seeds, const int32_t* seeds_sorted, int64_t B, int64_t k,
                                     int32_t* rows, int32_t* extra, int32_t* counts, void* stream) {
  clear_error();
  int rc = check_batch("han_block_rows", B, k);
  if (rc != ALLSET_OK) return rc;
  if (B == 0) return ALLSET_OK;
  ALLSET_REQUIRE(endpoints && seeds && seeds_sorted && rows && extra && counts, "han_block_rows: null pointer");
  block_rows_kernel<<<static_cast<unsigned>((B + kWavesPerBlock - 1) / kWavesPerBlock), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      endpoints, seeds, seeds_sorted, static_cast<int>(B), static_cast<int>(k), rows, extra, counts);
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_han_block_compact(const int32_t* rows, const int32_t* counts, const int32_t* rowptr, const int32_t* seeds_sorted,
                                        const int32_t* seed_perm, const int32_t* uniq, int64_t n_extra, int64_t B, int64_t k,
                                        int64_t nnz, int32_t* col, int32_t* dst, void* stream) {
  clear_error();
  int rc = check_batch("han_block_compact", B, k);
  if (rc != ALLSET_OK) return rc;
  ALLSET_REQUIRE(n_extra >= 0 && n_extra <= B * k && nnz >= 0 && nnz <= B * (k + 1), "han_block_compact: n_extra / nnz outside the slab");
  if (B == 0 || nnz == 0) return ALLSET_OK;
  ALLSET_REQUIRE(rows && counts && rowptr && seeds_sorted && seed_perm && col && dst, "han_block_compact: null pointer");
  ALLSET_REQUIRE(n_extra == 0 || uniq, "han_block_compact: null uniq with n_extra > 0");
  block_compact_kernel<<<lane_grid(B * (k + 1)), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      rows, counts, rowptr, seeds_sorted, seed_perm, uniq, static_cast<int>(n_extra), static_cast<int>(B), static_cast<int>(k),
      static_cast<int>(nnz), col, dst);
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_han_block_fixed_max_slab(int64_t* slots) {
  clear_error();
  ALLSET_REQUIRE(slots != nullptr, "han_block_fixed_max_slab: null pointer");
  *slots = kMaxFixedSlab;
  return ALLSET_OK;
}

extern "C" int allset_han_block_relabel(const int32_t* counts, const int32_t* extra_sorted, const int32_t* seeds_sorted, int64_t B,
                                        int64_t k, int32_t* rowptr, int32_t* uniq, int32_t* sizes, int32_t* status, void* stream) {
  clear_error();
  int rc = check_fixed("han_block_relabel", B, k);
  if (rc != ALLSET_OK) return rc;
  ALLSET_REQUIRE(counts && extra_sorted && seeds_sorted && rowptr && uniq && sizes, "han_block_relabel: null pointer");
  block_relabel_kernel<<<1, kScanBlock, 0, static_cast<hipStream_t>(stream)>>>(counts, extra_sorted, seeds_sorted, static_cast<int>(B),
                                                                              static_cast<int>(k), rowptr, uniq, sizes, status);
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_han_block_compact_fixed(const int32_t* rows, const int32_t* counts, const int32_t* rowptr, const int32_t* seeds,
                                              const int32_t* seeds_sorted, const int64_t* seed_order, const int32_t* uniq,
                                              const int32_t* sizes, int64_t B, int64_t k, int32_t* col, int32_t* dst, int32_t* key,
                                              int64_t* src_ids, void* stream) {
  clear_error();
  int rc = check_fixed("han_block_compact_fixed", B, k);
  if (rc != ALLSET_OK) return rc;
  ALLSET_REQUIRE(rows && counts && rowptr && seeds && seeds_sorted && seed_order && uniq && sizes && col && dst && key && src_ids,
                 "han_block_compact_fixed: null pointer");
  block_compact_fixed_kernel<<<lane_grid(B * (k + 1)), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      rows, counts, rowptr, seeds, seeds_sorted, seed_order, uniq, sizes, static_cast<int>(B), static_cast<int>(k), col, dst, key, src_ids);
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_han_block_transpose(const int32_t* keys_sorted, const int64_t* perm, const int32_t* dst, int64_t B, int64_t k,
                                          int32_t* rowptrT, int32_t* colT, int32_t* slotT, void* stream) {
  clear_error();
  int rc = check_fixed("han_block_transpose", B, k);
  if (rc != ALLSET_OK) return rc;
  ALLSET_REQUIRE(keys_sorted && perm && dst && rowptrT && colT && slotT, "han_block_transpose: null pointer");
  block_transpose_kernel<<<lane_grid(B * (k + 1) + 1), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      keys_sorted, perm, dst, static_cast<int>(B * (k + 1)), rowptrT, colT, slotT);
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_han_block_hop_fwd(int64_t nnz, const int32_t* rowptr, const int32_t* col, const float* el, const float* er,
                                        const float* x, int64_t ldx, float slope, const float* bias, float p_att, uint64_t seed,
                                        const uint64_t* seed_base, float* y, int64_t ldy, float* outpos, int64_t ldpos, float* ppos,
                                        float* lse, int64_t n_dst, int64_t n_src, int64_t H, int64_t C, void* stream) {
  clear_error();
  int rc = check_block("han_block_hop_fwd", n_dst, n_src, nnz);
  if (rc != ALLSET_OK) return rc;
  rc = check_heads("han_block_hop_fwd", H, C);
  if (rc != ALLSET_OK) return rc;
  return allset_han_hop_fwd(nnz, rowptr, col, el, er, x, ldx, slope, bias, p_att, seed, seed_base, y, ldy, outpos, ldpos, ppos, lse,
                            n_dst, H, C, stream);
}

extern "C" int allset_han_block_hop_bwd_stats(const float* y, int64_t ldy, const float* bias, const float* gy, int64_t ldgy,
                                              const float* outpos, int64_t ldpos, const float* ppos, const float* lse, float slope,
                                              float* g, int64_t ldg, float* stats, float* ger, int64_t n_dst, int64_t H, int64_t C,
                                              void* stream) {
  clear_error();
  ALLSET_REQUIRE(n_dst >= 0 && n_dst < INT32_MAX, "han_block_hop_bwd_stats: n_dst must fit int32");
  int rc = check_heads("han_block_hop_bwd_stats", H, C);
  if (rc != ALLSET_OK) return rc;
  return allset_han_hop_bwd_stats(y, ldy, bias, gy, ldgy, outpos, ldpos, ppos, lse, slope, g, ldg, stats, ger, n_dst, H, C, stream);
}

extern "C" int allset_han_block_hop_bwd_src(int64_t nnz, const int32_t* rowptrT, const int32_t* colT, const int32_t* slotT,
                                            const float* el, const float* er, const float* x, int64_t ldx, const float* g, int64_t ldg,
                                            const float* stats, float slope, float p_att, uint64_t seed, const uint64_t* seed_base,
                                            float* gx, int64_t ldgx, float* gel, int64_t n_dst, int64_t n_src, int64_t H, int64_t C,
                                            void* stream) {
  clear_error();
  int rc = check_block("han_block_hop_bwd_src", n_dst, n_src, nnz);
  if (rc != ALLSET_OK) return rc;
  rc = check_heads("han_block_hop_bwd_src", H, C);
  if (rc != ALLSET_OK) return rc;
  ALLSET_REQUIRE(nnz == 0 || n_dst > 0, "han_block_hop_bwd_src: edges into a block without targets");
  return allset_han_hop_bwd_src(nnz, rowptrT, colT, slotT, el, er, x, ldx, g, ldg, stats, slope, p_att, seed, seed_base, gx, ldgx, gel,
                                n_src, H, C, stream);
}
