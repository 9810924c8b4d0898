// Clique expansion of a hypergraph and its GCN normalisation for the CEGCN baseline (reference preprocessing.py:343-391
// ConstructV2V, and norm_contruction(TYPE='V2V') = torch_geometric 1.6.3 gcn_norm with add_self_loops) for gfx950.  The reference
// loops in Python over itertools.combinations of every hyperedge and fills a dict; here it is a count, a scan, an emit and a sort:
//   allset_clique_count: cnt[e] = k_e (k_e - 1) / 2 from the hyperedge -> member CSR (members ascending within a row);
//   allset_clique_emit:  one thread per incidence (member a of hyperedge e) writes its k_e - 1 - a pairs (v_a, v_b), b > a, as
//                        64-bit keys v_a << 32 | v_b at off[e] + a (k_e - 1) - a (a - 1) / 2 (off: exclusive scan of cnt);
//   (the caller sorts the keys and counts equal ones: the multiplicity of a pair)
//   allset_gcn_norm:     from the pairs (i, j) and their weights m: deg[j] = 1 + sum_{pairs (i, j)} m (the remaining self-loop of
//                        weight 1 of every id < n), then the edge list [pairs | loops 0..n-1] as int64 rows and
//                        w = deg^-1/2[i] * m * deg^-1/2[j].
// The degree sum is float atomics: exact and order-independent for integer-valued weights below 2^24 (the multiplicities of the
// reference's use); other weights may differ in their last bits from run to run.
#include "common.h"

namespace allset {
namespace clique {

__global__ __launch_bounds__(kBlock) void count_kernel(const int32_t* __restrict__ rowptr, int64_t n_e, int64_t* __restrict__ cnt) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= n_e) return;
  const int64_t k = rowptr[e + 1] - rowptr[e];
  cnt[e] = k * (k - 1) / 2;
}

__global__ __launch_bounds__(kBlock) void emit_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ member,
                                                      const int32_t* __restrict__ edge_of, const int64_t* __restrict__ off, int64_t nnz,
                                                      int64_t* __restrict__ keys) {
  const int64_t q = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (q >= nnz) return;
  const int e = edge_of[q];
  const int64_t start = rowptr[e];
  const int64_t k = rowptr[e + 1] - start;
  const int64_t a = q - start;
  int64_t* out = keys + off[e] + a * (k - 1) - a * (a - 1) / 2;
  const int64_t vi = static_cast<int64_t>(member[q]) << 32;
  for (int64_t b = a + 1; b < k; ++b) out[b - a - 1] = vi | static_cast<int64_t>(member[start + b]);
}

__global__ __launch_bounds__(kBlock) void deg_kernel(const int64_t* __restrict__ dst, const float* __restrict__ m, int64_t n_pairs,
                                                     float* __restrict__ deg) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (t < n_pairs) atomicAdd(deg + dst[t], m ? m[t] : 1.f);
}

__global__ __launch_bounds__(kBlock) void edges_kernel(const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                       const float* __restrict__ m, int64_t n_pairs, int64_t n,
                                                       const float* __restrict__ deg, int64_t* __restrict__ src_out,
                                                       int64_t* __restrict__ dst_out, float* __restrict__ w) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= n_pairs + n) return;
  int64_t i, j;
  float wt = 1.f;
  if (t < n_pairs) {
    i = src[t];
    j = dst[t];
    if (m) wt = m[t];
  } else {
    i = j = t - n_pairs;
  }
  const float di = 1.f / sqrtf(deg[i] + 1.f), dj = 1.f / sqrtf(deg[j] + 1.f);   // + 1: the self-loop of every id < n
  src_out[t] = i;
  dst_out[t] = j;
  w[t] = di * wt * dj;
}

static inline unsigned grid_of(int64_t n) { return static_cast<unsigned>((n + kBlock - 1) / kBlock); }

}  // namespace clique
}  // namespace allset

using namespace allset;
using namespace allset::clique;

extern "C" int allset_clique_count(const int32_t* rowptr, int64_t n_e, int64_t* cnt, void* stream) {
  clear_error();
  ALLSET_REQUIRE(n_e >= 0 && n_e < INT32_MAX, "clique_count: bad hyperedge count %lld", static_cast<long long>(n_e));
  if (n_e == 0) return ALLSET_OK;
  ALLSET_REQUIRE(rowptr && cnt, "clique_count: null pointer");
  count_kernel<<<grid_of(n_e), kBlock, 0, static_cast<hipStream_t>(stream)>>>(rowptr, n_e, cnt);
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_clique_emit(const int32_t* rowptr, const int32_t* member, const int32_t* edge_of, const int64_t* off, int64_t nnz,
                                  int64_t* keys, void* stream) {
  clear_error();
  ALLSET_REQUIRE(nnz >= 0 && nnz < INT32_MAX, "clique_emit: bad incidence count %lld", static_cast<long long>(nnz));
  if (nnz == 0) return ALLSET_OK;
  ALLSET_REQUIRE(rowptr && member && edge_of && off && keys, "clique_emit: null pointer");
  emit_kernel<<<grid_of(nnz), kBlock, 0, static_cast<hipStream_t>(stream)>>>(rowptr, member, edge_of, off, nnz, keys);
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

extern "C" int allset_gcn_norm(const int64_t* src, const int64_t* dst, const float* m, int64_t n_pairs, int64_t n, float* deg,
                               int64_t* src_out, int64_t* dst_out, float* w, void* stream) {
  clear_error();
  ALLSET_REQUIRE(n_pairs >= 0 && n >= 0 && n_pairs + n < INT32_MAX, "gcn_norm: bad sizes (%lld pairs, %lld ids)",
                 static_cast<long long>(n_pairs), static_cast<long long>(n));
  if (n_pairs + n == 0) return ALLSET_OK;
  ALLSET_REQUIRE(deg && src_out && dst_out && w && (n_pairs == 0 || (src && dst)), "gcn_norm: null pointer");
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (n > 0) ALLSET_HIP_CHECK(hipMemsetAsync(deg, 0, static_cast<size_t>(n) * sizeof(float), st));
  if (n_pairs > 0) {
    deg_kernel<<<grid_of(n_pairs), kBlock, 0, st>>>(dst, m, n_pairs, deg);
    ALLSET_LAUNCH_CHECK();
  }
  edges_kernel<<<grid_of(n_pairs + n), kBlock, 0, st>>>(src, dst, m, n_pairs, n, deg, src_out, dst_out, w);
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}
