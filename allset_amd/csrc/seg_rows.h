// Row loads and stores shared by the per-segment row kernels (loo.hip: leave-one-out sums; scan.hip: exclusive prefix / suffix sums):
// a feature row of d f32 is covered by LPR lanes x 16 B, a lane group ("slot") keeps kLooRows rows of its run in registers as packed
// 16-byte loads issued back to back.  Include after common.h.
#pragma once

namespace allset {

constexpr int kLooRows = 8;                       // rows of a run a slot holds in registers
constexpr int kLooLong = 64;                      // segments longer than this belong to the workgroup kernel
constexpr int kLooBlock = 512;
constexpr int kLooMaxD = 512;

struct LooArgs {
  const int32_t* rowptr;
  const int32_t* col;        // null: rows are the positions themselves
  const float* src;
  int64_t lds;
  const float* s_src;        // null: ones
  const float* s_seg;        // null: ones
  float* out;
  int64_t ldo;
  int d;
};

// rows q0 .. q0 + n of a run, scaled by s_src, zero beyond n (and in lanes beyond the row's width)
__device__ __forceinline__ void loo_load(const LooArgs& a, int q0, int n, int c0, bool active, float (&v)[kLooRows][4]) {
  int idx[kLooRows];
  float sc[kLooRows];
  Raw<float, 4> raw[kLooRows];
#pragma unroll
  for (int u = 0; u < kLooRows; ++u) idx[u] = (u < n && a.col != nullptr) ? a.col[q0 + u] : q0 + u;
#pragma unroll
  for (int u = 0; u < kLooRows; ++u) {
    sc[u] = (u < n && a.s_src != nullptr) ? a.s_src[idx[u]] : 1.f;
    if (u < n && active) raw[u] = load_raw<float, 4>(a.src + static_cast<int64_t>(idx[u]) * a.lds + c0);
    else raw[u] = zero_raw<float, 4>();
  }
#pragma unroll
  for (int u = 0; u < kLooRows; ++u) {
    const FVec<4> f = unpack<float, 4>(raw[u]);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[u][k] = sc[u] * f.v[k];
  }
}

__device__ __forceinline__ void loo_store(const LooArgs& a, int p, int c0, const float (&r)[4]) {
  FVec<4> f;
#pragma unroll
  for (int k = 0; k < 4; ++k) f.v[k] = r[k];
  store_vec<float, 4>(a.out + static_cast<int64_t>(p) * a.ldo + c0, f);
}

static inline int loo_lpr(int64_t d) {
  int lpr = 8;
  while (lpr * 4 < d && lpr < 64) lpr <<= 1;
  return lpr;
}

}  // namespace allset
