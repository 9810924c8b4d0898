// The row epilogue of the sparse-hop kernels, y = drop_p(act(v + bias)), and its backward factor: ONE definition, read together.
// Forwards: hconv.hip, gat.hip, hattn.hip, hypergcn.hip (unignn.hip keeps its own lines, see there).  Backward: hconv.hip's
// hconv_bwd_epi_kernel, the only one -- it regenerates the forward's mask from (seed, mask index) and inverts the activation from y
// alone, so the mask index (row * width + column), the threshold (common.h drop_threshold) and the activation below are what
// the two sides must agree on.  Include after common.h.
#pragma once

namespace allset {

enum { kActNone = ALLSET_HCONV_ACT_NONE, kActRelu = ALLSET_HCONV_ACT_RELU, kActElu = ALLSET_HCONV_ACT_ELU };

struct RowEpi {
  const float* bias;      // per output column, or NULL
  int act;
  float p;
  uint64_t seed;          // resolved (seed_base folded in) at kernel start
  uint32_t thr;
  float inv_keep;
};

inline RowEpi row_epi(const float* bias, int act, float p, uint64_t seed) {
  return RowEpi{bias, act, p, seed, drop_threshold(p), drop_inv_keep(p)};
}

// ELU: whether the elu branch is built (the relu-only hops must not carry it)
template <bool ELU>
__device__ __forceinline__ float row_act(float v, int act) {
  if (act == kActRelu) v = fmaxf(v, 0.f);
  else if constexpr (ELU) {
    if (act == kActElu) v = v > 0.f ? v : expm1f(v);
  }
  return v;
}

// one element of column c.  idx() returns its mask index, row * width + c, as the CALLER's own int64_t expression, and is called only
// under p > 0, where each hop's own lines formed it: (row, c, width) costs hconv.hip a 32-bit add and a sign extension per element
// where it had one 64-bit add, and an index evaluated as an argument, ahead of the bias branch, reorders every hop's instructions.
// Callers pass [=] { return static_cast<int64_t>(row) * width + ...; }.
template <bool ELU, typename Idx>
__device__ __forceinline__ float row_epilogue(const RowEpi& e, float v, int c, Idx idx) {
  if (e.bias) v += e.bias[c];
  v = row_act<ELU>(v, e.act);
  if (e.p > 0.f) v *= keep_scale(e.seed, idx(), e.thr, e.inv_keep);
  return v;
}

// g = gy * k * act'(y) with k the element's keep scale (0 or 1 / keep) and act' recovered from the saved output alone:
// relu -> y > 0; elu -> with a = y * keep the pre-dropout activation of a KEPT element, 1 if a > 0 else a + 1
// (elu'(z) = exp(z) = elu(z) + 1 for z <= 0)
__device__ __forceinline__ float row_epilogue_bwd(float gv, float yv, float k, int act, float keep) {
  if (act == kActRelu) return yv > 0.f ? gv * k : 0.f;             // (a select, as torch's relu backward: no 0 * NaN)
  if (act == kActElu) {
    const float a = yv * keep;
    return gv * k * (a > 0.f ? 1.f : a + 1.f);
  }
  return gv * k;
}

}  // namespace allset
