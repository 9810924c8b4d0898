// The fused Linear forward (math: fused_mlp.hip fused_linear_fwd_x6_kernel) for K = N = 128 with the CU's waves SPLIT BY ROLE, the
// organisation of the one-pass backward (fused_bwd4.hip) carried over -- and with what that kernel could not afford: TWO vector
// waves per SIMD.  768 threads: waves 0-7 do all the vector work, waves 8-11 all the matrix work; wave w runs on SIMD w % 4, so
// every SIMD holds two vector waves and one matrix wave (168 registers each).
//
// Why: the symmetric kernel spends, per 16-row chunk and wave, 1390 VALU instructions next to 192 MFMAs; on a SIMD with two (or
// three) such waves vector phases collide with vector phases and matrix phases with matrix phases, so the two kinds of time add
// (DESIGN.md 6a''').  With the roles split a SIMD's matrix pipe belongs to one wave that does nothing else (W slice in 96
// registers, no W in LDS), and its vector issue port alternates between two waves whose dependent chains (LayerNorm row sums,
// hashes, three-plane splits) hide each other's latency -- which a lone vector wave per SIMD could not (fused_bwd4.hip: 7.6 cycles
// per instruction).
//
// Stage = 32 rows, one workgroup barrier per stage:
//     tick t   vector waves: S0(t+1): x(t+1) -> LayerNorm / relu / dropout -> three bf16 planes -> img[(t+1) % 2]
//                            E(t-1) : ytile[(t-1) % 2] + bias -> relu / dropout / 1-bit mask -> y
//              matrix waves: S1(t)  : img[t % 2] @ W^T -> ytile[t % 2]            (96 x v_mfma_f32_16x16x32_bf16 per wave)
// Two operand images and two output tiles make every hand-off a tick boundary.  Vector wave v owns rows 4 v .. 4 v + 3 of a stage,
// one row per DPP row of 16 lanes (row sums = four DPP adds), 8 elements per lane and stage; the rows of the next TWO stages are in
// flight in two register sets.  Same k-order and product order as fused_linear_fwd_x6_kernel: given the same LayerNorm statistics
// the outputs are bit-identical to that kernel's; the statistics themselves differ in the last bits (DPP row sums vs per-lane
// partial sums + two shuffles).
// LDS: 2 x 24 KB images + 2 x 16.5 KB tiles + gamma / beta / bias = 83 KB.
//
// Arithmetic (round 4): behind a true LayerNorm prologue the products are formed from TWO fp16 planes per operand, three f16 MFMAs each
// (template F16, "fp16x3": fused_bwd6.hip has the scheme and its error model) -- 48 MFMAs per wave and stage, two LDS planes, W in 64
// registers, 112 registers per wave; the matrix waves were this kernel's critical role too (ablation: 0.285 ms, 0.182 without the
// MFMAs).  Without a norm and in the column-affine mode the operand has no bound known in advance and the kernel stays bf16x6.
#include <stdlib.h>

#include "common.h"
#include "mfma.h"

namespace allset {

constexpr int kF2Block = 768;
constexpr int kF2Rows = 32;                    // rows per stage
constexpr int kF2VWaves = 8;
constexpr int kF2Sets = 4;                     // register sets of prefetched rows per vector wave

#ifdef ALLSET_ABL5_NOBAR            // ablation builds only (tools/fwd_roles_ablation.py): timing without the barriers, results wrong
#define ALLSET_TICK() ALLSET_TICK_NO_BARRIER()
#else
#define ALLSET_TICK() ALLSET_TICK_BARRIER()
#endif

// XM ("extra mode", round 5 -- the PMA tail of reference layers.py:153-157 folded into its two rFF Linears, fp16x3 only):
//   1  prologue = LayerNorm(x + colb) (ln0 with the seed add riding in it), whose OUTPUT is also written to `uo` (the residual
//      branch and the backward need it): one kernel instead of allset_ln_res_fwd + allset_fused_linear_fwd;
//   2  no LayerNorm in front (row-scaled fp16x3, below); epilogue = z = relu?(. + bias) [1-bit mask of z], s = res + z -> `uo`,
//      y = dropout(relu_post?(LayerNorm_{gamma,beta,eps}(s))), statistics of s -> `stats`: ln1 and the residual add inside the
//      second rFF Linear, one kernel instead of allset_fused_linear_fwd + allset_ln_res_fwd.
// AUX (round 6): four auxiliary output columns aux_out[r, 0..3] = pro(x)[r, :] . aux_w[j, :] + aux_b[j] in plain fp32 FMAs of the vector
// waves -- PMA's folded attention logits riding along with its value projection (reference layers.py:128-130: the row is in the
// staging lane's registers anyway; a row's 128 columns sit in the 16 lanes of a DPP row).  Until round 6 an auxiliary projection took
// the symmetric bf16x6 kernel of fused_mlp.hip (0.35 ms per [1M, 128] launch against 0.20 here).
//   3  the output leaves as PACKED NONZERO ROWS (include/allset_hip_ext.h, DESIGN.md 4.5: 128-bit occupancy mask + the occupied elements,
//      256 bytes per row) -> `uo`, the format the forward Deep Sets gather reads, instead of the dense table: the epilogue packs each
//      row it holds in registers anyway, so neither the dense write nor pack_kernel's pass over it happens.  A row above kPackCap
//      occupied columns also goes, dense, to row r of `y` (the overflow side table: nothing else of it is ever written).  Built for
//      <HAS_LN, DROP_IN, DROP_OUT> = <true, true, true> only, in both arithmetics.
//   4  mode 3 with the CELL layout of include/allset_hip_ext.h (16 cells of {v0, v1, v2, {col0, col1, col2, k}}: each occupied element
//      with its column beside it, rank j in cell j % 16, slot j / 16), the format segreduce_cells_kernel gathers; rows above kCellCap
//      occupied columns also go to the side table.  Same restrictions as mode 3.
template <bool HAS_LN, bool DROP_IN, bool DROP_OUT, bool D8, bool F16, int XM = 0, bool AUX = false>
__global__ __launch_bounds__(kF2Block) void fused_linear_fwd_roles_kernel(
    const float* __restrict__ x, int64_t ldx, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
    int relu_in, float p_in, uint64_t seed_in, const float* __restrict__ W, const float* __restrict__ bias, int relu_out,
    float p_out, uint64_t seed_out, float* __restrict__ y, int64_t ldy, float* __restrict__ stats, int64_t n,
    const uint64_t* __restrict__ seed_base, uint32_t* __restrict__ mask_out, int64_t xcb, int64_t ycb, float ln_inv,
    const float* __restrict__ colb = nullptr, float* __restrict__ uo = nullptr, int64_t lduo = 0,
    const float* __restrict__ res = nullptr, int64_t ldres = 0, int relu_post = 0,
    const float* __restrict__ aux_w = nullptr, const float* __restrict__ aux_b = nullptr, float* __restrict__ aux_out = nullptr) {
  static_assert(!AUX || (XM == 0 && !DROP_IN && !HAS_LN), "auxiliary columns: the plain prologue only (behind a LayerNorm the fp16x3 form folds 2^Su into gamma / beta)");
  static_assert(XM == 0 || XM == 3 || XM == 4 || F16, "the tail modes are built on the fp16x3 arithmetic only");
  static_assert((XM != 3 && XM != 4) || (HAS_LN && DROP_IN && DROP_OUT && !AUX), "modes 3 and 4: LayerNorm prologue, dropout in and out");
  static_assert(XM != 1 || (HAS_LN && !DROP_IN && !DROP_OUT), "mode 1: LayerNorm prologue, no dropout");
  static_assert(XM != 2 || (!HAS_LN && !DROP_IN), "mode 2: plain operand, LayerNorm in the epilogue");
  constexpr bool ROWSC = F16 && !HAS_LN;        // fp16x3 without a bound on the operand: one power of two per ROW, from its largest element
  constexpr bool AFF = HAS_LN || XM == 2;       // sG / sB hold a LayerNorm's affine parameters (prologue's, or mode 2's epilogue's)
  // ln_inv: 1 / 128 for the LayerNorm prologue; 0 (with eps = 1) switches the row statistics off -- mean = 0, rstd = 1, which is
  // what gets written to `stats` -- and leaves the per-column affine map x * gamma + beta: BatchNorm with batch statistics
  // folded into (gamma, beta) by the caller (ALLSET_NORM_COLUMN_AFFINE, csrc/batchnorm.hip).
  // xcb / ycb: 0 = row-major [n][128] with leading dimension ldx / ldy; cb > 0 = COLUMN-BLOCKED [128 / cb][n][cb] (ld == cb): the
  // layout the column-sharded layer's all-to-all sends and receives (allset_amd/dist.py) -- reading / writing it here removes the
  // pack / unpack passes around the exchange.  A lane's 16 bytes stay inside one block (cb >= 4).
  constexpr int KD = 128, ND = 128;
  constexpr int R = kF2Rows;
  constexpr int PLANE = R * 256;                 // bytes per bf16 plane of an image
  constexpr int IMG = 3 * PLANE;
  constexpr int SPY = 132;                       // pitch (floats) of an output tile
  __shared__ __attribute__((aligned(16))) uint8_t sX[2 * IMG];
  __shared__ __attribute__((aligned(16))) float sY[2 * R * SPY];
  __shared__ __attribute__((aligned(16))) float sG[KD];
  __shared__ __attribute__((aligned(16))) float sB[KD];
  __shared__ __attribute__((aligned(16))) float sBias[ND];
  seed_in = resolve_seed(seed_base, seed_in);
  seed_out = resolve_seed(seed_base, seed_out);
  const int tid = threadIdx.x;
  __shared__ __attribute__((aligned(16))) float sCol[XM == 1 ? KD : 4];
  if (tid < KD) { sG[tid] = AFF ? gamma[tid] : 1.f; sB[tid] = AFF ? beta[tid] : 0.f; sBias[tid] = bias ? bias[tid] : 0.f; }
  if constexpr (XM == 1) { if (tid < KD) sCol[tid] = colb ? colb[tid] : 0.f; }
  __shared__ __attribute__((aligned(16))) float sAuxW[AUX ? 4 * KD + 4 : 4];       // aux_w [4][KD], then aux_b [4]
  if constexpr (AUX) {
    if (tid < 4 * KD) sAuxW[tid] = aux_w[tid];
    if (tid < 4) sAuxW[4 * KD + tid] = aux_b ? aux_b[tid] : 0.f;
  }
  const int lane0 = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t n_stages = (n + R - 1) / R;
  // this workgroup's stages: blockIdx.x + k * gridDim.x, k = 0 .. T - 1 (T >= 1: the grid never exceeds the stage count)
  const int64_t T = (n_stages - blockIdx.x + gridDim.x - 1) / gridDim.x;
  auto stage_of = [&](int64_t k) -> int64_t { return blockIdx.x + (k < T ? k : T - 1) * static_cast<int64_t>(gridDim.x); };
  auto rows_left = [&](int64_t stage) -> int {
    const int64_t left = n - stage * R;
    return left >= R ? R : (left > 0 ? static_cast<int>(left) : 0);
  };
  __syncthreads();
  // F16 (a true LayerNorm prologue only): the products are formed from two fp16 planes per operand, three MFMAs each (fused_bwd6.hip).
  // The LayerNorm output is bounded without a data pass, |u| <= (sqrt(127) max|gamma| + max|beta|) keep, so ONE power of two 2^Su for
  // the whole launch brings it below 2^14 -- folded into gamma and beta, it costs no instruction; W is scaled per matrix wave's
  // slice; both are undone where the wave writes its output tile.
  // Without a LayerNorm in front (ROWSC) the window comes from the row itself: the vector wave that stages a row takes the
  // exponent of its largest element (a DPP row maximum of values it already holds), scales the row's planes by that power of two
  // and undoes it in the SAME lanes' epilogue two ticks later (a lane owns the same rows in S0 and E).
  int Su = 0;
  if constexpr (F16 && HAS_LN) {
    float g = fmaxf(fabsf(sG[lane0]), fabsf(sG[lane0 + 64])), bm = fmaxf(fabsf(sB[lane0]), fabsf(sB[lane0 + 64]));
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { g = fmaxf(g, __shfl_xor(g, off)); bm = fmaxf(bm, __shfl_xor(bm, off)); }
    const float U = (11.27f * g + bm) * (DROP_IN ? 1.f / (1.f - p_in) : 1.f);
    const int eU = static_cast<int>(__float_as_uint(U) >> 23);          // U < 2^(eU - 126)
    Su = __builtin_amdgcn_readfirstlane(min(max(140 - eU, -100), 100));
  }
#ifdef ALLSET_ABL5_TIMING          // diagnostic builds only: cycles per segment of waves 0 (vector) and 8 (matrix) of workgroup 0
  uint64_t tph[4] = {0, 0, 0, 0}, tlast = __builtin_readcyclecounter();
#define ALLSET_MARK(k) ALLSET_PHASE_MARK(k)
#else
#define ALLSET_MARK(k) do {} while (0)
#endif

  if (wave < kF2VWaves) {
    // =================================================== vector waves ===================================================
    const float inv_k = ln_inv;
    const float keep_in = DROP_IN ? 1.f / (1.f - p_in) : 1.f;
    const float keep_out = DROP_OUT ? 1.f / (1.f - p_out) : 1.f;
    const uint32_t thr_in = drop_threshold(p_in), thr_out = drop_threshold(p_out);
    const int c = lane0 & 15, rg = lane0 >> 4;
    const int lr = 4 * wave + rg;                // this lane's row of a stage; columns 64 hb + 4 c .. + 3, hb = 0, 1
    float4 gam[2], bet[2], bia[2];
    // A lane's columns 64 hb + 4 c: byte offset of columns 4 c (one 32-bit VGPR per operand) + hb x a wave-uniform step --
    // 256 bytes in a row-major row, 64 columns' worth of blocks (256 n bytes) in the blocked layout (cb <= 64 divides 64)
    const uint32_t cox0 = xcb ? static_cast<uint32_t>((((4 * c) / xcb) * n * xcb + (4 * c) % xcb) * 4) : 16u * c;
    const uint32_t coy0 = ycb ? static_cast<uint32_t>((((4 * c) / ycb) * n * ycb + (4 * c) % ycb) * 4) : 16u * c;
    const int64_t dhx = xcb ? 256 * n : 256, dhy = ycb ? 256 * n : 256;
#pragma unroll
    for (int hb = 0; hb < 2; ++hb) {
      gam[hb] = *reinterpret_cast<const float4*>(&sG[64 * hb + 4 * c]);
      bet[hb] = *reinterpret_cast<const float4*>(&sB[64 * hb + 4 * c]);
      bia[hb] = *reinterpret_cast<const float4*>(&sBias[64 * hb + 4 * c]);
      if constexpr (F16 && HAS_LN && XM != 1) {     // (mode 1 stores the unscaled LayerNorm output: it scales at the split instead)
        const float su = __uint_as_float(static_cast<uint32_t>(127 + Su) << 23);
        gam[hb].x *= su; gam[hb].y *= su; gam[hb].z *= su; gam[hb].w *= su;
        bet[hb].x *= su; bet[hb].y *= su; bet[hb].z *= su; bet[hb].w *= su;
      }
    }
    const float su1 = XM == 1 ? __uint_as_float(static_cast<uint32_t>(127 + Su) << 23) : 1.f;
    int eA = 20, eB = 20, eC = 20;               // ROWSC: biased row exponents of the last three stages staged (E(k) reads eC, the last E eB)
    float4 resR[2];                              // mode 2: the residual rows of the next stage to leave
    auto request_res = [&](int64_t k) {
      if constexpr (XM == 2) {
        const int64_t s0 = stage_of(k);
        const int nrc = max(rows_left(s0), 1);
        const int lrc = min(lr, nrc - 1);
        const char* rb = reinterpret_cast<const char*>(res + s0 * R * ldres);
#pragma unroll
        for (int hb = 0; hb < 2; ++hb)
          resR[hb] = *reinterpret_cast<const float4*>(rb + hb * 256 + (static_cast<uint32_t>(lrc) * static_cast<uint32_t>(ldres) * 4u + 16u * c));
      }
    };
    // [set][hb]: the rows of the next kF2Sets stages.  Bytes in flight bound these kernels (~2 us of loaded latency, DESIGN.md 6a'''):
    // a vector wave's share of a stage is 2 KB, so four sets = 64 KB per CU, 16 MB chip-wide -- at 8 registers per set
    float4 xrS[kF2Sets][2];
    // Loads are unconditional on a clamped row / stage (no exec-mask branch around a memory instruction: its join costs
    // s_waitcnt vmcnt(0) and drains the prefetch); what was read for a row past n is never stored.
    auto request_x = [&](int64_t k, float4 (&xr)[2]) {
      const int64_t s0 = stage_of(k);
      const int nrc = max(rows_left(s0), 1);
      const int lrc = min(lr, nrc - 1);
      const char* xb = reinterpret_cast<const char*>(x + s0 * R * ldx);
#pragma unroll
      for (int hb = 0; hb < 2; ++hb)
        xr[hb] = *reinterpret_cast<const float4*>(xb + hb * dhx + (static_cast<uint32_t>(lrc) * static_cast<uint32_t>(ldx) * 4u + cox0));
    };
    // pair index of (row, column) = stage * 2048 + (lr * 128 + column) / 2: the lane's part is < 2048 -> an OR (common.h pair_hash)
    auto keep4 = [&](uint64_t seed, int64_t stage, int hb, uint32_t thr, float keep) -> float4 {
      const uint32_t sl = static_cast<uint32_t>(seed);
      // (D8: every active dropout of the launch has the 8-bit resolution -- known at compile time, the 16-bit path and the branch
      //  between them drop out of the heavy variant's vector loop: -4 % on its launch time)
      if (D8 || (thr & kDrop8)) {     // 8 bits per element: ONE hash for the lane's float4 (quad index = stage * 1024 + lane part < 1024)
        const uint64_t stage_quad = static_cast<uint64_t>(stage) * (R * KD / 4);
        const uint32_t hi_term = __umul24(static_cast<uint32_t>(stage_quad >> 32), 0x5EBCA7U) + static_cast<uint32_t>(seed >> 32);
        const uint32_t lo = static_cast<uint32_t>(stage_quad) | static_cast<uint32_t>((lr * KD + 64 * hb + 4 * c) >> 2);
        const uint32_t h = hash_mix((lo ^ sl) * 0x9E3779B1U + hi_term), t8 = thr & 0xffu;
        return make_float4((h & 0xffu) >= t8 ? keep : 0.f, ((h >> 8) & 0xffu) >= t8 ? keep : 0.f,
                           ((h >> 16) & 0xffu) >= t8 ? keep : 0.f, (h >> 24) >= t8 ? keep : 0.f);
      }
      const uint64_t stage_pair = static_cast<uint64_t>(stage) * (R * KD / 2);
      const uint32_t hi_term = __umul24(static_cast<uint32_t>(stage_pair >> 32), 0x5EBCA7U) + static_cast<uint32_t>(seed >> 32);
      const uint32_t lo = static_cast<uint32_t>(stage_pair) | static_cast<uint32_t>((lr * KD + 64 * hb + 4 * c) >> 1);
      const uint32_t h0 = hash_mix((lo ^ sl) * 0x9E3779B1U + hi_term);
      const uint32_t h1 = hash_mix(((lo + 1u) ^ sl) * 0x9E3779B1U + hi_term);
      return make_float4((h0 & 0xffffu) >= thr ? keep : 0.f, (h0 >> 16) >= thr ? keep : 0.f,
                         (h1 & 0xffffu) >= thr ? keep : 0.f, (h1 >> 16) >= thr ? keep : 0.f);
    };
    // ---- S0(k): the prologue of stage k -> three bf16 planes into img[k % 2]; then the request for x(k + 2)
    auto S0 = [&](int64_t k, float4 (&xr)[2]) {
      const int64_t stage = stage_of(k);
      const bool live = lr < rows_left(stage);
      uint8_t* img = sX + (k & 1) * IMG;
      float4 t[2] = {xr[0], xr[1]};
      if constexpr (XM == 1) {
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
          const float4 cb4 = *reinterpret_cast<const float4*>(&sCol[64 * hb + 4 * c]);
          t[hb].x += cb4.x; t[hb].y += cb4.y; t[hb].z += cb4.z; t[hb].w += cb4.w;
        }
      }
      if (relu_in) {
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
          t[hb].x = fmaxf(t[hb].x, 0.f); t[hb].y = fmaxf(t[hb].y, 0.f); t[hb].z = fmaxf(t[hb].z, 0.f); t[hb].w = fmaxf(t[hb].w, 0.f);
        }
      }
      if constexpr (HAS_LN) {
        const float s = row16_sum(((t[0].x + t[0].y) + (t[0].z + t[0].w)) + ((t[1].x + t[1].y) + (t[1].z + t[1].w)));
        const float mean = s * inv_k;
        float q2 = 0.f;
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
          t[hb].x -= mean; t[hb].y -= mean; t[hb].z -= mean; t[hb].w -= mean;
          q2 = fmaf(t[hb].x, t[hb].x, fmaf(t[hb].y, t[hb].y, fmaf(t[hb].z, t[hb].z, fmaf(t[hb].w, t[hb].w, q2))));
        }
        const float rstd = rsqrtf(row16_sum(q2) * inv_k + eps);
        if (live && c == 0) *reinterpret_cast<float2*>(stats + (stage * R + lr) * 2) = make_float2(mean, rstd);
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
          t[hb].x = fmaf(t[hb].x * rstd, gam[hb].x, bet[hb].x); t[hb].y = fmaf(t[hb].y * rstd, gam[hb].y, bet[hb].y);
          t[hb].z = fmaf(t[hb].z * rstd, gam[hb].z, bet[hb].z); t[hb].w = fmaf(t[hb].w * rstd, gam[hb].w, bet[hb].w);
        }
      }
      if constexpr (XM == 1) {                    // the LayerNorm output itself: `out` of reference layers.py:156
        if (live) {
          char* ub = reinterpret_cast<char*>(uo + stage * R * lduo) + static_cast<uint32_t>(lr) * static_cast<uint32_t>(lduo) * 4u + 16u * c;
          *reinterpret_cast<float4*>(ub) = t[0];
          *reinterpret_cast<float4*>(ub + 256) = t[1];
        }
      }
      if constexpr (AUX) {
        float s4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float4 w0 = *reinterpret_cast<const float4*>(&sAuxW[j * KD + 4 * c]), w1 = *reinterpret_cast<const float4*>(&sAuxW[j * KD + 64 + 4 * c]);
          s4[j] = row16_sum(fmaf(t[0].x, w0.x, fmaf(t[0].y, w0.y, fmaf(t[0].z, w0.z, t[0].w * w0.w))) +
                              fmaf(t[1].x, w1.x, fmaf(t[1].y, w1.y, fmaf(t[1].z, w1.z, t[1].w * w1.w))));
        }
        if (live && c == 0)
          *reinterpret_cast<float4*>(aux_out + (stage * R + lr) * 4) =
              make_float4(s4[0] + sAuxW[4 * KD], s4[1] + sAuxW[4 * KD + 1], s4[2] + sAuxW[4 * KD + 2], s4[3] + sAuxW[4 * KD + 3]);
      }
      float rsc = su1;                             // the factor applied at the split: mode 1's launch-wide 2^Su, ROWSC's row scale
      if constexpr (ROWSC) {
        float amax = 0.f;
#pragma unroll
        for (int hb = 0; hb < 2; ++hb)
          amax = fmaxf(fmaxf(fmaxf(fabsf(t[hb].x), fabsf(t[hb].y)), fmaxf(fabsf(t[hb].z), fabsf(t[hb].w))), amax);
        amax = fmaxf(amax, dpp_row<0xB1>(amax)); amax = fmaxf(amax, dpp_row<0x4E>(amax));
        amax = fmaxf(amax, dpp_row<0x141>(amax)); amax = fmaxf(amax, dpp_row<0x140>(amax));
        const int e = min(max(static_cast<int>(__float_as_uint(amax * keep_in) >> 23), 20), 254);
        eC = eB; eB = eA; eA = e;
        rsc = __uint_as_float(static_cast<uint32_t>(254 + 13 - e) << 23);       // the row's largest element -> [2^13, 2^14)
      }
#pragma unroll
      for (int hb = 0; hb < 2; ++hb) {
        if constexpr (DROP_IN) {
          const float4 kp = keep4(seed_in, stage, hb, thr_in, keep_in);
          t[hb].x *= kp.x; t[hb].y *= kp.y; t[hb].z *= kp.z; t[hb].w *= kp.w;
        }
        if constexpr (ROWSC || XM == 1) { t[hb].x *= rsc; t[hb].y *= rsc; t[hb].z *= rsc; t[hb].w *= rsc; }
        const int wo = swizzle256(lr, 128 * hb + 8 * c);
        if constexpr (F16) {
          uint32_t h0, l0, h1, l1;
          split2_f16(t[hb].x, t[hb].y, h0, l0);
          split2_f16(t[hb].z, t[hb].w, h1, l1);
          *reinterpret_cast<uint2*>(img + 0 * PLANE + wo) = make_uint2(h0, h1);
          *reinterpret_cast<uint2*>(img + 1 * PLANE + wo) = make_uint2(l0, l1);
        } else {
          uint32_t h0, m0, l0, h1, m1, l1;
          split3_bf16(t[hb].x, t[hb].y, h0, m0, l0);
          split3_bf16(t[hb].z, t[hb].w, h1, m1, l1);
          *reinterpret_cast<uint2*>(img + 0 * PLANE + wo) = make_uint2(h0, h1);
          *reinterpret_cast<uint2*>(img + 1 * PLANE + wo) = make_uint2(m0, m1);
          *reinterpret_cast<uint2*>(img + 2 * PLANE + wo) = make_uint2(l0, l1);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      request_x(k + kF2Sets, xr);                // into the set just consumed: kF2Sets stages ahead
      __builtin_amdgcn_sched_barrier(0);
    };
    // ---- E(k): the epilogue of stage k from ytile[k % 2]
    auto E = [&](int64_t k, int erow) {
      const int64_t stage = stage_of(k);
      const int nrows = rows_left(stage);
      const bool live = lr < nrows;
      const float* ty = sY + (k & 1) * (R * SPY);
      char* yb = reinterpret_cast<char*>(y + stage * R * ldy);
      const uint32_t yo = static_cast<uint32_t>(lr) * static_cast<uint32_t>(ldy) * 4u + coy0;
      const float unsc = ROWSC ? __uint_as_float(static_cast<uint32_t>(erow - 13) << 23) : 1.f;       // undoes the row's 2^(140 - e)
      float4 vv[2];
#pragma unroll
      for (int hb = 0; hb < 2; ++hb) {
        float4 v = *reinterpret_cast<const float4*>(&ty[lr * SPY + 64 * hb + 4 * c]);
        if constexpr (ROWSC) {
          v.x = fmaf(v.x, unsc, bia[hb].x); v.y = fmaf(v.y, unsc, bia[hb].y); v.z = fmaf(v.z, unsc, bia[hb].z); v.w = fmaf(v.w, unsc, bia[hb].w);
        } else {
          v.x += bia[hb].x; v.y += bia[hb].y; v.z += bia[hb].z; v.w += bia[hb].w;
        }
        if (relu_out) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        vv[hb] = v;
      }
      if constexpr (XM == 2) {
        // s = res + z -> uo;  y = dropout(relu_post?(LayerNorm(s)));  the statistics of s -> stats
        float4 sv[2];
        float a1 = 0.f;
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
          sv[hb] = make_float4(resR[hb].x + vv[hb].x, resR[hb].y + vv[hb].y, resR[hb].z + vv[hb].z, resR[hb].w + vv[hb].w);
          a1 += (sv[hb].x + sv[hb].y) + (sv[hb].z + sv[hb].w);
        }
        const float mean = row16_sum(a1) * (1.f / 128.f);
        float q2 = 0.f;
        float4 cv[2];
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
          cv[hb] = make_float4(sv[hb].x - mean, sv[hb].y - mean, sv[hb].z - mean, sv[hb].w - mean);
          q2 = fmaf(cv[hb].x, cv[hb].x, fmaf(cv[hb].y, cv[hb].y, fmaf(cv[hb].z, cv[hb].z, fmaf(cv[hb].w, cv[hb].w, q2))));
        }
        const float rstd = rsqrtf(row16_sum(q2) * (1.f / 128.f) + eps);
        if (live) {
          if (c == 0) *reinterpret_cast<float2*>(stats + (stage * R + lr) * 2) = make_float2(mean, rstd);
          char* ub = reinterpret_cast<char*>(uo + stage * R * lduo) + static_cast<uint32_t>(lr) * static_cast<uint32_t>(lduo) * 4u + 16u * c;
          *reinterpret_cast<float4*>(ub) = sv[0];
          *reinterpret_cast<float4*>(ub + 256) = sv[1];
        }
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
          float4 o = make_float4(fmaf(cv[hb].x * rstd, gam[hb].x, bet[hb].x), fmaf(cv[hb].y * rstd, gam[hb].y, bet[hb].y),
                                 fmaf(cv[hb].z * rstd, gam[hb].z, bet[hb].z), fmaf(cv[hb].w * rstd, gam[hb].w, bet[hb].w));
          if (relu_post) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
          if constexpr (DROP_OUT) {
            const float4 kp = keep4(seed_out, stage, hb, thr_out, keep_out);
            o.x *= kp.x; o.y *= kp.y; o.z *= kp.z; o.w *= kp.w;
          }
          if (live) *reinterpret_cast<float4*>(yb + hb * dhy + yo) = o;
        }
      }
#pragma unroll
      for (int hb = 0; hb < 2; ++hb) {
        float4 v = vv[hb];
        if constexpr (DROP_OUT && XM != 2) {
          const float4 kp = keep4(seed_out, stage, hb, thr_out, keep_out);
          v.x *= kp.x; v.y *= kp.y; v.z *= kp.z; v.w *= kp.w;
        }
        if constexpr (XM == 3 || XM == 4) vv[hb] = v;        // (packed below, once both halves of the row are final)
#ifdef ALLSET_ABL5_NOSTORE
        if (live && v.x == 123.456f)
#else
        if (live && XM != 2 && XM != 3 && XM != 4)
#endif
          *reinterpret_cast<float4*>(yb + hb * dhy + yo) = v;
        if (mask_out != nullptr) {
          // activation mask, 1 bit per element (include/allset_hip.h "mask layout"): block (row / 16, column / 64), dword
          // (row % 16, 32-column half h8), bit 8 q + (c % 8) for column 4 c + q.  A ballot's bit 16 rg + c is lane (c, rg): byte
          // (2 rg + h8) of the ballot for q is byte q of the dword of row rg, half h8 -- lane L < 8 assembles dword (rg = L >> 1,
          // h8 = L & 1); the wave's rows 4 v .. 4 v + 3 are 8 consecutive dwords of the block: one 32-byte store
          const uint64_t b0 = __ballot(v.x > 0.f), b1 = __ballot(v.y > 0.f), b2 = __ballot(v.z > 0.f), b3 = __ballot(v.w > 0.f);
          const int sh = 8 * (lane0 & 7);
          const uint32_t word = static_cast<uint32_t>((b0 >> sh) & 0xffu) | (static_cast<uint32_t>((b1 >> sh) & 0xffu) << 8) |
                                (static_cast<uint32_t>((b2 >> sh) & 0xffu) << 16) | (static_cast<uint32_t>((b3 >> sh) & 0xffu) << 24);
          if (lane0 < 8 && 16 * (wave >> 2) < nrows)         // (a 16-row block entirely past n has no words in the buffer)
            mask_out[((stage * (R / 16) + (wave >> 2)) * (ND / 64) + hb) * 32 + (wave & 3) * 8 + lane0] = word;
        }
      }
      if constexpr (XM == 3 || XM == 4) {
        // Packed row of lr (include/allset_hip_ext.h): occupancy = the BIT PATTERN is not zero (-0.0, NaN, Inf are values) -- not the
        // v > 0 ballots of the activation mask above.  The 16 lanes of a DPP row hold the row; lane c's columns 64 hb + 4 c .. + 3 are
        // nibble c % 8 of mask dword 2 hb + c / 8: an OR over the 8 lanes of a half row gives that dword (`own`), a row mirror the
        // half row's other dword (`oth`).  Position of an element = 4 + occupied columns below it.
        uint32_t u[2][4], own[2] = {0u, 0u}, oth[2] = {0u, 0u};
        int pos[2], kocc;
        const uint32_t sh = 4u * (c & 7);
        const bool hi = c >= 8;
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
          u[hb][0] = __float_as_uint(vv[hb].x); u[hb][1] = __float_as_uint(vv[hb].y);
          u[hb][2] = __float_as_uint(vv[hb].z); u[hb][3] = __float_as_uint(vv[hb].w);
        }
        if constexpr (XM == 4) {
          // Cell rows carry no mask, only ranks: the lane's counts of the two half rows ride in one register (at most 64 each: a byte
          // apiece) through one inclusive scan over the DPP row (row_shr 1, 2, 4, 8; a lane the shift leaves without a source adds 0)
          // and one butterfly sum for the totals -- 8 DPP adds where the two masks take 8 DPP moves, 6 popcounts and the nibbles.
          int n2[2];
#pragma unroll
          for (int hb = 0; hb < 2; ++hb)
            n2[hb] = ((u[hb][0] != 0u ? 1 : 0) + (u[hb][1] != 0u ? 1 : 0)) + ((u[hb][2] != 0u ? 1 : 0) + (u[hb][3] != 0u ? 1 : 0));
          const int pk = n2[0] | (n2[1] << 8);
          int inc = pk, tot = pk;
          inc += __builtin_amdgcn_update_dpp(0, inc, 0x111, 0xf, 0xf, true);
          inc += __builtin_amdgcn_update_dpp(0, inc, 0x112, 0xf, 0xf, true);
          inc += __builtin_amdgcn_update_dpp(0, inc, 0x114, 0xf, 0xf, true);
          inc += __builtin_amdgcn_update_dpp(0, inc, 0x118, 0xf, 0xf, true);
          tot += __builtin_amdgcn_update_dpp(0, tot, 0xB1, 0xf, 0xf, false);
          tot += __builtin_amdgcn_update_dpp(0, tot, 0x4E, 0xf, 0xf, false);
          tot += __builtin_amdgcn_update_dpp(0, tot, 0x141, 0xf, 0xf, false);
          tot += __builtin_amdgcn_update_dpp(0, tot, 0x140, 0xf, 0xf, false);
          const int exc = inc - pk, cnt0 = tot & 0xff;
          kocc = cnt0 + (tot >> 8);
          pos[0] = 4 + (exc & 0xff);
          pos[1] = 4 + cnt0 + (exc >> 8);
        } else {
#pragma unroll
          for (int hb = 0; hb < 2; ++hb) {
            const uint32_t nib = (u[hb][0] != 0u ? 1u : 0u) | (u[hb][1] != 0u ? 2u : 0u) | (u[hb][2] != 0u ? 4u : 0u) | (u[hb][3] != 0u ? 8u : 0u);
            float mw = __uint_as_float(nib << sh);                  // (dpp_row moves bits; nothing is computed on the float)
            mw = __uint_as_float(__float_as_uint(mw) | __float_as_uint(dpp_row<0xB1>(mw)));
            mw = __uint_as_float(__float_as_uint(mw) | __float_as_uint(dpp_row<0x4E>(mw)));
            mw = __uint_as_float(__float_as_uint(mw) | __float_as_uint(dpp_row<0x141>(mw)));
            own[hb] = __float_as_uint(mw);
            oth[hb] = __float_as_uint(dpp_row<0x140>(mw));
          }
          const uint32_t below = (1u << sh) - 1u;
          const int cnt0 = __popc(own[0]) + __popc(oth[0]);
          kocc = cnt0 + __popc(own[1]) + __popc(oth[1]);               // the row's occupied columns: uniform over its 16 lanes
          pos[0] = 4 + (hi ? __popc(oth[0]) : 0) + __popc(own[0] & below);
          pos[1] = 4 + cnt0 + (hi ? __popc(oth[1]) : 0) + __popc(own[1] & below);
        }
        // The image of the wave's four rows is built in LDS IN PLACE of their rows of ytile[k % 2]: this wave alone reads those rows
        // (every lane of it has them in vv by now -- a wave's LDS operations are served in issue order, the fence keeps the compiler
        // from moving one across), the matrix waves write the OTHER tile during this tick and this one only after the tick's barrier,
        // which this wave reaches with its image reads returned (they feed the store below).  A position is at most 4 + 127 < SPY: an
        // overflow row's tail stays inside its own tile row (only dwords 0..63 of the image leave).  No extra LDS, no extra barrier.
        uint32_t* im = reinterpret_cast<uint32_t*>(sY + (k & 1) * (R * SPY) + lr * SPY);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if constexpr (XM == 4) {
          // Cell rows, staged IN RANK ORDER: the element of rank j = pos - 4 goes to dword j of the tile row and its column to dword
          // 64 + j (one running position per half row, as in mode 3; the two stores share an address register).  Nobody reads dwords
          // kCellCap .. kCellCap + 3 or their twins 64 above: an empty column goes to the first of them, and a half row's running
          // position starts at most there (one clamp per half row, not per element), so a rank >= kCellCap lands among the four.
          // In issue order: (1) lane c writes its own three slots -- ranks c, 16 + c, 32 + c -- empty: value bits 0, dummy column
          // 128 + c; (2) the elements.  Lane c then builds cell c in registers from those six dwords (below): nothing is scattered
          // into a cell image and none is read back.
          static_assert(kCellCap == 48 && kCellCap + 3 < 64 && 64 + kCellCap + 3 < SPY, "three slots per cell; the staged columns sit 64 dwords above the values");
          const uint32_t dcol = 128u + c;
#pragma unroll
          for (int s = 0; s < 3; ++s) { im[16 * s + c] = 0u; im[64 + 16 * s + c] = dcol; }
#pragma unroll
          for (int hb = 0; hb < 2; ++hb) {
            int j = min(pos[hb] - 4, kCellCap);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const bool occ = u[hb][i] != 0u;
              const int at = occ ? j : kCellCap;
              im[at] = u[hb][i];
              im[64 + at] = static_cast<uint32_t>(64 * hb + 4 * c + i);
              j += occ ? 1 : 0;
            }
          }
        } else {
        // In issue order: (1) the 16 lanes of a row clear dwords 0..63 of its image, so that what no value overwrites leaves as zeros;
        // (2) the mask, which the lanes of the low half row hold in dword order (own, oth), to dwords 0..3 -- the high half's copy and
        // (3) the zero of every empty column go to dwords >= 64 of the row, which never leave; every element is stored, none under a
        // branch (eight exec-mask branches per stage cost more than the stores).
        *reinterpret_cast<uint4*>(im + 4 * c) = make_uint4(0u, 0u, 0u, 0u);
        *reinterpret_cast<uint4*>(im + (hi ? SPY - 4 : 0)) = make_uint4(own[0], oth[0], own[1], oth[1]);
#pragma unroll
        for (int hb = 0; hb < 2; ++hb)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const bool occ = u[hb][i] != 0u;
            im[occ ? pos[hb] : SPY - 1] = u[hb][i];
            pos[hb] += occ ? 1 : 0;
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // lane c takes dwords 4 c .. 4 c + 3 of its own row's image (cell rows: cell c = its three staged values, then their columns
        // as bytes with k on top); the wave's four rows are 1 KB contiguous: one 16-byte store per lane
        uint4 o;
        if constexpr (XM == 4)
          o = make_uint4(im[c], im[16 + c], im[32 + c], (im[64 + c] | (im[80 + c] << 8)) | ((im[96 + c] | (static_cast<uint32_t>(kocc) << 8)) << 16));
        else
          o = *reinterpret_cast<const uint4*>(im + 4 * c);
        if (live) *reinterpret_cast<uint4*>(reinterpret_cast<uint32_t*>(uo) + (stage * R + lr) * kPackPitchDw + 4 * c) = o;
        if (live && kocc > (XM == 4 ? kCellCap : kPackCap)) {              // row-uniform, rare: the row did not fit -- the gather reads it from the side table
          *reinterpret_cast<float4*>(yb + yo) = vv[0];
          *reinterpret_cast<float4*>(yb + 256 + yo) = vv[1];
        }
      }
      if constexpr (XM == 2) {
        __builtin_amdgcn_sched_barrier(0);
        request_res(k + 1);                       // the next stage's residual rows: a tick ahead of their use
        __builtin_amdgcn_sched_barrier(0);
      }
    };

    static_assert(kF2Sets == 4, "the trip below is written for four register sets");
#pragma unroll
    for (int q = 0; q < kF2Sets; ++q) request_x(q, xrS[q]);
    request_res(0);
    S0(0, xrS[0]);
    ALLSET_TICK();
    S0(1, xrS[1]);                               // tick 0 (stage 1 may be a re-run of the last stage: never consumed)
    ALLSET_TICK();
    // ticks 1 .. T - 1, four per trip (stage t + 1 lives in register set (t + 1) % 4); the last 1..3 ticks are peeled off: a
    // conditional part inside the trip makes hipcc wait vmcnt(0) at the loop header (DESIGN.md 6a''')
#define ALLSET_F2_FULL_TICK(tt, set) do { ALLSET_MARK(3); S0((tt) + 1, xrS[set]); ALLSET_MARK(0); E((tt) - 1, eC); ALLSET_MARK(1); ALLSET_TICK(); ALLSET_MARK(2); } while (0)
    int64_t t = 1;
    for (; t + 3 < T; t += 4) {
      ALLSET_F2_FULL_TICK(t, 2);
      ALLSET_F2_FULL_TICK(t + 1, 3);
      ALLSET_F2_FULL_TICK(t + 2, 0);
      ALLSET_F2_FULL_TICK(t + 3, 1);
    }
    if (t < T) ALLSET_F2_FULL_TICK(t, 2);
    if (t + 1 < T) ALLSET_F2_FULL_TICK(t + 1, 3);
    if (t + 2 < T) ALLSET_F2_FULL_TICK(t + 2, 0);
#undef ALLSET_F2_FULL_TICK
    E(T - 1, eB);                                // tick T (the last S0 staged stage T: a re-run of the last stage, never consumed)
  } else {
    // =================================================== matrix waves ===================================================
    const int m = wave - kF2VWaves;
    // this wave's slice of W^T as MFMA B fragments: output columns 32 m + 16 ct + nn, k-step t, plane pl; lane (nn = lane & 15,
    // kg = lane >> 4) holds W[column][k = 32 kg + 8 t + j], j = 0..7 (the k-order of fused_linear_fwd_x6_kernel)
    Frag wq[2][4][F16 ? 2 : 3];
    float inv_s = 1.f;                           // (fp16x3: undoes the slice's W scale and 2^Su on the way to the output tile)
    if constexpr (F16) {
      const int nn = lane0 & 15, kg = lane0 >> 4;
      float4 wa[2][4], wb[2][4];
      float amax = 0.f;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          const float4* wr = reinterpret_cast<const float4*>(W + (32 * m + 16 * ct + nn) * KD + 32 * kg + 8 * tt);
          wa[ct][tt] = wr[0]; wb[ct][tt] = wr[1];
          amax = fmaxf(fmaxf(fmaxf(fabsf(wa[ct][tt].x), fabsf(wa[ct][tt].y)), fmaxf(fabsf(wa[ct][tt].z), fabsf(wa[ct][tt].w))), amax);
          amax = fmaxf(fmaxf(fmaxf(fabsf(wb[ct][tt].x), fabsf(wb[ct][tt].y)), fmaxf(fabsf(wb[ct][tt].z), fabsf(wb[ct][tt].w))), amax);
        }
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) amax = fmaxf(amax, __shfl_xor(amax, off));
      const int ew = __builtin_amdgcn_readfirstlane(min(max(static_cast<int>(__float_as_uint(amax) >> 23), 20), 254));
      const float sw = __uint_as_float(static_cast<uint32_t>(254 + 13 - ew) << 23);       // slice maximum -> [2^13, 2^14)
      // 2^(ew - 140 - Su) as two factors (each exponent field stays valid for any ew, Su)
      const int X = ew - 140 - Su, X1 = X >> 1, X2 = X - X1;
      inv_s = __uint_as_float(static_cast<uint32_t>(127 + X1) << 23) * __uint_as_float(static_cast<uint32_t>(127 + X2) << 23);
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          const float4 a = wa[ct][tt], b = wb[ct][tt];
          uint32_t ph[4], pl[4];
          split2_f16(a.x * sw, a.y * sw, ph[0], pl[0]);
          split2_f16(a.z * sw, a.w * sw, ph[1], pl[1]);
          split2_f16(b.x * sw, b.y * sw, ph[2], pl[2]);
          split2_f16(b.z * sw, b.w * sw, ph[3], pl[3]);
          wq[ct][tt][0].u = make_uint4(ph[0], ph[1], ph[2], ph[3]);
          wq[ct][tt][1].u = make_uint4(pl[0], pl[1], pl[2], pl[3]);
        }
    } else {
      const int nn = lane0 & 15, kg = lane0 >> 4;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          const float4* wr = reinterpret_cast<const float4*>(W + (32 * m + 16 * ct + nn) * KD + 32 * kg + 8 * tt);
          const float4 a = wr[0], b = wr[1];
          uint32_t ph[4], pm[4], pl[4];
          split3_bf16(a.x, a.y, ph[0], pm[0], pl[0]);
          split3_bf16(a.z, a.w, ph[1], pm[1], pl[1]);
          split3_bf16(b.x, b.y, ph[2], pm[2], pl[2]);
          split3_bf16(b.z, b.w, ph[3], pm[3], pl[3]);
          wq[ct][tt][0].u = make_uint4(ph[0], ph[1], ph[2], ph[3]);
          wq[ct][tt][1].u = make_uint4(pm[0], pm[1], pm[2], pm[3]);
          wq[ct][tt][2].u = make_uint4(pl[0], pl[1], pl[2], pl[3]);
        }
    }
    auto S1 = [&](int64_t k) {
      ALLSET_FRESH_LANE(lane);
      const int ri = lane & 15, kg = lane >> 4;
      const uint8_t* img = sX + (k & 1) * IMG;
      float* ty = sY + (k & 1) * (R * SPY);
      constexpr int NP = F16 ? 2 : 3;
      auto load_a = [&](Frag (&f0)[3], Frag (&f1)[3], int tt) {
        const int o0 = swizzle256(ri, 64 * kg + 16 * tt), o1 = swizzle256(16 + ri, 64 * kg + 16 * tt);
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) {
          f0[pl].u = *reinterpret_cast<const uint4*>(img + pl * PLANE + o0);
          f1[pl].u = *reinterpret_cast<const uint4*>(img + pl * PLANE + o1);
        }
      };
      Frag fa0[2][3], fa1[2][3];
      f32x4 acc[2][2];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
      load_a(fa0[0], fa1[0], 0);
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        if (tt + 1 < 4) load_a(fa0[(tt + 1) & 1], fa1[(tt + 1) & 1], tt + 1);
        const Frag (&a0)[3] = fa0[tt & 1];
        const Frag (&a1)[3] = fa1[tt & 1];
        constexpr int PA_[6] = {2, 0, 1, 1, 0, 0}, PB_[6] = {0, 2, 1, 0, 1, 0};     // l.h, h.l, m.m, m.h, h.m, h.h
#ifdef ALLSET_ABL5_NOMFMA
        acc[0][0][0] += __builtin_bit_cast(float, a0[0].u.x ^ a0[1].u.y ^ a0[2].u.z); acc[1][0][0] += __builtin_bit_cast(float, a1[0].u.x ^ a1[1].u.y ^ a1[2].u.z);
        for (int pr = 0; pr < 0; ++pr) {
#else
#pragma unroll
        for (int pr = 0; pr < (F16 ? 0 : 6); ++pr) {
#endif
          if constexpr (!F16) {
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[PA_[pr]].v, wq[0][tt][PB_[pr]].v, acc[0][0], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[PA_[pr]].v, wq[0][tt][PB_[pr]].v, acc[1][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[PA_[pr]].v, wq[1][tt][PB_[pr]].v, acc[0][1], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[PA_[pr]].v, wq[1][tt][PB_[pr]].v, acc[1][1], 0, 0, 0);
          }
        }
#ifndef ALLSET_ABL5_NOMFMA
        if constexpr (F16) {
          constexpr int QA_[3] = {1, 0, 0}, QB_[3] = {0, 1, 0};     // l.h, h.l, h.h
#pragma unroll
          for (int pr = 0; pr < 3; ++pr) {
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0[QA_[pr]].h, wq[0][tt][QB_[pr]].h, acc[0][0], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[QA_[pr]].h, wq[0][tt][QB_[pr]].h, acc[1][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0[QA_[pr]].h, wq[1][tt][QB_[pr]].h, acc[0][1], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[QA_[pr]].h, wq[1][tt][QB_[pr]].h, acc[1][1], 0, 0, 0);
          }
        }
#endif
        __builtin_amdgcn_sched_barrier(0);
      }
      // acc[rt][ct][r] = y[row 16 rt + 4 kg + r][column 32 m + 16 ct + ri]
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) ty[(16 * rt + 4 * kg + r) * SPY + 32 * m + 16 * ct + ri] = F16 ? acc[rt][ct][r] * inv_s : acc[rt][ct][r];
    };
    ALLSET_TICK();
    for (int64_t k = 0; k < T; ++k) {
      ALLSET_MARK(3);
      S1(k);
      ALLSET_MARK(0);
      ALLSET_TICK();
      ALLSET_MARK(2);
    }
  }
#ifdef ALLSET_ABL5_TIMING
  // vector wave 0: [0] S0, [1] E, [2] barrier wait; matrix wave 8: [4] S1, [6] wait  (cycles, all stages) -> the first floats of y
  __syncthreads();
  if (blockIdx.x == 0 && (tid == 0 || tid == 512)) {
    float* dbg = y + (tid == 0 ? 0 : 4);
    for (int k = 0; k < 4; ++k) dbg[k] = static_cast<float>(tph[k]);
  }
#endif
}

}  // namespace allset

using namespace allset;

// 1 = the split-role forward takes this call (K = N = 128, no auxiliary columns): a pure function of its arguments
int fused_linear_fwd_roles_supported(int64_t K, int64_t N, int has_aux) {
  (void)has_aux;                 // (round 6: the plain Linear takes its four auxiliary columns along; launch_fused_linear_fwd_roles_aux)
  return (K == 128 && N == 128) ? 1 : 0;
}

// one persistent workgroup per CU
static inline unsigned f2_grid(int64_t n) {
  const int64_t blocks = (n + kF2Rows - 1) / kF2Rows;
  return static_cast<unsigned>(blocks > 256 ? 256 : (blocks < 1 ? 1 : blocks));
}

// The plain Linear (no norm, no dropout, row-major operands) with four auxiliary output columns: y = relu_out?(relu_in?(x) W^T + b),
// aux_out = relu_in?(x) aux_w^T + aux_b
int launch_fused_linear_fwd_roles_aux(hipStream_t st, const float* x, int64_t ldx, int relu_in, const float* W, const float* bias,
                                      int relu_out, float* y, int64_t ldy, int64_t n, uint32_t* mask_out, const float* aux_w,
                                      const float* aux_b, float* aux_out, int arith) {
  const unsigned grid = f2_grid(n);
#define ALLSET_F2_AUX(H16)                                                                                                             \
  fused_linear_fwd_roles_kernel<false, false, false, false, H16, 0, true><<<grid, kF2Block, 0, st>>>(                                   \
      x, ldx, nullptr, nullptr, 1e-5f, relu_in, 0.f, 0, W, bias, relu_out, 0.f, 0, y, ldy, nullptr, n, nullptr, mask_out, 0, 0, 1.f / 128.f, \
      nullptr, nullptr, 0, nullptr, 0, 0, aux_w, aux_b, aux_out)
#ifdef ALLSET_NO_F16X3
  (void)arith; ALLSET_F2_AUX(false);
#else
  if (arith != ALLSET_ARITH_BF16X6) ALLSET_F2_AUX(true); else ALLSET_F2_AUX(false);
#endif
#undef ALLSET_F2_AUX
  return 0;
}

int launch_fused_linear_fwd_roles(hipStream_t st, const float* x, int64_t ldx, const float* gamma, const float* beta, float eps,
                                  int relu_in, float p_in, uint64_t seed_in, const float* W, const float* bias, int relu_out,
                                  float p_out, uint64_t seed_out, float* y, int64_t ldy, float* stats, int64_t n,
                                  const uint64_t* seed_base, uint32_t* mask_out, int64_t xcb, int64_t ycb, float ln_inv, int arith) {
  const unsigned grid = f2_grid(n);
  // the dropout resolution is a function of p alone (common.h drop_threshold): 8 bits per element when p * 256 is an integer
  const bool d8 = drop_is8(p_in) && drop_is8(p_out);
  // fp16x3 arithmetic: behind a true LayerNorm prologue (its bound on the operand gives one scale per launch) and -- round 5 -- without
  // any norm (one scale per row, from the row's largest element); bf16x6 in the column-affine mode and on request (ALLSET_ARITH_BF16X6)
#ifdef ALLSET_NO_F16X3
  const bool f16 = false; (void)arith;
#else
  const bool f16 = arith != ALLSET_ARITH_BF16X6 && (gamma == nullptr || ln_inv != 0.f);
#endif
#define ALLSET_F2_KE(LN, DI, DO, E8, H16)                                                                                              \
  fused_linear_fwd_roles_kernel<LN, DI, DO, E8, H16><<<grid, kF2Block, 0, st>>>(x, ldx, gamma, beta, eps, relu_in, p_in, seed_in, W, bias, \
                                                                                relu_out, p_out, seed_out, y, ldy, stats, n, seed_base,   \
                                                                                mask_out, xcb, ycb, ln_inv)
#define ALLSET_F2_KD(LN, DI, DO, E8) do { if (f16) ALLSET_F2_KE(LN, DI, DO, E8, true); else ALLSET_F2_KE(LN, DI, DO, E8, false); } while (0)
#define ALLSET_F2_K(LN, DI, DO) do { if ((DI || DO) && d8) ALLSET_F2_KD(LN, DI, DO, true); else ALLSET_F2_KD(LN, DI, DO, false); } while (0)
  const int v = (gamma != nullptr ? 4 : 0) | (p_in > 0.f ? 2 : 0) | (p_out > 0.f ? 1 : 0);
  switch (v) {
    case 0: ALLSET_F2_K(false, false, false); break;
    case 1: ALLSET_F2_K(false, false, true); break;
    case 2: ALLSET_F2_K(false, true, false); break;
    case 3: ALLSET_F2_K(false, true, true); break;
    case 4: ALLSET_F2_K(true, false, false); break;
    case 5: ALLSET_F2_K(true, false, true); break;
    case 6: ALLSET_F2_K(true, true, false); break;
    default: ALLSET_F2_K(true, true, true); break;
  }
#undef ALLSET_F2_K
#undef ALLSET_F2_KD
#undef ALLSET_F2_KE
  return 0;
}

// ---- modes 3 and 4: the Linear whose output leaves as packed nonzero rows (the last f_enc Linear in front of a forward Deep Sets gather) --
// -- mask rows (XM = 3, the format segreduce_packed_kernel gathers) or cell rows (XM = 4, segreduce_cells_kernel's)
extern "C" int allset_fused_linear_fwd_packed_supported(int64_t K, int64_t N, int has_ln, float p_in, float p_out) {
  return (K == 128 && N == 128 && has_ln && p_in > 0.f && p_in < 1.f && p_out > 0.f && p_out < 1.f) ? 1 : 0;
}

extern "C" int allset_fused_linear_fwd_cells_supported(int64_t K, int64_t N, int has_ln, float p_in, float p_out) {
  return allset_fused_linear_fwd_packed_supported(K, N, has_ln, p_in, p_out);
}

// `fn`: the exported function's name for the messages; `supported`: ITS query
template <int XM>
static int fused_linear_fwd_packed_impl(const char* fn, int (*supported)(int64_t, int64_t, int, float, float), const float* x, int64_t ldx,
                                        const float* gamma, const float* beta, float eps, int relu_in, float p_in, uint64_t seed_in,
                                        const float* W, const float* bias, int relu_out, float p_out, uint64_t seed_out, void* packed,
                                        float* side, int64_t ldside, float* stats, int64_t n, int64_t K, int64_t N,
                                        const uint64_t* seed_base, uint32_t* mask_out, int arith, void* stream) {
  static_assert(XM == 3 || XM == 4, "the two packed epilogues");
  clear_error();
  ALLSET_REQUIRE(n >= 0, "%s: negative size", fn);
  ALLSET_REQUIRE(arith == ALLSET_ARITH_AUTO || arith == ALLSET_ARITH_BF16X6 || arith == ALLSET_ARITH_FP16X3,
                 "%s: arith must be ALLSET_ARITH_AUTO, ALLSET_ARITH_BF16X6 or ALLSET_ARITH_FP16X3", fn);
  if (!supported(K, N, gamma != nullptr, p_in, p_out)) {
    set_error("%s: built for K = N = 128 behind a LayerNorm with dropout in and out only (allset_%s_supported)", fn, fn);
    return ALLSET_ERR_UNSUPPORTED;
  }
#ifdef ALLSET_NO_F16X3
  if (arith == ALLSET_ARITH_FP16X3) { set_error("%s: this build has no fp16x3 arithmetic", fn); return ALLSET_ERR_UNSUPPORTED; }
#endif
  if (n == 0) return ALLSET_OK;
  ALLSET_REQUIRE(x && beta && W && packed && side && stats, "%s: null pointer", fn);
  ALLSET_REQUIRE(aligned16(x) && aligned16(side) && aligned16(W) && (reinterpret_cast<uintptr_t>(stats) & 7u) == 0,
                 "%s: x / side / W must be 16-byte aligned, stats 8-byte aligned", fn);
  ALLSET_REQUIRE((reinterpret_cast<uintptr_t>(packed) & 255u) == 0, "%s: the packed buffer must be 256-byte aligned", fn);
  ALLSET_REQUIRE(ldx >= K && ldx % 4 == 0 && ldside >= N && ldside % 4 == 0 && ldx < (1 << 24) && ldside < (1 << 24),
                 "%s: rows must be 16-byte aligned, leading dimensions below 2^24", fn);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const bool d8 = drop_is8(p_in) && drop_is8(p_out);
#ifdef ALLSET_NO_F16X3
  const bool f16 = false;
#else
  const bool f16 = arith != ALLSET_ARITH_BF16X6;
#endif
#define ALLSET_F2_PK(E8, H16)                                                                                                            \
  fused_linear_fwd_roles_kernel<true, true, true, E8, H16, XM><<<f2_grid(n), kF2Block, 0, st>>>(                                            \
      x, ldx, gamma, beta, eps, relu_in, p_in, seed_in, W, bias, relu_out, p_out, seed_out, side, ldside, stats, n, seed_base, mask_out, 0, 0, \
      1.f / 128.f, nullptr, static_cast<float*>(packed), 0)
  if (d8) { if (f16) ALLSET_F2_PK(true, true); else ALLSET_F2_PK(true, false); }
  else    { if (f16) ALLSET_F2_PK(false, true); else ALLSET_F2_PK(false, false); }
#undef ALLSET_F2_PK
  ALLSET_LAUNCH_CHECK();
  return ALLSET_OK;
}

// packed[r] = pack(dropout_{p_out}(relu_out?(dropout_{p_in}(relu_in?(LayerNorm(x)))[r] W^T + bias)));  side[r, :] = that row, dense, for
// the rows above kPackCap occupied columns ONLY (every other row of `side` is left untouched);  stats[r] = {mean, rstd};  mask_out: 1 bit
// per element > 0, as allset_fused_linear_fwd writes it.  Bit for bit what allset_fused_linear_fwd_ex + allset_pack_rows_f32 give.
extern "C" int allset_fused_linear_fwd_packed(const float* x, int64_t ldx, const float* gamma, const float* beta, float eps, int relu_in,
                                              float p_in, uint64_t seed_in, const float* W, const float* bias, int relu_out, float p_out,
                                              uint64_t seed_out, void* packed, float* side, int64_t ldside, float* stats, int64_t n,
                                              int64_t K, int64_t N, const uint64_t* seed_base, uint32_t* mask_out, int arith,
                                              void* stream) {
  return fused_linear_fwd_packed_impl<3>("fused_linear_fwd_packed", allset_fused_linear_fwd_packed_supported, x, ldx, gamma, beta, eps,
                                         relu_in, p_in, seed_in, W, bias, relu_out, p_out, seed_out, packed, side, ldside, stats, n, K, N,
                                         seed_base, mask_out, arith, stream);
}

// allset_fused_linear_fwd_packed with cells[r] = pack_cells(...) and side[r, :] written for the rows above kCellCap occupied columns ONLY.
// Bit for bit what allset_fused_linear_fwd_ex + allset_pack_cells_f32 give.
extern "C" int allset_fused_linear_fwd_cells(const float* x, int64_t ldx, const float* gamma, const float* beta, float eps, int relu_in,
                                             float p_in, uint64_t seed_in, const float* W, const float* bias, int relu_out, float p_out,
                                             uint64_t seed_out, void* cells, float* side, int64_t ldside, float* stats, int64_t n,
                                             int64_t K, int64_t N, const uint64_t* seed_base, uint32_t* mask_out, int arith,
                                             void* stream) {
  return fused_linear_fwd_packed_impl<4>("fused_linear_fwd_cells", allset_fused_linear_fwd_cells_supported, x, ldx, gamma, beta, eps,
                                         relu_in, p_in, seed_in, W, bias, relu_out, p_out, seed_out, cells, side, ldside, stats, n, K, N,
                                         seed_base, mask_out, arith, stream);
}

// ---- the PMA tail (reference layers.py:153-157) folded into its two rFF Linears: modes 1 and 2 of the kernel above (fp16x3) -------
extern "C" int allset_fused_linear_tail_supported(int64_t K, int64_t N) {
#ifdef ALLSET_NO_F16X3
  (void)K; (void)N;
  return 0;
#else
  return (K == 128 && N == 128) ? 1 : 0;
#endif
}

// uo = LayerNorm_{gamma,beta,eps}(x + colb);  y = relu_out?(uo W^T + bias);  stats[r] = {mean, rstd} of x + colb
extern "C" int allset_fused_linear_fwd_ln_side(const float* x, int64_t ldx, const float* colb, const float* gamma, const float* beta,
                                               float eps, const float* W, const float* bias, int relu_out, float* y, int64_t ldy,
                                               float* uo, int64_t lduo, float* stats, int64_t n, int64_t K, int64_t N, void* stream) {
  clear_error();
  ALLSET_REQUIRE(n >= 0, "fused_linear_fwd_ln_side: negative size");
  if (!allset_fused_linear_tail_supported(K, N)) {
    set_error("fused_linear_fwd_ln_side: built for K = N = 128 only (allset_fused_linear_tail_supported)");
    return ALLSET_ERR_UNSUPPORTED;
  }
  if (n == 0) return ALLSET_OK;
  ALLSET_REQUIRE(x && gamma && beta && W && y && uo && stats, "fused_linear_fwd_ln_side: null pointer");
  ALLSET_REQUIRE(aligned16(x) && aligned16(y) && aligned16(uo) && aligned16(W) && (reinterpret_cast<uintptr_t>(stats) & 7u) == 0,
                 "fused_linear_fwd_ln_side: x / y / uo / W must be 16-byte aligned, stats 8-byte aligned");
  ALLSET_REQUIRE(ldx >= K && ldx % 4 == 0 && ldy >= N && ldy % 4 == 0 && lduo >= K && lduo % 4 == 0 && ldx < (1 << 24) && ldy < (1 << 24) &&
                 lduo < (1 << 24), "fused_linear_fwd_ln_side: rows must be 16-byte aligned, leading dimensions below 2^24");
#ifndef ALLSET_NO_F16X3
  const hipStream_t st = static_cast<hipStream_t>(stream);
  fused_linear_fwd_roles_kernel<true, false, false, false, true, 1><<<f2_grid(n), kF2Block, 0, st>>>(
      x, ldx, gamma, beta, eps, 0, 0.f, 0, W, bias, relu_out, 0.f, 0, y, ldy, stats, n, nullptr, nullptr, 0, 0, 1.f / 128.f, colb, uo, lduo,
      nullptr, 0, 0);
  ALLSET_LAUNCH_CHECK();
#endif
  return ALLSET_OK;
}

// z = relu_out?(relu_in?(x) W^T + bias) [mask_out: 1 bit per element of z > 0];  s = res + z -> s_out;  stats[r] = {mean, rstd} of s;
// y = dropout_{p_out}(relu_post?(LayerNorm_{gamma,beta,eps}(s)))
extern "C" int allset_fused_linear_fwd_res_ln(const float* x, int64_t ldx, int relu_in, const float* W, const float* bias, int relu_out,
                                              const float* res, int64_t ldres, const float* gamma, const float* beta, float eps,
                                              int relu_post, float p_out, uint64_t seed_out, const uint64_t* seed_base, float* y,
                                              int64_t ldy, float* s_out, int64_t lds, float* stats, uint32_t* mask_out, int64_t n,
                                              int64_t K, int64_t N, void* stream) {
  clear_error();
  ALLSET_REQUIRE(n >= 0, "fused_linear_fwd_res_ln: negative size");
  ALLSET_REQUIRE(p_out >= 0.f && p_out < 1.f, "fused_linear_fwd_res_ln: dropout p must be in [0,1)");
  if (!allset_fused_linear_tail_supported(K, N)) {
    set_error("fused_linear_fwd_res_ln: built for K = N = 128 only (allset_fused_linear_tail_supported)");
    return ALLSET_ERR_UNSUPPORTED;
  }
  if (n == 0) return ALLSET_OK;
  ALLSET_REQUIRE(x && W && res && gamma && beta && y && s_out && stats, "fused_linear_fwd_res_ln: null pointer");
  ALLSET_REQUIRE(aligned16(x) && aligned16(y) && aligned16(s_out) && aligned16(res) && aligned16(W) &&
                 (reinterpret_cast<uintptr_t>(stats) & 7u) == 0,
                 "fused_linear_fwd_res_ln: x / res / y / s_out / W must be 16-byte aligned, stats 8-byte aligned");
  ALLSET_REQUIRE(ldx >= K && ldx % 4 == 0 && ldy >= N && ldy % 4 == 0 && lds >= N && lds % 4 == 0 && ldres >= N && ldres % 4 == 0 &&
                 ldx < (1 << 24) && ldy < (1 << 24) && lds < (1 << 24) && ldres < (1 << 24),
                 "fused_linear_fwd_res_ln: rows must be 16-byte aligned, leading dimensions below 2^24");
#ifndef ALLSET_NO_F16X3
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const float t8 = p_out * 256.0f;
  const bool d8 = p_out <= 0.f || t8 == floorf(t8);
#define ALLSET_F2_TB(DO, E8)                                                                                                            \
  fused_linear_fwd_roles_kernel<false, false, DO, E8, true, 2><<<f2_grid(n), kF2Block, 0, st>>>(                                          \
      x, ldx, gamma, beta, eps, relu_in, 0.f, 0, W, bias, relu_out, p_out, seed_out, y, ldy, stats, n, seed_base, mask_out, 0, 0, 0.f,    \
      nullptr, s_out, lds, res, ldres, relu_post)
  if (p_out > 0.f) { if (d8) ALLSET_F2_TB(true, true); else ALLSET_F2_TB(true, false); }
  else ALLSET_F2_TB(false, false);
#undef ALLSET_F2_TB
  ALLSET_LAUNCH_CHECK();
#endif
  return ALLSET_OK;
}
