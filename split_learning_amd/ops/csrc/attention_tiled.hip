// Tiled MFMA attention for gfx950: flash-style forward with an online softmax
// and a two-kernel recompute backward.  Any S >= 1, hd in {32, 64}, optional
// additive key bias, causal mask and in-kernel dropout; no [BH,S,S] array exists anywhere:
// the forward saves out and lse = m + log(l) ([BH,S]), the backward recomputes
// P = exp(score*scale + bias - lse) and redraws the keep mask from the offset
// the forward read (returned as a one-element device tensor, so a hipGraph
// replay's backward redraws its own forward's mask).
//
// All three kernels: 256 threads = 4 waves, one 64-row tile per block, each
// wave owns 16 rows of it, and the block walks the other axis in tiles of 64
// staged in LDS (zero-filled past S, next tile's global loads in flight under
// the MFMA phase).  Math is v_mfma_f32_16x16x4_f32 (exact fp32 products):
// lane l supplies A[i = l&15][k = l>>4] and B[k = l>>4][j = l&15] and receives
// D[i = 4*(l>>4) + r][j = l&15], r = 0..3.  Write c = l&15, g = l>>4.
//
// Forward (block = query tile, wave = 16 query rows):
//   S^T = K Q^T : A = K[16j + c][4*step + g] from LDS, B = the wave's Q rows,
//         held in registers for the whole kernel (lane: Q[row c][4*step + g]).
//         Lane l receives the scores of query row c at keys 16j + 4g + r: 16
//         scores of ONE query row per key tile, so the row max takes two
//         cross-lane steps (the four g groups) and every per-row quantity
//         (m, l, the rescale) is one scalar per lane.
//   O^T += V^T P^T : the score accumulators are used as the B operand where
//         they are.  B[k = g][j = c] wants "key k of query c"; in k-step r of
//         key block j the lane group g holds key 16j + 4g + r, so that key is
//         simply LABELLED k = g, and A reads the matching row,
//         V[16j + 4g + r][16*db + c].  A sum over keys does not care in which
//         order they are labelled, so P never leaves registers.
//         Lane l ends with O[row c][16*db + 4g + 0..3]: one float4 store.
// dq kernel: the same walk; dP^T = V gO^T (A = V rows like K, B = gO rows in
//   registers), dS^T = P^T o (dP^T - delta), dQ^T += K^T dS^T with the
//   relabelled read of K.  Also writes delta[row] = sum_d gO*O.
// dkv kernel (block = key tile, wave = 16 keys, walks query tiles): K and V
//   rows in registers as B, Q and gO staged in LDS as A: S = Q K^T and
//   dP = gO V^T give lane l key c at query rows 16i + 4g + r;
//   dV^T += gO^T P_d and dK^T += Q^T dS read gO and Q relabelled.
//   Deterministic: no atomics, no zero-fill, each output written once.
//
// Two operand layouts, one kernel body (template parameter HEADS):
//   contiguous   [BH,S,HD]: block bh reads ptr + bh*S*HD, rows HD apart.
//   head-strided [B,S,H*HD] views, as a projection GEMM writes them: element
//     (b, s, h, d) of an operand is ptr + b*batch + s*row + h*HD + d with the
//     operand's own (batch, row) strides, bh = b*heads + h.  q, k, v may be
//     three tensors or the column thirds of one packed [B,S,3E] (row = 3E);
//     out and gout are [B,S,E] as the output projection reads and writes
//     them; for packed operands gq, gk, gv are the thirds of ONE [B,S,3E]
//     gradient (dq kernel: columns [0,E), dkv kernel: [E,3E)), so each
//     element is still written exactly once and nothing is zero-filled or
//     concatenated.  lse and delta stay [BH,S] and the dropout element index
//     stays (bh*S + row)*S + key: only addresses differ, every MFMA, softmax
//     update and LDS access is the contiguous kernel's, results bit for bit.
//   b and h are block-uniform, so each operand's slice base is scalar
//   arithmetic done once (at_slice); the row stride is one more SGPR.  The
//   float4 moves need 16-byte-aligned bases and strides that are multiples
//   of 4 floats; the host checks that (at_heads_operand).
//
// Causal mode (template parameter CAUSAL; query row attends to keys <= row).
// Row tile and walked tile are both 64, so a (query tile, key tile) pair is
// fully visible (key tile < query tile), empty (key tile > query tile) or the
// diagonal.  Empty pairs are never visited: the forward and dq kernels walk
// key tiles 0..qt (prologue load, prefetch and loop bound), the dkv kernel
// walks query tiles kt..last (ldsL / ldsD staging starts there too).  Fully
// visible tiles run the non-causal body.  On the diagonal tile the mask is a
// select on registers, by tile-local position: forward and dq lanes hold
// query row 16*wid + c against keys 16j + 4g + r, the dkv lane holds key
// 16*wid + c against query rows 16i + 4g + r; an entry with key > row gets
// the score -inf before the running max (forward) or the exponent -inf (dq,
// dkv).  Its probability is then exp(-inf) = +0 exactly, and every product it
// enters (P V, dS K, P_d gO, dS Q; the operands are finite) is an exact zero
// added to an accumulator, the same zero a skipped tile leaves out: a key in
// a row's future cannot move a bit of that row's output, and gets no gradient
// from it.  No mask tensor is read and nothing is added to LDS.  Key bias and
// dropout combine unchanged: the dropout element index stays
// (bh*S + row)*S + key, so the keep decisions are the non-causal kernels'.
// Blocks carry unequal work (qt + 1 resp. ntiles - kt tiles) and take their
// (tile, bh) from the launch order level by level, heaviest level first
// (at_block); the non-causal mapping is blockIdx as before.
//
// LDS layout.  Every staged tile [64][HD] is read in two patterns by the 32
// lanes that share an LDS cycle (g in {0,1} or {2,3}; 32 banks of 4 bytes):
//   (a) row 16j + c, column C + g          (16 rows x 2 adjacent columns)
//   (b) row 16j + 4g + r, column 16*db + c (2 rows 4 apart x 16 columns)
// A padded row stride s cannot serve both: (b) needs 4s = 16 (mod 32), so
// s = 4 (mod 8), and then rows c = 0 and c = 8 of (a) share a bank.  So rows
// keep stride HD (a multiple of 32: every row starts at bank 0) and the column
// is XORed with sw(row) = 2*pi(row & 15), pi = swap bits 2 and 3:
//   (a) bank = (C + g) ^ 2*pi(c): 2*pi(c) runs over the 16 even values below
//       32 and g&1 supplies bit 0 -> 32 distinct banks;
//   (b) row & 15 = 4g + r: bit 2 of it (g&1) lands in bit 4 of sw, so the two
//       rows sit in opposite 16-bank halves and c fills each half -> 32
//       distinct banks.
// sw is even, so staged float2 pairs stay adjacent (8-byte LDS writes).
//
// Compiler resource report (hipcc --offload-arch=gfx950 -O3
// -Rpass-analysis=kernel-resource-usage), the DROPOUT and BIAS instantiation
// of each kernel (the most VGPRs of its four; the others reach the same
// occupancy, the HD=32 dq kernel 3 waves); scratch is 0 in all 24 contiguous
// instantiations:
//   kernel                      HD  VGPR  AGPR  LDS bytes  scratch  waves/SIMD
//   attn_tiled_fwd_kernel       32   104    16      16640        0      4
//   attn_tiled_fwd_kernel       64   174    16      33024        0      2
//   attn_tiled_bwd_dq_kernel    32   152    24      16640        0      2
//   attn_tiled_bwd_dq_kernel    64   195    40      33024        0      2
//   attn_tiled_bwd_dkv_kernel   32   162    32      16896        0      2
//   attn_tiled_bwd_dkv_kernel   64   244    48      33280        0      1
// The 24 head-strided instantiations (HEADS = true) report the same VGPR,
// AGPR, LDS and occupancy figures as their contiguous twins, row for row, and
// scratch 0; the contiguous ones are unchanged by the template parameter.
// The 48 causal instantiations (same command, DROPOUT and BIAS, contiguous;
// scratch 0 in all 48, the head-strided twins within 3 VGPRs and at the same
// occupancy); the 48 non-causal ones are unchanged by the template parameter:
//   kernel                      HD  VGPR  AGPR  LDS bytes  scratch  waves/SIMD
//   attn_tiled_fwd_kernel       32   112    16      16640        0      4
//   attn_tiled_fwd_kernel       64   178    16      33024        0      2
//   attn_tiled_bwd_dq_kernel    32   118    40      16640        0      3
//   attn_tiled_bwd_dq_kernel    64   200    32      33024        0      2
//   attn_tiled_bwd_dkv_kernel   32   134    44      16896        0      2
//   attn_tiled_bwd_dkv_kernel   64   232    48      33280        0      1
// The compiler spends registers on hoisted LDS addresses and batched LDS
// reads; occupancy is register-bound, not LDS-bound (160 KB per CU).
//
// The argument block, the layouts' addressing, the causal block order and the
// template dispatch live in attention_tiled.h, shared with the bf16-operand
// kernels of attention_tiled_bf16.hip; the host functions below launch those
// instead when their `bf16` argument is set (same checks, same outputs).
#include "attention_tiled.h"

namespace slk {

__device__ __forceinline__ int at_sw(int row) {
  return 2 * ((row & 3) | ((row & 4) << 1) | ((row & 8) >> 1));
}

template <int HD>
__device__ __forceinline__ int at_phys(int row, int col) {
  return row * HD + (col ^ at_sw(row));
}

__device__ __forceinline__ f32x4 at_mfma(float a, float b, f32x4 acc) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
}

// One [64][HD] tile on its way global -> registers -> LDS.  A thread moves
// HD/16 float4s; rows >= S arrive as zeros (loaded from the clamped last row
// and selected away: no load sits under a branch).
template <int HD>
struct AtTile {
  static constexpr int NV = HD / 16;
  f32x4 r[NV];
  __device__ __forceinline__ void load(AtSlice<const float> src, int row0,
                                       int S, int tid) {
    #pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int i = tid + 256 * u;
      const int row = row0 + i / (HD / 4);
      const f32x4 x = *reinterpret_cast<const f32x4*>(
          src.p + (long)min(row, S - 1) * src.ld + 4 * (i % (HD / 4)));
      r[u] = row < S ? x : f32x4{};
    }
  }
  __device__ __forceinline__ void store(float* __restrict__ lds, int tid) const {
    #pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int i = tid + 256 * u;
      const int row = i / (HD / 4), col = 4 * (i % (HD / 4));
      *reinterpret_cast<f32x2*>(&lds[at_phys<HD>(row, col)]) = f32x2{r[u].x, r[u].y};
      *reinterpret_cast<f32x2*>(&lds[at_phys<HD>(row, col + 2)]) = f32x2{r[u].z, r[u].w};
    }
  }
};

// a wave's 16 rows as the B operand: lane (c, g) holds row c, columns 4*step+g
template <int HD>
__device__ __forceinline__ void at_load_rows(float (&reg)[HD / 4],
                                             AtSlice<const float> src,
                                             int row, int S, int g) {
  const float* p = src.p + (long)min(row, S - 1) * src.ld + g;
  #pragma unroll
  for (int s = 0; s < HD / 4; ++s) reg[s] = row < S ? p[4 * s] : 0.f;
}

// acc[j] += tile[16j + c][:] . reg  (pattern (a)); four independent chains
template <int HD>
__device__ __forceinline__ void at_gemm_rows(f32x4 (&acc)[4],
                                             const float* __restrict__ lds,
                                             const float (&reg)[HD / 4], int c,
                                             int g) {
  #pragma unroll
  for (int s = 0; s < HD / 4; ++s) {
    #pragma unroll
    for (int j = 0; j < 4; ++j)
      acc[j] = at_mfma(lds[at_phys<HD>(16 * j + c, 4 * s + g)], reg[s], acc[j]);
  }
}

// acc[db] += tile[16j + 4g + r][16db + c] * w[j][r] over the tile's 64 rows
// (pattern (b): the relabelled contraction)
template <int HD>
__device__ __forceinline__ void at_gemm_relabel(f32x4 (&acc)[HD / 16],
                                                const float* __restrict__ lds,
                                                const float (&w)[4][4], int c,
                                                int g) {
  #pragma unroll
  for (int j = 0; j < 4; ++j) {
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      #pragma unroll
      for (int db = 0; db < HD / 16; ++db)
        acc[db] = at_mfma(lds[at_phys<HD>(16 * j + 4 * g + r, 16 * db + c)],
                          w[j][r], acc[db]);
    }
  }
}

template <int HD, bool DROPOUT, bool BIAS, bool HEADS, bool CAUSAL>
__global__ __launch_bounds__(256) void attn_tiled_fwd_kernel(AtArgs a) {
  __shared__ __align__(16) float ldsK[AT_TILE * HD];
  __shared__ __align__(16) float ldsV[AT_TILE * HD];
  __shared__ __align__(16) float ldsB[AT_TILE];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const AtBlock blk = at_block<CAUSAL>(true);
  const int S = a.S, bh = blk.bh, qt = blk.tile;
  const int row = qt * AT_TILE + 16 * wid + c;
  const auto qs = at_slice<HD, HEADS>(a.q, a.sq, bh, a.heads, S);
  const auto ks = at_slice<HD, HEADS>(a.k, a.sk, bh, a.heads, S);
  const auto vs = at_slice<HD, HEADS>(a.v, a.sv, bh, a.heads, S);

  uint32_t rng_stream = 0;
  if (DROPOUT) {
    const uint64_t offset = a.offset_in ? (uint64_t)a.offset_in[0] : 0;
    rng_stream = at_rng_stream(a.seed, offset);
    if (blockIdx.x == 0 && bh == 0 && tid == 0) a.offset_out[0] = (long)offset;
  }
  const float* kbr = BIAS ? a.key_bias + (long)(bh / a.heads) * S : nullptr;

  float qreg[HD / 4];
  at_load_rows<HD>(qreg, qs, row, S, g);

  f32x4 oacc[HD / 16] = {};
  float m = -INFINITY, l = 0.f;   // l: this lane's share of the row sum
  const long ridx = ((long)bh * S + row) * S;

  AtTile<HD> tk, tv;
  float nb = 0.f;
  const int ntiles = CAUSAL ? qt + 1 : (S + AT_TILE - 1) / AT_TILE;
  tk.load(ks, 0, S, tid);
  tv.load(vs, 0, S, tid);
  if (tid < AT_TILE) nb = at_key_bias<BIAS>(kbr, tid, S);

  for (int t = 0; t < ntiles; ++t) {
    __syncthreads();              // the previous tile's reads are done
    tk.store(ldsK, tid);
    tv.store(ldsV, tid);
    if (tid < AT_TILE) ldsB[tid] = nb;
    __syncthreads();
    if (t + 1 < ntiles) {
      tk.load(ks, (t + 1) * AT_TILE, S, tid);
      tv.load(vs, (t + 1) * AT_TILE, S, tid);
      if (tid < AT_TILE) nb = at_key_bias<BIAS>(kbr, (t + 1) * AT_TILE + tid, S);
    }

    f32x4 sacc[4] = {};
    at_gemm_rows<HD>(sacc, ldsK, qreg, c, g);

    float w[4][4];
    float mx = -INFINITY;
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 kb = *reinterpret_cast<const f32x4*>(&ldsB[16 * j + 4 * g]);
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        w[j][r] = sacc[j][r] * a.scale + kb[r];
        if (CAUSAL && at_hidden(t == qt, 16 * wid + c, 16 * j + 4 * g + r))
          w[j][r] = -INFINITY;
        mx = fmaxf(mx, w[j][r]);
      }
    }
    const float m_new = fmaxf(m, at_group_max(mx));
    // a tile of -inf keys leaves the max at -inf: exponents then refer to 0,
    // so they are exp(-inf) = 0 and not exp(-inf + inf) = NaN
    const float m_ref = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = expf(m - m_ref);
    m = m_new;
    float ps = 0.f;
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        float e = expf(w[j][r] - m_ref);
        ps += e;                  // the row sum takes the CLEAN probabilities
        if (DROPOUT) {
          const int key = t * AT_TILE + 16 * j + 4 * g + r;
          const bool keep =
              slk_uniform32(rng_stream, (uint32_t)(ridx + key)) >= a.p;
          e = keep ? e * a.inv_keep : 0.f;
        }
        w[j][r] = e;
      }
    }
    l = l * alpha + ps;
    #pragma unroll
    for (int db = 0; db < HD / 16; ++db) oacc[db] *= alpha;
    at_gemm_relabel<HD>(oacc, ldsV, w, c, g);
  }

  l = at_group_sum(l);
  if (row < S) {
    const float inv = 1.f / l;    // no finite key: 0/0 = NaN, as torch
    const auto os = at_slice<HD, HEADS>(a.out, a.so, bh, a.heads, S);
    float* o = os.p + (long)row * os.ld + 4 * g;
    #pragma unroll
    for (int db = 0; db < HD / 16; ++db)
      *reinterpret_cast<f32x4*>(o + 16 * db) = oacc[db] * inv;
    if (g == 0) a.lse[(long)bh * S + row] = m + logf(l);
  }
}

template <int HD, bool DROPOUT, bool BIAS, bool HEADS, bool CAUSAL>
__global__ __launch_bounds__(256) void attn_tiled_bwd_dq_kernel(AtArgs a) {
  __shared__ __align__(16) float ldsK[AT_TILE * HD];
  __shared__ __align__(16) float ldsV[AT_TILE * HD];
  __shared__ __align__(16) float ldsB[AT_TILE];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const AtBlock blk = at_block<CAUSAL>(true);
  const int S = a.S, bh = blk.bh, qt = blk.tile;
  const int row = qt * AT_TILE + 16 * wid + c;
  const auto qs = at_slice<HD, HEADS>(a.q, a.sq, bh, a.heads, S);
  const auto ks = at_slice<HD, HEADS>(a.k, a.sk, bh, a.heads, S);
  const auto vs = at_slice<HD, HEADS>(a.v, a.sv, bh, a.heads, S);
  const auto gouts = at_slice<HD, HEADS>(a.gout, a.sgo, bh, a.heads, S);

  uint32_t rng_stream = 0;
  if (DROPOUT)
    rng_stream = at_rng_stream(a.seed, a.offset_in ? (uint64_t)a.offset_in[0] : 0);
  const float* kbr = BIAS ? a.key_bias + (long)(bh / a.heads) * S : nullptr;

  float qreg[HD / 4], greg[HD / 4];
  at_load_rows<HD>(qreg, qs, row, S, g);
  at_load_rows<HD>(greg, gouts, row, S, g);
  // delta = sum_d gO * O (= sum_c dP*P, with or without dropout: O = P_d V)
  float delta = 0.f;
  {
    float oreg[HD / 4];
    at_load_rows<HD>(
        oreg, at_slice<HD, HEADS, const float>(a.out, a.so, bh, a.heads, S),
        row, S, g);
    #pragma unroll
    for (int s = 0; s < HD / 4; ++s) delta += greg[s] * oreg[s];
    delta = at_group_sum(delta);
  }
  // rows past S: any finite lse; their results are never stored
  const float lse = row < S ? a.lse[(long)bh * S + row] : 0.f;
  if (row < S && g == 0) a.delta[(long)bh * S + row] = delta;

  f32x4 dq[HD / 16] = {};
  const long ridx = ((long)bh * S + row) * S;

  AtTile<HD> tk, tv;
  float nb = 0.f;
  const int ntiles = CAUSAL ? qt + 1 : (S + AT_TILE - 1) / AT_TILE;
  tk.load(ks, 0, S, tid);
  tv.load(vs, 0, S, tid);
  if (tid < AT_TILE) nb = at_key_bias<BIAS>(kbr, tid, S);

  for (int t = 0; t < ntiles; ++t) {
    __syncthreads();
    tk.store(ldsK, tid);
    tv.store(ldsV, tid);
    if (tid < AT_TILE) ldsB[tid] = nb;
    __syncthreads();
    if (t + 1 < ntiles) {
      tk.load(ks, (t + 1) * AT_TILE, S, tid);
      tv.load(vs, (t + 1) * AT_TILE, S, tid);
      if (tid < AT_TILE) nb = at_key_bias<BIAS>(kbr, (t + 1) * AT_TILE + tid, S);
    }

    f32x4 sacc[4] = {}, dp[4] = {};
    at_gemm_rows<HD>(sacc, ldsK, qreg, c, g);
    at_gemm_rows<HD>(dp, ldsV, greg, c, g);

    float w[4][4];
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 kb = *reinterpret_cast<const f32x4*>(&ldsB[16 * j + 4 * g]);
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        // keys past S: bias -inf -> P = 0, and dP = 0 from the zero-filled V
        float x = sacc[j][r] * a.scale + kb[r] - lse;
        if (CAUSAL && at_hidden(t == qt, 16 * wid + c, 16 * j + 4 * g + r))
          x = -INFINITY;
        const float pr = expf(x);
        float d = dp[j][r];
        if (DROPOUT) {
          const int key = t * AT_TILE + 16 * j + 4 * g + r;
          const bool keep =
              slk_uniform32(rng_stream, (uint32_t)(ridx + key)) >= a.p;
          d = keep ? d * a.inv_keep : 0.f;
        }
        w[j][r] = pr * (d - delta);
      }
    }
    at_gemm_relabel<HD>(dq, ldsK, w, c, g);
  }

  if (row < S) {
    const auto gqs = at_slice<HD, HEADS>(a.gq, a.sgq, bh, a.heads, S);
    float* o = gqs.p + (long)row * gqs.ld + 4 * g;
    #pragma unroll
    for (int db = 0; db < HD / 16; ++db)
      *reinterpret_cast<f32x4*>(o + 16 * db) = dq[db] * a.scale;
  }
}

template <int HD, bool DROPOUT, bool BIAS, bool HEADS, bool CAUSAL>
__global__ __launch_bounds__(256) void attn_tiled_bwd_dkv_kernel(AtArgs a) {
  __shared__ __align__(16) float ldsQ[AT_TILE * HD];
  __shared__ __align__(16) float ldsG[AT_TILE * HD];
  __shared__ __align__(16) float ldsL[AT_TILE];   // lse rows, +inf past S
  __shared__ __align__(16) float ldsD[AT_TILE];   // delta rows

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const AtBlock blk = at_block<CAUSAL>(false);
  const int S = a.S, bh = blk.bh, kt = blk.tile;
  const int key = kt * AT_TILE + 16 * wid + c;
  const auto qs = at_slice<HD, HEADS>(a.q, a.sq, bh, a.heads, S);
  const auto ks = at_slice<HD, HEADS>(a.k, a.sk, bh, a.heads, S);
  const auto vs = at_slice<HD, HEADS>(a.v, a.sv, bh, a.heads, S);
  const auto gouts = at_slice<HD, HEADS>(a.gout, a.sgo, bh, a.heads, S);

  uint32_t rng_stream = 0;
  if (DROPOUT)
    rng_stream = at_rng_stream(a.seed, a.offset_in ? (uint64_t)a.offset_in[0] : 0);
  const float* kbr = BIAS ? a.key_bias + (long)(bh / a.heads) * S : nullptr;
  const float kb = at_key_bias<BIAS>(kbr, key, S);   // -inf: a key past S

  float kreg[HD / 4], vreg[HD / 4];
  at_load_rows<HD>(kreg, ks, key, S, g);
  at_load_rows<HD>(vreg, vs, key, S, g);

  f32x4 dk[HD / 16] = {}, dv[HD / 16] = {};

  // the tile's lse (threads 0..63) and delta (threads 64..127) rows.  A row
  // past S gets lse = +inf, so its P is exp(-inf) = 0 and it adds nothing.
  auto load_row_stat = [&](int t) -> float {
    const int r = t * AT_TILE + (tid & 63);
    if (tid < AT_TILE) return r < S ? a.lse[(long)bh * S + r] : INFINITY;
    if (tid < 2 * AT_TILE) return r < S ? a.delta[(long)bh * S + r] : 0.f;
    return 0.f;
  };

  AtTile<HD> tq, tg;
  const int ntiles = (S + AT_TILE - 1) / AT_TILE;
  const int t0 = CAUSAL ? kt : 0;   // query tiles above the diagonal see no key here
  tq.load(qs, t0 * AT_TILE, S, tid);
  tg.load(gouts, t0 * AT_TILE, S, tid);
  float ns = load_row_stat(t0);

  for (int t = t0; t < ntiles; ++t) {
    __syncthreads();
    tq.store(ldsQ, tid);
    tg.store(ldsG, tid);
    if (tid < AT_TILE) ldsL[tid] = ns;
    else if (tid < 2 * AT_TILE) ldsD[tid - AT_TILE] = ns;
    __syncthreads();
    if (t + 1 < ntiles) {
      tq.load(qs, (t + 1) * AT_TILE, S, tid);
      tg.load(gouts, (t + 1) * AT_TILE, S, tid);
      ns = load_row_stat(t + 1);
    }

    f32x4 sacc[4] = {}, dp[4] = {};
    at_gemm_rows<HD>(sacc, ldsQ, kreg, c, g);
    at_gemm_rows<HD>(dp, ldsG, vreg, c, g);

    float pd[4][4], ds[4][4];
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f32x4 L = *reinterpret_cast<const f32x4*>(&ldsL[16 * i + 4 * g]);
      const f32x4 D = *reinterpret_cast<const f32x4*>(&ldsD[16 * i + 4 * g]);
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        float x = sacc[i][r] * a.scale + kb - L[r];
        if (CAUSAL && at_hidden(t == kt, 16 * i + 4 * g + r, 16 * wid + c))
          x = -INFINITY;
        const float pr = expf(x);
        float d = dp[i][r], pk = pr;
        if (DROPOUT) {
          const int row = t * AT_TILE + 16 * i + 4 * g + r;
          const bool keep = slk_uniform32(
              rng_stream, (uint32_t)(((long)bh * S + row) * S + key)) >= a.p;
          d = keep ? d * a.inv_keep : 0.f;
          pk = keep ? pr * a.inv_keep : 0.f;
        }
        pd[i][r] = pk;
        ds[i][r] = pr * (d - D[r]);
      }
    }
    at_gemm_relabel<HD>(dv, ldsG, pd, c, g);
    at_gemm_relabel<HD>(dk, ldsQ, ds, c, g);
  }

  if (key < S) {
    const auto gvs = at_slice<HD, HEADS>(a.gv, a.sgv, bh, a.heads, S);
    const auto gks = at_slice<HD, HEADS>(a.gk, a.sgk, bh, a.heads, S);
    float* ov = gvs.p + (long)key * gvs.ld + 4 * g;
    float* ok = gks.p + (long)key * gks.ld + 4 * g;
    #pragma unroll
    for (int db = 0; db < HD / 16; ++db) {
      *reinterpret_cast<f32x4*>(ov + 16 * db) = dv[db];
      *reinterpret_cast<f32x4*>(ok + 16 * db) = dk[db] * a.scale;
    }
  }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------

// [BH,S,hd] fp32 cuda, contiguous, 16-byte aligned (the kernels move float4s)
static at::Tensor at_operand(const at::Tensor& t, const at::Tensor& like,
                             const char* who, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.dim() == 3, who,
              ": ", name, " must be a float32 cuda tensor [BH,S,hd]");
  TORCH_CHECK(t.device() == like.device() && t.sizes() == like.sizes(), who,
              ": ", name, " must have q's shape and device");
  auto tc = t.contiguous();
  if ((reinterpret_cast<uintptr_t>(tc.data_ptr()) & 15) != 0) tc = tc.clone();
  return tc;
}

// the rules both layouts share, on the problem's (BH, S, hd)
static AtProblem at_check_dims(const at::Tensor& q, long BH, long S, long hd,
                               double p,
                               const c10::optional<at::Tensor>& offset,
                               const c10::optional<at::Tensor>& key_bias,
                               int64_t heads, const char* who) {
  AtProblem pr;
  pr.causal = false;
  pr.BH = BH;
  TORCH_CHECK(S >= 1 && S < (1 << 24), who, ": S=", S, " out of range");
  pr.S = (int)S;
  pr.hd = (int)hd;
  TORCH_CHECK(pr.hd == 32 || pr.hd == 64, who, ": hd must be 32 or 64 (got ",
              hd, ")");
  TORCH_CHECK(pr.BH <= 65535, who, ": BH=", pr.BH, " exceeds the grid's 65535");
  TORCH_CHECK(p >= 0.0 && p < 1.0, who, ": p in [0,1) (got ", p, ")");
  pr.drop = p > 0.0;
  pr.bias = key_bias.has_value();
  if (pr.bias) {
    TORCH_CHECK(key_bias->device() == q.device(), who,
                ": key_bias must be on q's device");
    pr.kb = check_key_bias(*key_bias, pr.BH, pr.S, heads, who);
  }
  if (pr.drop && offset.has_value()) {
    TORCH_CHECK(offset->is_cuda() && offset->device() == q.device() &&
                    offset->scalar_type() == at::kLong && offset->numel() == 1,
                who, ": offset must be a one-element int64 tensor on q's device");
    pr.off = offset->contiguous();
  }
  return pr;
}

static AtProblem at_check(const at::Tensor& q, double p,
                          const c10::optional<at::Tensor>& offset,
                          const c10::optional<at::Tensor>& key_bias,
                          int64_t heads, const char* who) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kFloat && q.dim() == 3, who,
              ": q must be a float32 cuda tensor [BH,S,hd]");
  return at_check_dims(q, q.size(0), q.size(1), q.size(2), p, offset, key_bias,
                       heads, who);
}

static AtArgs at_args(const AtProblem& pr, const at::Tensor& q,
                      const at::Tensor& k, const at::Tensor& v, double scale,
                      double p, int64_t seed, int64_t heads) {
  AtArgs a = {};
  a.q = q.data_ptr<float>();
  a.k = k.data_ptr<float>();
  a.v = v.data_ptr<float>();
  a.key_bias = pr.bias ? pr.kb.data_ptr<float>() : nullptr;
  a.offset_in = pr.off.defined() ? pr.off.data_ptr<long>() : nullptr;
  a.seed = pr.drop ? (uint64_t)seed : 0;
  a.S = pr.S;
  a.heads = (int)heads;
  a.scale = (float)scale;
  a.p = pr.drop ? (float)p : 0.f;
  a.inv_keep = pr.drop ? (float)(1.0 / (1.0 - p)) : 1.f;
  return a;
}

// -> {out [BH,S,hd], lse [BH,S], offset_used [1] int64 (empty when p == 0)}
std::vector<at::Tensor> attn_tiled_fwd(const at::Tensor& q, const at::Tensor& k,
                                       const at::Tensor& v, double scale,
                                       double p, int64_t seed,
                                       c10::optional<at::Tensor> offset,
                                       c10::optional<at::Tensor> key_bias,
                                       int64_t heads, bool is_causal,
                                       bool bf16) {
  const char* who = "attn_tiled_fwd";
  AtProblem pr = at_check(q, p, offset, key_bias, heads, who);
  pr.causal = is_causal;
  auto qc = at_operand(q, q, who, "q"), kc = at_operand(k, q, who, "k"),
       vc = at_operand(v, q, who, "v");
  auto out = at::empty_like(qc);
  auto lse = at::empty({pr.BH, pr.S}, qc.options());
  auto used = at::empty({pr.drop ? 1 : 0}, qc.options().dtype(at::kLong));
  if (pr.BH == 0) return {out, lse, used};
  AtArgs a = at_args(pr, qc, kc, vc, scale, p, seed, heads);
  a.out = out.data_ptr<float>();
  a.lse = lse.data_ptr<float>();
  a.offset_out = pr.drop ? used.data_ptr<long>() : nullptr;
  const dim3 grid(ceil_div(pr.S, AT_TILE), (unsigned)pr.BH);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  if (bf16) at_bf16_fwd(false, pr, grid, stream, a);
  else SLK_AT_DISPATCH(attn_tiled_fwd_kernel, false, pr, grid, stream, a);
  return {out, lse, used};
}

// -> {gq, gk, gv}; offset is the tensor attn_tiled_fwd returned
std::vector<at::Tensor> attn_tiled_bwd(const at::Tensor& gout, const at::Tensor& q,
                                       const at::Tensor& k, const at::Tensor& v,
                                       const at::Tensor& out, const at::Tensor& lse,
                                       double scale, double p, int64_t seed,
                                       c10::optional<at::Tensor> offset,
                                       c10::optional<at::Tensor> key_bias,
                                       int64_t heads, bool is_causal,
                                       bool bf16) {
  const char* who = "attn_tiled_bwd";
  if (offset.has_value() && offset->numel() == 0) offset = c10::nullopt;
  AtProblem pr = at_check(q, p, offset, key_bias, heads, who);
  pr.causal = is_causal;
  TORCH_CHECK(!pr.drop || pr.off.defined(), who,
              ": p > 0 needs the offset tensor the forward returned");
  auto qc = at_operand(q, q, who, "q"), kc = at_operand(k, q, who, "k"),
       vc = at_operand(v, q, who, "v"), oc = at_operand(out, q, who, "out"),
       gc = at_operand(gout, q, who, "gout");
  TORCH_CHECK(lse.is_cuda() && lse.device() == q.device() &&
                  lse.scalar_type() == at::kFloat && lse.dim() == 2 &&
                  lse.size(0) == pr.BH && lse.size(1) == pr.S,
              who, ": lse must be a float32 cuda tensor [BH,S]");
  auto lc = lse.contiguous();
  auto gq = at::empty_like(qc), gk = at::empty_like(qc), gv = at::empty_like(qc);
  if (pr.BH == 0) return {gq, gk, gv};
  auto delta = at::empty_like(lc);
  AtArgs a = at_args(pr, qc, kc, vc, scale, p, seed, heads);
  a.out = oc.data_ptr<float>();
  a.lse = lc.data_ptr<float>();
  a.gout = gc.data_ptr<float>();
  a.delta = delta.data_ptr<float>();
  a.gq = gq.data_ptr<float>();
  a.gk = gk.data_ptr<float>();
  a.gv = gv.data_ptr<float>();
  const dim3 grid(ceil_div(pr.S, AT_TILE), (unsigned)pr.BH);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  if (bf16) at_bf16_bwd_dq(false, pr, grid, stream, a);
  else SLK_AT_DISPATCH(attn_tiled_bwd_dq_kernel, false, pr, grid, stream, a);
  // same stream: delta is complete before the dkv kernel starts
  if (bf16) at_bf16_bwd_dkv(false, pr, grid, stream, a);
  else SLK_AT_DISPATCH(attn_tiled_bwd_dkv_kernel, false, pr, grid, stream, a);
  return {gq, gk, gv};
}

// ---------------------------------------------------------------------------
// head-strided layout: operands are [B,S,E = heads*hd] views with a unit last
// stride, read where the projection GEMM left them
// ---------------------------------------------------------------------------

// the float4 loads and stores need a 16-byte-aligned base and row and batch
// strides that keep that alignment; a dimension of size 1 is never stepped
static AtStride at_heads_operand(const at::Tensor& t, const at::Tensor& like,
                                 const char* who, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.dim() == 3, who,
              ": ", name, " must be a float32 cuda tensor [B,S,E]");
  TORCH_CHECK(t.device() == like.device() && t.sizes() == like.sizes(), who,
              ": ", name, " must have q's shape (B, S, E) and device");
  TORCH_CHECK(t.stride(2) == 1, who, ": ", name,
              " must have a last-dim stride of 1 (got ", t.stride(2), ")");
  const long rs = t.size(1) > 1 ? t.stride(1) : 0;
  const long bs = t.size(0) > 1 ? t.stride(0) : 0;
  TORCH_CHECK(rs % 4 == 0 && bs % 4 == 0 && rs < (1L << 31), who, ": ", name,
              "'s row and batch strides (", rs, ", ", bs,
              ") must be multiples of 4 floats: the kernels move float4s");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0, who, ": ",
              name, " must start at a 16-byte-aligned address");
  return {bs, (int)rs};
}

static AtProblem at_heads_check(const at::Tensor& q, int64_t heads, double p,
                                const c10::optional<at::Tensor>& offset,
                                const c10::optional<at::Tensor>& key_bias,
                                const char* who) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kFloat && q.dim() == 3, who,
              ": q must be a float32 cuda tensor [B,S,E]");
  TORCH_CHECK(heads >= 1 && q.size(2) % heads == 0, who, ": E=", q.size(2),
              " is not heads=", heads, " times a head size");
  return at_check_dims(q, q.size(0) * heads, q.size(1), q.size(2) / heads, p,
                       offset, key_bias, heads, who);
}

// q, k, v are the column slices [0,E), [E,2E), [2E,3E) of one dense [B,S,3E]
static bool at_heads_packed(const at::Tensor& q, const at::Tensor& k,
                            const at::Tensor& v) {
  const long B = q.size(0), S = q.size(1), E = q.size(2);
  return q.is_alias_of(k) && q.is_alias_of(v) && k.strides() == q.strides() &&
         v.strides() == q.strides() &&
         k.storage_offset() == q.storage_offset() + E &&
         v.storage_offset() == q.storage_offset() + 2 * E &&
         (S == 1 || q.stride(1) == 3 * E) && (B == 1 || q.stride(0) == S * 3 * E);
}

// -> {out [B,S,E], lse [B*heads,S], offset_used [1] int64 (empty when p == 0)}
std::vector<at::Tensor> attn_heads_fwd(const at::Tensor& q, const at::Tensor& k,
                                       const at::Tensor& v, int64_t heads,
                                       double scale, double p, int64_t seed,
                                       c10::optional<at::Tensor> offset,
                                       c10::optional<at::Tensor> key_bias,
                                       bool is_causal, bool bf16) {
  const char* who = "attn_heads_fwd";
  AtProblem pr = at_heads_check(q, heads, p, offset, key_bias, who);
  pr.causal = is_causal;
  auto out = at::empty(q.sizes(), q.options());
  auto lse = at::empty({pr.BH, pr.S}, q.options());
  auto used = at::empty({pr.drop ? 1 : 0}, q.options().dtype(at::kLong));
  AtArgs a = at_args(pr, q, k, v, scale, p, seed, heads);
  a.sq = at_heads_operand(q, q, who, "q");
  a.sk = at_heads_operand(k, q, who, "k");
  a.sv = at_heads_operand(v, q, who, "v");
  a.so = at_heads_operand(out, q, who, "out");
  if (pr.BH == 0) return {out, lse, used};
  a.out = out.data_ptr<float>();
  a.lse = lse.data_ptr<float>();
  a.offset_out = pr.drop ? used.data_ptr<long>() : nullptr;
  const dim3 grid(ceil_div(pr.S, AT_TILE), (unsigned)pr.BH);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  if (bf16) at_bf16_fwd(true, pr, grid, stream, a);
  else SLK_AT_DISPATCH(attn_tiled_fwd_kernel, true, pr, grid, stream, a);
  return {out, lse, used};
}

// -> {gq, gk, gv} in q's layout class: for q, k, v packed in one [B,S,3E]
// tensor, three views of ONE [B,S,3E] gradient, which is returned as a fourth
// element (dq kernel writes columns [0,E), dkv kernel [E,3E): every element
// once, nothing zero-filled or concatenated); otherwise three dense [B,S,E]
std::vector<at::Tensor> attn_heads_bwd(const at::Tensor& gout, const at::Tensor& q,
                                       const at::Tensor& k, const at::Tensor& v,
                                       const at::Tensor& out, const at::Tensor& lse,
                                       int64_t heads, double scale, double p,
                                       int64_t seed,
                                       c10::optional<at::Tensor> offset,
                                       c10::optional<at::Tensor> key_bias,
                                       bool is_causal, bool bf16) {
  const char* who = "attn_heads_bwd";
  if (offset.has_value() && offset->numel() == 0) offset = c10::nullopt;
  AtProblem pr = at_heads_check(q, heads, p, offset, key_bias, who);
  pr.causal = is_causal;
  TORCH_CHECK(!pr.drop || pr.off.defined(), who,
              ": p > 0 needs the offset tensor the forward returned");
  TORCH_CHECK(lse.is_cuda() && lse.device() == q.device() &&
                  lse.scalar_type() == at::kFloat && lse.dim() == 2 &&
                  lse.size(0) == pr.BH && lse.size(1) == pr.S,
              who, ": lse must be a float32 cuda tensor [B*heads,S]");
  auto lc = lse.contiguous();
  // the incoming gradient is autograd's, not the caller's: take any layout
  // the kernels can read, copy the rest
  TORCH_CHECK(gout.dim() == 3 && gout.sizes() == q.sizes(), who,
              ": gout must have q's shape (B, S, E)");
  const bool g_ok = gout.stride(2) == 1 && gout.stride(1) % 4 == 0 &&
                    gout.stride(0) % 4 == 0 &&
                    (reinterpret_cast<uintptr_t>(gout.data_ptr()) & 15) == 0;
  auto gc = g_ok ? gout : gout.contiguous();
  const long B = q.size(0), E = q.size(2);
  AtArgs a = at_args(pr, q, k, v, scale, p, seed, heads);
  a.sq = at_heads_operand(q, q, who, "q");
  a.sk = at_heads_operand(k, q, who, "k");
  a.sv = at_heads_operand(v, q, who, "v");
  a.so = at_heads_operand(out, q, who, "out");
  a.sgo = at_heads_operand(gc, q, who, "gout");
  std::vector<at::Tensor> g;
  if (at_heads_packed(q, k, v)) {
    auto packed = at::empty({B, pr.S, 3 * E}, q.options());
    g = {packed.narrow(2, 0, E), packed.narrow(2, E, E),
         packed.narrow(2, 2 * E, E), packed};
  } else {
    g = {at::empty(q.sizes(), q.options()), at::empty(q.sizes(), q.options()),
         at::empty(q.sizes(), q.options())};
  }
  if (pr.BH == 0) return g;
  a.sgq = at_heads_operand(g[0], q, who, "gq");
  a.sgk = at_heads_operand(g[1], q, who, "gk");
  a.sgv = at_heads_operand(g[2], q, who, "gv");
  auto delta = at::empty_like(lc);
  a.out = out.data_ptr<float>();
  a.lse = lc.data_ptr<float>();
  a.gout = gc.data_ptr<float>();
  a.delta = delta.data_ptr<float>();
  a.gq = g[0].data_ptr<float>();
  a.gk = g[1].data_ptr<float>();
  a.gv = g[2].data_ptr<float>();
  const dim3 grid(ceil_div(pr.S, AT_TILE), (unsigned)pr.BH);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  if (bf16) at_bf16_bwd_dq(true, pr, grid, stream, a);
  else SLK_AT_DISPATCH(attn_tiled_bwd_dq_kernel, true, pr, grid, stream, a);
  // same stream: delta is complete before the dkv kernel starts
  if (bf16) at_bf16_bwd_dkv(true, pr, grid, stream, a);
  else SLK_AT_DISPATCH(attn_tiled_bwd_dkv_kernel, true, pr, grid, stream, a);
  return g;
}

}  // namespace slk
