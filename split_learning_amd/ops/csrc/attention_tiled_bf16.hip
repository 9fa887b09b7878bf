// bf16-operand tiled attention for gfx950: the forward, dq and dkv kernels of
// attention_tiled.hip with bf16 MFMA operands.  Same contract (any S >= 1, hd
// in {32, 64}, contiguous [BH,S,hd] or head-strided [B,S,H*hd] operands
// including the packed [B,S,3E] one, key bias, causal tile skipping, in-kernel
// dropout at element index (bh*S + row)*S + key, used offset as a device
// tensor, no atomics, no S^2 array), same host functions (their `bf16`
// argument), same grid, block order and saved state.  Tensors in memory stay
// fp32; an operand is rounded to bf16 (v_cvt_pk_bf16_f32: nearest even, NaN
// and inf kept) once, between its global load and LDS or its register home.
//
// What is rounded (x_b = x rounded to bf16); everything else is fp32:
//   forward   s = scale * (q_b . k_b) + bias, exact products, fp32 sum.  The
//             online softmax is fp32; l and lse = m + log l take the UNROUNDED
//             tile probabilities; the probabilities after the dropout select
//             are rounded as the operand of P . v_b.  Accumulators, rescale,
//             divide and store are fp32.
//   backward  P = exp(s - lse) in fp32, dP = gO_b . v_b,
//             delta = sum_d gO_b * out in fp32 (the rounded gO: the whole
//             backward is the gradient at upstream gO_b),
//             dS = P o (dP_dropped - delta) in fp32, rounded as the operand of
//             dS . k_b (dq) and dS^T . q_b (dk); the dropped P is rounded as
//             the operand of P_d^T . gO_b (dv).
//
// Work split: as the fp32 kernels.  256 threads = 4 waves, one 64-row tile per
// block (query rows in forward and dq, keys in dkv), a wave owns 16 rows of
// it, the block walks the other axis in tiles of 64 staged in LDS, the next
// tile's global loads in flight under the MFMA phase.  c = lane & 15,
// g = lane >> 4.
//
// One instruction does all the math: v_mfma_f32_16x16x32_bf16.  Lane l
// supplies A[i = c][k = 8g .. 8g+7] and B[k = 8g .. 8g+7][j = c], eight
// consecutive k in four VGPRs, and receives D[i = 4g + r][j = c], r = 0..3.
//
//   Products that reduce over d (scores S^T = K Q^T, dP^T = V gO^T; in dkv
//   S = Q K^T, dP = gO V^T): B is the wave's own rows, converted once and held
//   in registers for the whole kernel (lane: row c, d = 32 step + 8g .. +7, so
//   HD/32 x 4 VGPRs per operand against the fp32 kernels' HD/4).  A is a row
//   of the walked tile, read from a row-major bf16 tile [64][HD + 8] as one
//   ds_read_b128 (row 16j + c, d = 32 step + 8g .. +7).  HD/32 MFMAs per 16
//   walked rows where the fp32 kernels issue HD/4.  As there, the lane ends
//   with the 16 entries (16j + 4g + r, r = 0..3, j = 0..3) of ONE own row c,
//   so the softmax statistics are one scalar per lane and two shuffles.
//
//   Products that reduce over the walked axis (O^T += V^T P^T, dQ^T += K^T
//   dS^T, dV^T += gO^T P_d, dK^T += Q^T dS): the accumulator entries
//   D[4g + r] of block j are four consecutive walked rows 16j + 4g + r, and
//   the B operand wants consecutive k from lane group g: so the lane packs
//   blocks j = 2h and 2h + 1 into one operand, k = 8g + e LABELLING walked row
//   16(2h) + 4g + e for e < 4 and 16(2h+1) + 4g + e - 4 for e >= 4.  A sum
//   over the walked rows does not care how they are labelled as long as A
//   uses the same labels: A reads, for output column d = 16 db + c, the same
//   two runs of four walked rows.  That needs four consecutive walked rows at
//   one column: a TRANSPOSED bf16 tile [HD][64 + 4], written transposed by
//   the staging store, read as two ds_read_b64.  P and dS go from accumulator
//   to operand with a pack and never leave registers.  Two MFMAs per 16
//   output columns per walked tile where the fp32 kernels issue 16.
//
//   So forward stages K row-major and V transposed; dq K both ways and V
//   row-major; dkv Q and gO both ways.  A thread stages a key pair: rows
//   2p, 2p + 1 at columns 4cg .. 4cg+3, two float4 loads per operand (rows
//   past S load the clamped last row and select zeros), converted at once so
//   the prefetch registers hold bf16: 4 VGPRs per pair against 8.  Row-major
//   store: two ds_write_b64.  Transposed store: four ds_write_b32, one per
//   column, each holding the pair (2p, 2p + 1).
//
// LDS banks (4-byte banks; a read of w dwords per lane is served 64/w lanes at
// a time when the array moves 64 dwords per clock, 32/w when it moves 32).
//   * row-major b128 reads: row stride HD + 8 bf16 = 36 (HD 64) or 20 (HD 32)
//     dwords = 9 or 5 sixteen-byte slots.  The 16 lanes of one g read rows
//     16j + c at a fixed column: slots 9c or 5c mod 16 (or mod 8), an odd
//     multiplier, so 16 (8) consecutive rows take distinct slots.  No
//     conflict in either model.
//   * transposed b64 reads: row stride 64 + 4 bf16 = 34 dwords.  Lanes (c, g)
//     read dwords 34c + 2g + {0, 1} (+ const).  16 lanes of one g: 34c mod 32
//     = 2c, 16 distinct even banks, no conflict.  32 lanes (g and g + 1) in a
//     64-bank array: (17c + g) mod 32 collides once (c = 15, g odd against
//     c = 0, g even): one 2-way conflict per read.  No stride serves both
//     models exactly (c t + g = c' t mod 32 always has a solution with
//     |c - c'| < 16 for odd t, and even t fails the 16-lane case).
//   * transposed b32 stores: dword (4cg + jj) * 34 + p = 8cg + 2jj + p (mod
//     32); the thread map (AbTile::unit) gives 32 consecutive lanes cg & 3 =
//     lane & 3 and p & 7 = (lane >> 2) & 7: 32 distinct banks.
//   * row-major b64 stores: dword 2p * (36 or 20) + 2cg = 8p + 2cg (mod 32)
//     over p & 7, cg & 3: 2-way conflicts, not removed: these are 2 of the 6
//     staging stores per unit and the staging phase is short against the
//     MFMA phase it precedes.
//
// Edges: rows past S stage as zeros and carry bias -inf (forward, dq: P = 0)
// or lse = +inf (dkv: P = 0); their own results are never stored.  A key
// whose bias is -inf has P = exp(-inf) = +0 exactly, a bf16 +0 operand.  An
// all-masked row has m = -inf, l = 0 and out = 0/0 = NaN, as the fp32
// kernels.  Causal: attention_tiled.hip's rule unchanged (tiles above the
// diagonal are not visited; the diagonal tile's hidden entries get -inf
// before the max or the exponent).
//
// Build flags: this file takes build.py's _NO_PK_F32 like its fp32 twin.
// Compiled both ways, every instantiation has scratch 0 and the same
// occupancy; without packed fp32 ops (v_pk_mul_f32 and kin for the float4
// rescales) the hd = 64 forward and dq kernels take 1 to 6 VGPRs fewer and
// the dkv kernel 2 more.  Nothing is gained by packing, so the file keeps its
// twin's flag and its twin's scalar fp32 instruction mix.
//
// Compiler resource report (hipcc --offload-arch=gfx950 -O3
// -Rpass-analysis=kernel-resource-usage, with _NO_PK_F32), the DROPOUT and
// BIAS instantiation of each kernel, contiguous layout, not causal / causal;
// scratch is 0 in all 96 instantiations, and the head-strided twins are
// within 5 VGPRs of these and at the same occupancy:
//   kernel                          HD   VGPR      AGPR    LDS bytes  waves/SIMD
//   attn_tiled_bf16_fwd_kernel      32   72 /  76  12 / 16      9728    5 / 5
//   attn_tiled_bf16_fwd_kernel      64   97 / 102  16 / 16     18176    4 / 4
//   attn_tiled_bf16_bwd_dq_kernel   32   82 /  75  28 / 28     14848    4 / 4
//   attn_tiled_bf16_bwd_dq_kernel   64  134 / 128  28 / 32     27392    3 / 3
//   attn_tiled_bf16_bwd_dkv_kernel  32  116 /  96  28 / 28     19456    3 / 4
//   attn_tiled_bf16_bwd_dkv_kernel  64  162 / 146  40 / 44     36352    2 / 2
// Against the fp32 kernels at hd = 64 (174 / 195 / 244 VGPRs, 2 / 2 / 1
// waves): forward 4, dq 3, dkv 2 waves per SIMD.  LDS: the forward's is 55 %
// of the fp32 kernels' 33 KB; dq (three tiles) 83 %; dkv, which needs Q and
// gO in both orientations, 110 %.  Occupancy stays register-bound: 160 KB of
// LDS per CU hold four dkv blocks.
#include "attention_tiled.h"

namespace slk {
namespace {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

constexpr int AB_LDT = AT_TILE + 4;   // bf16 per row of a transposed tile

template <int HD>
constexpr int ab_ldr() { return HD + 8; }   // bf16 per row of a row-major tile

// two floats -> one dword of two bf16 (nearest even, NaN and inf kept); lo is
// the lower index
__device__ __forceinline__ unsigned ab_pack(float lo, float hi) {
  const bf16x2 v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(unsigned, v);
}

__device__ __forceinline__ u32x2 ab_pack4(f32x4 x) {
  return u32x2{ab_pack(x.x, x.y), ab_pack(x.z, x.w)};
}

__device__ __forceinline__ f32x4 ab_mfma(u32x4 a, u32x4 b, f32x4 acc) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(
      __builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
}

// bf16 element e of a packed row, back as fp32 (exact)
__device__ __forceinline__ float ab_elem(const u32x4& x, int e) {
  const unsigned w = x[e >> 1];
  return __uint_as_float((e & 1) ? (w & 0xffff0000u) : (w << 16));
}

// One [64][HD] tile on its way global -> registers (bf16) -> LDS.  A thread
// moves HD/32 units; a unit is rows 2p, 2p + 1 at columns 4cg .. 4cg + 3.
template <int HD>
struct AbTile {
  static constexpr int NU = HD / 32;
  static constexpr int CGB = HD == 64 ? 2 : 1;   // log2(HD / 16)
  u32x2 lo[NU], hi[NU];   // row 2p and row 2p + 1

  // unit u -> column group cg (0 .. HD/4 - 1) and row pair p (0 .. 31): a
  // bijection whose low five bits are cg & 3 and p & 7 (the bank argument)
  static __device__ __forceinline__ int unit_cg(int u) {
    return (u & 3) | (((u >> 5) & (HD / 16 - 1)) << 2);
  }
  static __device__ __forceinline__ int unit_p(int u) {
    return ((u >> 2) & 7) | ((u >> (5 + CGB)) << 3);
  }

  __device__ __forceinline__ void load(AtSlice<const float> src, int row0,
                                       int S, int tid) {
    #pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int unit = tid + 256 * u;
      const int row = row0 + 2 * unit_p(unit);
      const float* p = src.p + 4 * unit_cg(unit);
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(
          p + (long)min(row, S - 1) * src.ld);
      const f32x4 x1 = *reinterpret_cast<const f32x4*>(
          p + (long)min(row + 1, S - 1) * src.ld);
      lo[u] = ab_pack4(row < S ? x0 : f32x4{});
      hi[u] = ab_pack4(row + 1 < S ? x1 : f32x4{});
    }
  }
  // as [row][d], rows ab_ldr<HD>() apart
  __device__ __forceinline__ void store_rows(__bf16* __restrict__ lds,
                                             int tid) const {
    #pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int unit = tid + 256 * u;
      __bf16* at = lds + 2 * unit_p(unit) * ab_ldr<HD>() + 4 * unit_cg(unit);
      *reinterpret_cast<u32x2*>(at) = lo[u];
      *reinterpret_cast<u32x2*>(at + ab_ldr<HD>()) = hi[u];
    }
  }
  // as [d][row], rows AB_LDT apart
  __device__ __forceinline__ void store_cols(__bf16* __restrict__ lds,
                                             int tid) const {
    unsigned* l32 = reinterpret_cast<unsigned*>(lds);
    #pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int unit = tid + 256 * u;
      unsigned* at = l32 + 4 * unit_cg(unit) * (AB_LDT / 2) + unit_p(unit);
      #pragma unroll
      for (int h = 0; h < 2; ++h) {
        at[(2 * h) * (AB_LDT / 2)] = (lo[u][h] & 0xffffu) | (hi[u][h] << 16);
        at[(2 * h + 1) * (AB_LDT / 2)] =
            (lo[u][h] >> 16) | (hi[u][h] & 0xffff0000u);
      }
    }
  }
};

// a wave's 16 rows as the B operand of the d-reducing products: lane (c, g)
// holds row c, columns 32 step + 8g .. + 7, as bf16; a row past S is zeros
template <int HD>
__device__ __forceinline__ void ab_load_rows(u32x4 (&reg)[HD / 32],
                                             AtSlice<const float> src, int row,
                                             int S, int g) {
  const float* p = src.p + (long)min(row, S - 1) * src.ld + 8 * g;
  #pragma unroll
  for (int s = 0; s < HD / 32; ++s) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p + 32 * s);
    const f32x4 b = *reinterpret_cast<const f32x4*>(p + 32 * s + 4);
    const u32x2 x = ab_pack4(row < S ? a : f32x4{});
    const u32x2 y = ab_pack4(row < S ? b : f32x4{});
    reg[s] = u32x4{x.x, x.y, y.x, y.y};
  }
}

// acc[j] += tile[16j + c][:] . reg  (row-major tile, b128 reads)
template <int HD>
__device__ __forceinline__ void ab_gemm_rows(f32x4 (&acc)[4],
                                             const __bf16* __restrict__ lds,
                                             const u32x4 (&reg)[HD / 32], int c,
                                             int g) {
  #pragma unroll
  for (int s = 0; s < HD / 32; ++s) {
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
      const u32x4 a = *reinterpret_cast<const u32x4*>(
          lds + (16 * j + c) * ab_ldr<HD>() + 32 * s + 8 * g);
      acc[j] = ab_mfma(a, reg[s], acc[j]);
    }
  }
}

// acc[db] += sum over the tile's 64 walked rows of
// tile[16j + 4g + r][16db + c] * w[j][r]  (transposed tile, b64 reads; w[j] is
// the lane's four entries of block j packed to bf16)
template <int HD>
__device__ __forceinline__ void ab_gemm_walked(f32x4 (&acc)[HD / 16],
                                               const __bf16* __restrict__ ldsT,
                                               const u32x2 (&w)[4], int c,
                                               int g) {
  #pragma unroll
  for (int h = 0; h < 2; ++h) {
    const u32x4 b = {w[2 * h].x, w[2 * h].y, w[2 * h + 1].x, w[2 * h + 1].y};
    #pragma unroll
    for (int db = 0; db < HD / 16; ++db) {
      const __bf16* at = ldsT + (16 * db + c) * AB_LDT + 32 * h + 4 * g;
      const u32x2 a0 = *reinterpret_cast<const u32x2*>(at);
      const u32x2 a1 = *reinterpret_cast<const u32x2*>(at + 16);
      acc[db] = ab_mfma(u32x4{a0.x, a0.y, a1.x, a1.y}, b, acc[db]);
    }
  }
}

template <int HD, bool DROPOUT, bool BIAS, bool HEADS, bool CAUSAL>
__global__ __launch_bounds__(256) void attn_tiled_bf16_fwd_kernel(AtArgs a) {
  __shared__ __align__(16) __bf16 ldsK[AT_TILE * ab_ldr<HD>()];   // [key][d]
  __shared__ __align__(16) __bf16 ldsVT[HD * AB_LDT];             // [d][key]
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

  u32x4 qreg[HD / 32];
  ab_load_rows<HD>(qreg, qs, row, S, g);

  f32x4 oacc[HD / 16] = {};
  float m = -INFINITY, l = 0.f;   // l: this lane's share of the row sum
  const long ridx = ((long)bh * S + row) * S;

  AbTile<HD> tk, tv;
  float nb = 0.f;
  const int ntiles = CAUSAL ? qt + 1 : (S + AT_TILE - 1) / AT_TILE;
  tk.load(ks, 0, S, tid);
  tv.load(vs, 0, S, tid);
  if (tid < AT_TILE) nb = at_key_bias<BIAS>(kbr, tid, S);

  for (int t = 0; t < ntiles; ++t) {
    __syncthreads();              // the previous tile's reads are done
    tk.store_rows(ldsK, tid);
    tv.store_cols(ldsVT, tid);
    if (tid < AT_TILE) ldsB[tid] = nb;
    __syncthreads();
    if (t + 1 < ntiles) {
      tk.load(ks, (t + 1) * AT_TILE, S, tid);
      tv.load(vs, (t + 1) * AT_TILE, S, tid);
      if (tid < AT_TILE) nb = at_key_bias<BIAS>(kbr, (t + 1) * AT_TILE + tid, S);
    }

    f32x4 sacc[4] = {};
    ab_gemm_rows<HD>(sacc, ldsK, qreg, c, g);

    float mx = -INFINITY;
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 kb = *reinterpret_cast<const f32x4*>(&ldsB[16 * j + 4 * g]);
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        sacc[j][r] = sacc[j][r] * a.scale + kb[r];
        if (CAUSAL && at_hidden(t == qt, 16 * wid + c, 16 * j + 4 * g + r))
          sacc[j][r] = -INFINITY;
        mx = fmaxf(mx, sacc[j][r]);
      }
    }
    const float m_new = fmaxf(m, at_group_max(mx));
    // a tile of -inf keys leaves the max at -inf: exponents then refer to 0,
    // so they are exp(-inf) = 0 and not exp(-inf + inf) = NaN
    const float m_ref = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = expf(m - m_ref);
    m = m_new;
    float ps = 0.f;
    u32x2 w[4];
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
      f32x4 e;
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        e[r] = expf(sacc[j][r] - m_ref);
        ps += e[r];               // the row sum takes the clean fp32 values
        if (DROPOUT) {
          const int key = t * AT_TILE + 16 * j + 4 * g + r;
          const bool keep =
              slk_uniform32(rng_stream, (uint32_t)(ridx + key)) >= a.p;
          e[r] = keep ? e[r] * a.inv_keep : 0.f;
        }
      }
      w[j] = ab_pack4(e);
    }
    l = l * alpha + ps;
    #pragma unroll
    for (int db = 0; db < HD / 16; ++db) oacc[db] *= alpha;
    ab_gemm_walked<HD>(oacc, ldsVT, w, c, g);
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
__global__ __launch_bounds__(256) void attn_tiled_bf16_bwd_dq_kernel(AtArgs a) {
  __shared__ __align__(16) __bf16 ldsK[AT_TILE * ab_ldr<HD>()];   // [key][d]
  __shared__ __align__(16) __bf16 ldsKT[HD * AB_LDT];             // [d][key]
  __shared__ __align__(16) __bf16 ldsV[AT_TILE * ab_ldr<HD>()];   // [key][d]
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

  u32x4 qreg[HD / 32], greg[HD / 32];
  ab_load_rows<HD>(qreg, qs, row, S, g);
  ab_load_rows<HD>(greg, gouts, row, S, g);
  // delta = sum_d gO_b * O in fp32 (= sum_c dP*P at upstream gO_b)
  float delta = 0.f;
  {
    const auto os = at_slice<HD, HEADS, const float>(a.out, a.so, bh, a.heads, S);
    const float* o = os.p + (long)min(row, S - 1) * os.ld + 8 * g;
    #pragma unroll
    for (int s = 0; s < HD / 32; ++s) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(o + 32 * s);
      const f32x4 y = *reinterpret_cast<const f32x4*>(o + 32 * s + 4);
      #pragma unroll
      for (int e = 0; e < 4; ++e) {
        delta += ab_elem(greg[s], e) * x[e];
        delta += ab_elem(greg[s], 4 + e) * y[e];
      }
    }
    delta = at_group_sum(delta);   // rows past S: greg is 0, delta is 0
  }
  // rows past S: any finite lse; their results are never stored
  const float lse = row < S ? a.lse[(long)bh * S + row] : 0.f;
  if (row < S && g == 0) a.delta[(long)bh * S + row] = delta;

  f32x4 dq[HD / 16] = {};
  const long ridx = ((long)bh * S + row) * S;

  AbTile<HD> tk, tv;
  float nb = 0.f;
  const int ntiles = CAUSAL ? qt + 1 : (S + AT_TILE - 1) / AT_TILE;
  tk.load(ks, 0, S, tid);
  tv.load(vs, 0, S, tid);
  if (tid < AT_TILE) nb = at_key_bias<BIAS>(kbr, tid, S);

  for (int t = 0; t < ntiles; ++t) {
    __syncthreads();
    tk.store_rows(ldsK, tid);
    tk.store_cols(ldsKT, tid);
    tv.store_rows(ldsV, tid);
    if (tid < AT_TILE) ldsB[tid] = nb;
    __syncthreads();
    if (t + 1 < ntiles) {
      tk.load(ks, (t + 1) * AT_TILE, S, tid);
      tv.load(vs, (t + 1) * AT_TILE, S, tid);
      if (tid < AT_TILE) nb = at_key_bias<BIAS>(kbr, (t + 1) * AT_TILE + tid, S);
    }

    f32x4 sacc[4] = {}, dp[4] = {};
    ab_gemm_rows<HD>(sacc, ldsK, qreg, c, g);
    ab_gemm_rows<HD>(dp, ldsV, greg, c, g);

    u32x2 w[4];
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 kb = *reinterpret_cast<const f32x4*>(&ldsB[16 * j + 4 * g]);
      f32x4 ds;
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
        ds[r] = pr * (d - delta);
      }
      w[j] = ab_pack4(ds);
    }
    ab_gemm_walked<HD>(dq, ldsKT, w, c, g);
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
__global__ __launch_bounds__(256) void attn_tiled_bf16_bwd_dkv_kernel(AtArgs a) {
  __shared__ __align__(16) __bf16 ldsQ[AT_TILE * ab_ldr<HD>()];   // [row][d]
  __shared__ __align__(16) __bf16 ldsQT[HD * AB_LDT];             // [d][row]
  __shared__ __align__(16) __bf16 ldsG[AT_TILE * ab_ldr<HD>()];
  __shared__ __align__(16) __bf16 ldsGT[HD * AB_LDT];
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

  u32x4 kreg[HD / 32], vreg[HD / 32];
  ab_load_rows<HD>(kreg, ks, key, S, g);
  ab_load_rows<HD>(vreg, vs, key, S, g);

  f32x4 dk[HD / 16] = {}, dv[HD / 16] = {};

  // the tile's lse (threads 0..63) and delta (threads 64..127) rows.  A row
  // past S gets lse = +inf, so its P is exp(-inf) = 0 and it adds nothing.
  auto load_row_stat = [&](int t) -> float {
    const int r = t * AT_TILE + (tid & 63);
    if (tid < AT_TILE) return r < S ? a.lse[(long)bh * S + r] : INFINITY;
    if (tid < 2 * AT_TILE) return r < S ? a.delta[(long)bh * S + r] : 0.f;
    return 0.f;
  };

  AbTile<HD> tq, tg;
  const int ntiles = (S + AT_TILE - 1) / AT_TILE;
  const int t0 = CAUSAL ? kt : 0;   // query tiles above the diagonal see no key here
  tq.load(qs, t0 * AT_TILE, S, tid);
  tg.load(gouts, t0 * AT_TILE, S, tid);
  float ns = load_row_stat(t0);

  for (int t = t0; t < ntiles; ++t) {
    __syncthreads();
    tq.store_rows(ldsQ, tid);
    tq.store_cols(ldsQT, tid);
    tg.store_rows(ldsG, tid);
    tg.store_cols(ldsGT, tid);
    if (tid < AT_TILE) ldsL[tid] = ns;
    else if (tid < 2 * AT_TILE) ldsD[tid - AT_TILE] = ns;
    __syncthreads();
    if (t + 1 < ntiles) {
      tq.load(qs, (t + 1) * AT_TILE, S, tid);
      tg.load(gouts, (t + 1) * AT_TILE, S, tid);
      ns = load_row_stat(t + 1);
    }

    f32x4 sacc[4] = {}, dp[4] = {};
    ab_gemm_rows<HD>(sacc, ldsQ, kreg, c, g);
    ab_gemm_rows<HD>(dp, ldsG, vreg, c, g);

    u32x2 pd[4], ds[4];
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f32x4 L = *reinterpret_cast<const f32x4*>(&ldsL[16 * i + 4 * g]);
      const f32x4 D = *reinterpret_cast<const f32x4*>(&ldsD[16 * i + 4 * g]);
      f32x4 pk4, ds4;
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
        pk4[r] = pk;
        ds4[r] = pr * (d - D[r]);
      }
      pd[i] = ab_pack4(pk4);
      ds[i] = ab_pack4(ds4);
    }
    ab_gemm_walked<HD>(dv, ldsGT, pd, c, g);
    ab_gemm_walked<HD>(dk, ldsQT, ds, c, g);
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

}  // namespace

// ---------------------------------------------------------------------------
// host: one launch each.  The argument checks, the outputs and the grid are
// the fp32 route's (attention_tiled.hip: attn_tiled_fwd / attn_tiled_bwd /
// attn_heads_fwd / attn_heads_bwd call these when their bf16 flag is set), so
// dtype, device, shapes, hd, the bias shape against heads and the
// head-strided alignment and stride rules cannot differ between the two.
// ---------------------------------------------------------------------------

void at_bf16_fwd(bool heads_layout, const AtProblem& pr, dim3 grid,
                 hipStream_t stream, const AtArgs& a) {
  if (heads_layout)
    SLK_AT_DISPATCH(attn_tiled_bf16_fwd_kernel, true, pr, grid, stream, a);
  else
    SLK_AT_DISPATCH(attn_tiled_bf16_fwd_kernel, false, pr, grid, stream, a);
}

void at_bf16_bwd_dq(bool heads_layout, const AtProblem& pr, dim3 grid,
                    hipStream_t stream, const AtArgs& a) {
  if (heads_layout)
    SLK_AT_DISPATCH(attn_tiled_bf16_bwd_dq_kernel, true, pr, grid, stream, a);
  else
    SLK_AT_DISPATCH(attn_tiled_bf16_bwd_dq_kernel, false, pr, grid, stream, a);
}

void at_bf16_bwd_dkv(bool heads_layout, const AtProblem& pr, dim3 grid,
                     hipStream_t stream, const AtArgs& a) {
  if (heads_layout)
    SLK_AT_DISPATCH(attn_tiled_bf16_bwd_dkv_kernel, true, pr, grid, stream, a);
  else
    SLK_AT_DISPATCH(attn_tiled_bf16_bwd_dkv_kernel, false, pr, grid, stream, a);
}

}  // namespace slk
