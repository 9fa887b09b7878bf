// Fused LoRA adapter kernels for gfx950: everything around the base GEMM of
//   out = x W^T + b + scaling * (dropout(x) A^T) B^T
// x [M,K], A [r,K], B [N,r], 1 <= r <= 16 (padded to 16 with zeros inside the
// kernels), K % 4 == 0, N % 4 == 0.  No xd, no mask and no delta array exists:
// the keep decision of element (row, col) of x is redrawn wherever it is
// needed as slk_uniform(seed, offset, row*K + col) >= p, the draw of
// dropout_fwd_dev_kernel on the contiguous x, from the offset the forward read
// on the device (returned as a one-element tensor, so a hipGraph replay's
// backward redraws its own forward's mask).
//
// Math is v_mfma_f32_16x16x4_f32 (exact fp32 products): lane l supplies
// A[i = l&15][k = l>>4] and B[k = l>>4][j = l&15] and receives
// D[i = 4*(l>>4) + q][j = l&15], q = 0..3.  Write c = l&15, g = l>>4.
//
// Row kernel (one template: forward, and backward by rows).  256 threads = 4
// waves own 16 rows of the big activation In [M,C]:
//   down  T[16][16] = In[16][C] Wd[C][r].  The waves interleave over the
//         contraction axis in pieces of 16 columns (a step of the block eats
//         64 consecutive floats of each row: two whole cache lines); lane
//         (c, g) reads the 16 bytes In[row c][col + 4g .. + 3] and feeds them
//         as four k-steps in which column col + 4g + e is LABELLED k = g: a
//         sum does not care in which order its terms are labelled.  The small
//         operand is read at the matching rows straight from L2 (forward:
//         the same 16 bytes of A's row c; backward: four floats of B's column
//         c), four steps of loads in flight before the first MFMA.  Chosen
//         over an LDS stage: A is 24 KB at K = 768 but 96 KB at K = 3072, a
//         block reads each element of it exactly once, and the 256 blocks of
//         M = 4096 all read the same bytes, so they stay in L2.
//         The four partial tiles are summed through LDS in wave order; the
//         first r columns of T go to global memory ([M,r]) for the
//         weight-gradient kernel.
//   up    Out[16][D] = Base + coef * T Wu[r][D], in place on the base GEMM's
//         fresh output.  Computed transposed, Out^T = Wu^T T^T, so that lane
//         (c, g) receives Out[row c][d0 + 4g .. + 3]: one 16-byte read and
//         write of Base/Out per lane and 16-column tile, the waves
//         interleaving over the tiles.  T^T is the B operand, read once from
//         LDS (four floats a lane); Wu^T comes from L2.  MFMA rather than
//         VALU: a 16x16 tile costs ceil(r/4) MFMAs (2 at r = 8, 64 cycles)
//         against r = 8 v_fma per lane and tile plus the broadcasts (128+),
//         and the k-steps past r are skipped.
//   forward:  In = x with keep/(1-p) applied as elements are loaded,
//             Wd[c][j] = A[j][c], T = xa, Wu[j][n] = B[n][j], coef = scaling.
//   backward: In = g, Wd[c][j] = B[c][j], T = gxa = scaling * g B, Wu = A,
//             Base = g W; the update is multiplied by the redrawn keep/(1-p)
//             before it is added.  Skipped (no Base) when x needs no gradient.
//
// Weight-gradient kernel: both gradients are Out[j][c] = sum_m Small[m][j]
// Big[m][c], gA from (gxa, dropout(x)) and gB from (xa, g) (times scaling).
// One grid covers both: blockIdx.x walks the 64-column chunks of K and then
// of N, blockIdx.y the slabs of M (lora_wgrad_slabs: ~2 blocks per CU at
// M = 4096, one slab at small M).  A block's four waves interleave over the
// slab's rows four at a time; lane (c, g) reads the 16 bytes
// Big[m + g][col0 + 4c .. + 3] (a wave reads 256 contiguous bytes of each of
// four rows) and feeds element e to accumulator e, whose column j = c is
// LABELLED col0 + 4c + e; Small^T is the A operand.  The waves' partials are
// summed through LDS in wave order and go to a slab buffer; slab_reduce_pair
// (one launch) sums the slabs of both outputs in slab order into gA [r,K] and
// gB [N,r].  No atomics, no zero-fill, every output written once.
//
// Compiler resource report (hipcc --offload-arch=gfx950 -O3
// -Rpass-analysis=kernel-resource-usage); scratch is 0 in all six:
//   kernel                          VGPR  AGPR  LDS bytes  scratch  waves/SIMD
//   lora_row_kernel<fwd, drop>        76     4       5440        0      6
//   lora_row_kernel<fwd, nodrop>      76     4       5440        0      6
//   lora_row_kernel<bwd, drop>        88     4       5440        0      5
//   lora_row_kernel<bwd, nodrop>      74     4       5440        0      6
//   lora_wgrad_kernel<drop>           76    20      16384        0      5
//   lora_wgrad_kernel<nodrop>         54    16      16384        0      7
// A block is one wave per SIMD, so the row kernel's 256 blocks at M = 4096 sit
// far below these limits: what it has in flight is its own batched loads.
//
// QKV-grouped kernels (lora_qkv_*): the query, key and value adapters of one
// self-attention block share x, M, K, N, r, scaling and p and differ in their
// small operands and their dropout offset (o, o+1, o+2: what three successive
// single calls read).  Same lane maps, same interleaves, same summation orders
// as above, so every output element of the forward has the bits three single
// calls give it; what changes is what is read and written how often:
//   row, forward   a lane's 16 bytes of x are loaded once per step, masked
//                  three times and fed to three accumulators against A_q,
//                  A_k, A_v; xa is [3][M][r].  The up phase reads the three
//                  dense base products and writes Out_j = Base_j + scaling *
//                  T_j B_j^T into the column thirds of ONE packed [M,3N]
//                  tensor, the layout the head-strided attention kernels
//                  read.  (Base and Out are separate pointers with their own
//                  row strides: the base GEMMs of both routes keep their
//                  dense stores, and the traffic is the in-place form's: one
//                  read, one write per element.)  The thirds are walked one
//                  after the other, the waves interleaving over each third's
//                  tiles: T_j^T is then four registers, not twelve selected
//                  at run time.
//   row, backward  reads the thirds of the packed gradient in place (row
//                  stride given), gxa is [3][M][r]; the up phase adds all
//                  three masked updates to Base = sum_j g_j W_j in one read
//                  and one write of gx.
//   weight grad    a gA block streams its slab of x once into gA_q, gA_k,
//                  gA_v (three masks on the one load, twelve accumulators);
//                  the gB blocks walk the 3 * ceil(N/64) chunks of the packed
//                  gradient.  Slabs are [slabs][3][r][K] and [slabs][3][N][r],
//                  so slab_reduce_pair sums all six outputs in one launch.
//   kernel                          VGPR  AGPR  LDS bytes  scratch  waves/SIMD
//   lora_qkv_row_kernel<fwd, drop>   114    12      16320        0      4
//   lora_qkv_row_kernel<fwd, nodrop>  98    12      16320        0      4
//   lora_qkv_row_kernel<bwd, drop>   161    12      16320        0      2
//   lora_qkv_row_kernel<bwd, nodrop> 148    12      16320        0      3
//   lora_qkv_wgrad_kernel<drop>       98    60      16384        0      3
//   lora_qkv_wgrad_kernel<nodrop>     72    48      16384        0      4
// Scratch is 0 at the single kernels' batch depths (4 row steps, 8 row
// groups), so they are kept; a block is still one wave per SIMD.
#include <type_traits>

#include "torch_util.h"

namespace slk {

constexpr int LR_ROWS = 16;      // rows of the activation per row-kernel block
constexpr int LR_RMAX = 16;      // r is padded to one MFMA tile
constexpr int LW_COLS = 64;      // columns per weight-gradient block
constexpr int LW_TARGET = 512;   // weight-gradient blocks wanted: 2 per CU

__device__ __forceinline__ f32x4 lr_mfma(float a, float b, f32x4 acc) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
}

// x[row][col .. col+3] after dropout: keep/(1-p) on the elements of x
template <bool DROPOUT>
__device__ __forceinline__ f32x4 lr_drop(f32x4 v, uint64_t seed, uint64_t offset,
                                         uint64_t idx, float p, float inv_keep) {
  if (DROPOUT) {
    #pragma unroll
    for (int e = 0; e < 4; ++e)
      v[e] = slk_uniform(seed, offset, idx + e) >= p ? v[e] * inv_keep : 0.f;
  }
  return v;
}

struct LoraRowArgs {
  const float* in;         // [M,C]: x (forward) or g (backward)
  const float* wd;         // forward A [r,C]; backward B [C,r]
  const float* wu;         // forward B [D,r]; backward A [r,D]
  float* t;                // [M,r]: xa or gxa, written
  float* out;              // [M,D]: Base in, Out out; null skips the up phase
  const long* offset_in;   // dropout counter (forward: live; backward: saved)
  long* offset_out;        // forward: the offset it read
  uint64_t seed;
  int M, C, D, r;
  float tscale, ucoef, p, inv_keep;
};

struct LrDown { f32x4 v, w; };
struct LrUp { f32x4 base; float wa[4]; };

template <bool BWD, bool DROPOUT>
__global__ __launch_bounds__(256) void lora_row_kernel(LoraRowArgs a) {
  __shared__ float part[4][LR_ROWS][LR_RMAX + 1];
  __shared__ float Ts[LR_ROWS][LR_RMAX + 1];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int M = a.M, C = a.C, D = a.D, r = a.r;
  const int row0 = blockIdx.x * LR_ROWS;
  const int row = row0 + c;
  const bool row_ok = row < M;
  const long rowc = row_ok ? row : M - 1;

  uint64_t offset = 0;
  if (DROPOUT) {
    offset = (uint64_t)a.offset_in[0];
    if (!BWD && blockIdx.x == 0 && tid == 0) a.offset_out[0] = (long)offset;
  }

  // ---- down: T = In Wd, the waves interleaved over C ----
  f32x4 acc = {};
  {
    const float* inrow = a.in + rowc * C;
    const int jc = min(c, r - 1);
    const bool j_ok = c < r;
    slk_batched<4, LrDown>(
        0, (C + 63) / 64, 1,
        [&](int s) {
          const int col = 64 * s + 16 * wid + 4 * g;
          const bool ok = col < C;
          const int cc = ok ? col : 0;
          LrDown l;
          l.v = *reinterpret_cast<const f32x4*>(inrow + cc);
          if (!BWD) {
            l.w = *reinterpret_cast<const f32x4*>(a.wd + (long)jc * C + cc);
          } else {
            #pragma unroll
            for (int e = 0; e < 4; ++e) l.w[e] = a.wd[(long)(cc + e) * r + jc];
          }
          if (!(ok && row_ok)) l.v = f32x4{};
          if (!(ok && j_ok)) l.w = f32x4{};
          return l;
        },
        [&](int s, const LrDown& l) {
          const int col = 64 * s + 16 * wid + 4 * g;
          const f32x4 v = lr_drop<DROPOUT && !BWD>(
              l.v, a.seed, offset, (uint64_t)rowc * C + col, a.p, a.inv_keep);
          #pragma unroll
          for (int e = 0; e < 4; ++e) acc = lr_mfma(v[e], l.w[e], acc);
        });
  }
  #pragma unroll
  for (int q = 0; q < 4; ++q) part[wid][4 * g + q][c] = acc[q];
  __syncthreads();
  {
    const int i = tid >> 4, j = tid & 15;
    const float t =
        (((part[0][i][j] + part[1][i][j]) + part[2][i][j]) + part[3][i][j]) *
        a.tscale;
    Ts[i][j] = t;
    if (row0 + i < M && j < r) a.t[(long)(row0 + i) * r + j] = t;
  }
  if (a.out == nullptr) return;
  __syncthreads();

  // ---- up: Out^T = Base^T + coef * Wu^T T^T, the waves interleaved over D ----
  float tb[4];
  #pragma unroll
  for (int ks = 0; ks < 4; ++ks) tb[ks] = Ts[c][4 * ks + g];
  float* outrow = a.out + rowc * D;
  slk_batched<4, LrUp>(
      wid, (D + 15) / 16, 4,
      [&](int tile) {
        const int dcol = 16 * tile + c;
        const bool d_ok = dcol < D;
        const int dc = d_ok ? dcol : 0;
        LrUp l;
        #pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const int k = 4 * ks + g;
          const int kc = min(k, r - 1);
          const float w = BWD ? a.wu[(long)kc * D + dc] : a.wu[(long)dc * r + kc];
          l.wa[ks] = d_ok && k < r ? w : 0.f;
        }
        l.base = *reinterpret_cast<const f32x4*>(
            outrow + min(16 * tile + 4 * g, D - 4));
        return l;
      },
      [&](int tile, const LrUp& l) {
        f32x4 u = {};
        #pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          if (4 * ks < r) u = lr_mfma(l.wa[ks], tb[ks], u);
        const int col = 16 * tile + 4 * g;
        u = u * a.ucoef;
        u = lr_drop<DROPOUT && BWD>(u, a.seed, offset, (uint64_t)rowc * D + col,
                                    a.p, a.inv_keep);
        if (row_ok && col < D)
          *reinterpret_cast<f32x4*>(outrow + col) = l.base + u;
      });
}

struct LoraWgradArgs {
  const float* x;          // [M,K]
  const float* g;          // [M,N]
  const float* xa;         // [M,r]
  const float* gxa;        // [M,r]
  float* slab_a;           // [slabs][r][K]
  float* slab_b;           // [slabs][N][r]
  const long* offset;      // the offset the forward saved
  uint64_t seed;
  int M, K, N, r, rows_per_slab;
  float scaling, p, inv_keep;
};

struct LwStep { f32x4 big; float small; };

template <bool DROPOUT>
__global__ __launch_bounds__(256) void lora_wgrad_kernel(LoraWgradArgs a) {
  __shared__ float red[4][4][4][64];   // [wave][e][q][lane]

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int r = a.r;
  const int chunks_k = (a.K + LW_COLS - 1) / LW_COLS;
  const bool job_a = (int)blockIdx.x < chunks_k;          // block-uniform
  const int C = job_a ? a.K : a.N;
  const int col0 = LW_COLS * (job_a ? blockIdx.x : blockIdx.x - chunks_k);
  const float* __restrict__ big = job_a ? a.x : a.g;
  const float* __restrict__ small = job_a ? a.gxa : a.xa;
  const int m_lo = blockIdx.y * a.rows_per_slab;
  const int m_hi = min(a.M, m_lo + a.rows_per_slab);

  uint64_t offset = 0;
  if (DROPOUT) offset = (uint64_t)a.offset[0];

  const int col = col0 + 4 * c;
  const bool col_ok = col < C;
  const int cc = col_ok ? col : 0;
  const int jc = min(c, r - 1);
  const bool j_ok = c < r;

  f32x4 acc[4] = {};
  slk_batched<8, LwStep>(
      m_lo + 4 * wid, m_hi, 16,
      [&](int m4) {
        const int m = m4 + g;
        const bool m_ok = m < m_hi;
        const long mc = m_ok ? m : m_hi - 1;
        LwStep l;
        l.big = *reinterpret_cast<const f32x4*>(big + mc * C + cc);
        l.small = small[mc * r + jc];
        if (!(m_ok && col_ok)) l.big = f32x4{};
        if (!(m_ok && j_ok)) l.small = 0.f;
        return l;
      },
      [&](int m4, const LwStep& l) {
        f32x4 v = l.big;
        if (DROPOUT && job_a) {
          const long mc = min(m4 + g, m_hi - 1);
          v = lr_drop<DROPOUT>(v, a.seed, offset, (uint64_t)mc * C + cc, a.p,
                               a.inv_keep);
        }
        #pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = lr_mfma(l.small, v[e], acc[e]);
      });

  #pragma unroll
  for (int e = 0; e < 4; ++e) {
    #pragma unroll
    for (int q = 0; q < 4; ++q) red[wid][e][q][lane] = acc[e][q];
  }
  __syncthreads();
  // thread (q = wid, lane): Out[j = 4g + q][col .. col + 3], waves in order
  const int j = 4 * g + wid;
  f32x4 s;
  #pragma unroll
  for (int e = 0; e < 4; ++e)
    s[e] = ((red[0][e][wid][lane] + red[1][e][wid][lane]) +
            red[2][e][wid][lane]) + red[3][e][wid][lane];
  if (!(j < r && col_ok)) return;
  if (job_a) {
    *reinterpret_cast<f32x4*>(a.slab_a + ((long)blockIdx.y * r + j) * a.K + col) = s;
  } else {
    float* o = a.slab_b + ((long)blockIdx.y * a.N + col) * r + j;
    #pragma unroll
    for (int e = 0; e < 4; ++e) o[(long)e * r] = s[e] * a.scaling;
  }
}

// ---------------------------------------------------------------------------
// QKV-grouped adapters: j = 0, 1, 2 is query, key, value
// ---------------------------------------------------------------------------

constexpr int LQ = 3;

struct LoraQkvRowArgs {
  const float* in;         // forward x [M,C]; backward the packed gradient,
  long ld_in;              //   third j at in + j*C; ld_in: its row stride
  const float* wd[LQ];     // forward A_j [r,C]; backward B_j [C,r]
  const float* wu[LQ];     // forward B_j [D,r]; backward A_j [r,D]
  float* t;                // [3][M][r]: xa or gxa, written
  const float* base[LQ];   // forward: x W_j^T + b_j [M,D]; backward: base[0]
  long ld_base;            //   = sum_j g_j W_j [M,D]; ld_base: row stride
  float* out;              // forward: packed [M,3D], third j at out + j*D;
  long ld_out;             //   backward: gx [M,D]; null skips the up phase
  const long* offset_in;   // forward: the live counter, already advanced by 3;
  long* offset_out;        //   backward: what the forward wrote here, the
  uint64_t seed;           //   offset of q's mask (k: + 1, v: + 2)
  int M, C, D, r;
  float tscale, ucoef, p, inv_keep;
};

template <bool BWD> struct LqDown { f32x4 v[BWD ? LQ : 1], w[LQ]; };
struct LqUp { f32x4 base; float wa[LQ][4]; };

template <bool BWD, bool DROPOUT>
__global__ __launch_bounds__(256) void lora_qkv_row_kernel(LoraQkvRowArgs a) {
  __shared__ float part[LQ][4][LR_ROWS][LR_RMAX + 1];
  __shared__ float Ts[LQ][LR_ROWS][LR_RMAX + 1];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int M = a.M, C = a.C, D = a.D, r = a.r;
  const int row0 = blockIdx.x * LR_ROWS;
  const int row = row0 + c;
  const bool row_ok = row < M;
  const long rowc = row_ok ? row : M - 1;

  uint64_t offset = 0;
  if (DROPOUT) {
    offset = (uint64_t)a.offset_in[0];
    if (!BWD) {
      offset -= LQ - 1;
      if (blockIdx.x == 0 && tid == 0) a.offset_out[0] = (long)offset;
    }
  }

  // ---- down: T_j = In_j Wd_j (forward: one In), the waves interleaved over C
  f32x4 acc[LQ] = {};
  {
    const float* inrow = a.in + rowc * a.ld_in;
    const int jc = min(c, r - 1);
    const bool j_ok = c < r;
    slk_batched<4, LqDown<BWD>>(
        0, (C + 63) / 64, 1,
        [&](int s) {
          const int col = 64 * s + 16 * wid + 4 * g;
          const bool ok = col < C;
          const int cc = ok ? col : 0;
          LqDown<BWD> l;
          #pragma unroll
          for (int j = 0; j < (BWD ? LQ : 1); ++j) {
            l.v[j] = *reinterpret_cast<const f32x4*>(inrow + (long)j * C + cc);
            if (!(ok && row_ok)) l.v[j] = f32x4{};
          }
          #pragma unroll
          for (int j = 0; j < LQ; ++j) {
            if (!BWD) {
              l.w[j] = *reinterpret_cast<const f32x4*>(a.wd[j] + (long)jc * C + cc);
            } else {
              #pragma unroll
              for (int e = 0; e < 4; ++e)
                l.w[j][e] = a.wd[j][(long)(cc + e) * r + jc];
            }
            if (!(ok && j_ok)) l.w[j] = f32x4{};
          }
          return l;
        },
        [&](int s, const LqDown<BWD>& l) {
          const int col = 64 * s + 16 * wid + 4 * g;
          #pragma unroll
          for (int j = 0; j < LQ; ++j) {
            const f32x4 v = lr_drop<DROPOUT && !BWD>(
                l.v[BWD ? j : 0], a.seed, offset + j, (uint64_t)rowc * C + col,
                a.p, a.inv_keep);
            #pragma unroll
            for (int e = 0; e < 4; ++e) acc[j] = lr_mfma(v[e], l.w[j][e], acc[j]);
          }
        });
  }
  #pragma unroll
  for (int j = 0; j < LQ; ++j) {
    #pragma unroll
    for (int q = 0; q < 4; ++q) part[j][wid][4 * g + q][c] = acc[j][q];
  }
  __syncthreads();
  {
    const int i = tid >> 4, k = tid & 15;
    #pragma unroll
    for (int j = 0; j < LQ; ++j) {
      const float t = (((part[j][0][i][k] + part[j][1][i][k]) + part[j][2][i][k]) +
                       part[j][3][i][k]) * a.tscale;
      Ts[j][i][k] = t;
      if (row0 + i < M && k < r) a.t[((long)j * M + row0 + i) * r + k] = t;
    }
  }
  if (a.out == nullptr) return;
  __syncthreads();

  const int tiles = (D + 15) / 16;
  if constexpr (!BWD) {
    // ---- up: Out_j^T = Base_j^T + coef * Wu_j^T T_j^T, third after third ----
    #pragma unroll
    for (int j = 0; j < LQ; ++j) {
      float tb[4];
      #pragma unroll
      for (int ks = 0; ks < 4; ++ks) tb[ks] = Ts[j][c][4 * ks + g];
      const float* baserow = a.base[j] + rowc * a.ld_base;
      float* outrow = a.out + rowc * a.ld_out + (long)j * D;
      const float* wu = a.wu[j];
      slk_batched<4, LrUp>(
          wid, tiles, 4,
          [&](int tile) {
            const int dcol = 16 * tile + c;
            const bool d_ok = dcol < D;
            const int dc = d_ok ? dcol : 0;
            LrUp l;
            #pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
              const int k = 4 * ks + g;
              const float w = wu[(long)dc * r + min(k, r - 1)];
              l.wa[ks] = d_ok && k < r ? w : 0.f;
            }
            l.base = *reinterpret_cast<const f32x4*>(
                baserow + min(16 * tile + 4 * g, D - 4));
            return l;
          },
          [&](int tile, const LrUp& l) {
            f32x4 u = {};
            #pragma unroll
            for (int ks = 0; ks < 4; ++ks)
              if (4 * ks < r) u = lr_mfma(l.wa[ks], tb[ks], u);
            const int col = 16 * tile + 4 * g;
            u = u * a.ucoef;
            if (row_ok && col < D)
              *reinterpret_cast<f32x4*>(outrow + col) = l.base + u;
          });
    }
  } else {
    // ---- up: gx^T = Base^T + sum_j keep_j/(1-p) o (A_j^T gxa_j^T) ----
    float tb[LQ][4];
    #pragma unroll
    for (int j = 0; j < LQ; ++j) {
      #pragma unroll
      for (int ks = 0; ks < 4; ++ks) tb[j][ks] = Ts[j][c][4 * ks + g];
    }
    const float* baserow = a.base[0] + rowc * a.ld_base;
    float* outrow = a.out + rowc * a.ld_out;
    slk_batched<4, LqUp>(
        wid, tiles, 4,
        [&](int tile) {
          const int dcol = 16 * tile + c;
          const bool d_ok = dcol < D;
          const int dc = d_ok ? dcol : 0;
          LqUp l;
          #pragma unroll
          for (int j = 0; j < LQ; ++j) {
            #pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
              const int k = 4 * ks + g;
              const float w = a.wu[j][(long)min(k, r - 1) * D + dc];
              l.wa[j][ks] = d_ok && k < r ? w : 0.f;
            }
          }
          l.base = *reinterpret_cast<const f32x4*>(
              baserow + min(16 * tile + 4 * g, D - 4));
          return l;
        },
        [&](int tile, const LqUp& l) {
          const int col = 16 * tile + 4 * g;
          f32x4 s = l.base;
          #pragma unroll
          for (int j = 0; j < LQ; ++j) {
            f32x4 u = {};
            #pragma unroll
            for (int ks = 0; ks < 4; ++ks)
              if (4 * ks < r) u = lr_mfma(l.wa[j][ks], tb[j][ks], u);
            u = u * a.ucoef;
            s += lr_drop<DROPOUT>(u, a.seed, offset + j, (uint64_t)rowc * D + col,
                                  a.p, a.inv_keep);
          }
          if (row_ok && col < D) *reinterpret_cast<f32x4*>(outrow + col) = s;
        });
  }
}

struct LoraQkvWgradArgs {
  const float* x;          // [M,K]
  const float* g;          // packed gradient, third j at g + j*N
  long ld_g;               // its row stride
  const float* xa;         // [3][M][r]
  const float* gxa;        // [3][M][r]
  float* slab_a;           // [slabs][3][r][K]
  float* slab_b;           // [slabs][3][N][r]
  const long* offset;      // the offset the forward saved (q's)
  uint64_t seed;
  int M, K, N, r, rows_per_slab;
  float scaling, p, inv_keep;
};

template <int NJ> struct LqwStep { f32x4 big; float small[NJ]; };

// acc[j][e] += Small_j^T Big over rows m_lo .. m_hi of one 64-column chunk:
// lora_wgrad_kernel's loop with NJ small operands (small + j * small_step)
// against the one load of Big; MASKED redraws mask j at offset + j
template <int NJ, bool MASKED>
__device__ __forceinline__ void lqw_accumulate(
    const float* __restrict__ big, long ld, int C, int cc, bool col_ok,
    const float* __restrict__ small, long small_step, int r, int m_lo, int m_hi,
    uint64_t seed, uint64_t offset, float p, float inv_keep,
    f32x4 (&acc)[NJ][4]) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int jc = min(c, r - 1);
  const bool j_ok = c < r;
  slk_batched<8, LqwStep<NJ>>(
      m_lo + 4 * wid, m_hi, 16,
      [&](int m4) {
        const int m = m4 + g;
        const bool m_ok = m < m_hi;
        const long mc = m_ok ? m : m_hi - 1;
        LqwStep<NJ> l;
        l.big = *reinterpret_cast<const f32x4*>(big + mc * ld + cc);
        if (!(m_ok && col_ok)) l.big = f32x4{};
        #pragma unroll
        for (int j = 0; j < NJ; ++j) {
          l.small[j] = small[j * small_step + mc * r + jc];
          if (!(m_ok && j_ok)) l.small[j] = 0.f;
        }
        return l;
      },
      [&](int m4, const LqwStep<NJ>& l) {
        const long mc = min(m4 + g, m_hi - 1);
        #pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const f32x4 v = lr_drop<MASKED>(l.big, seed, offset + j,
                                          (uint64_t)mc * C + cc, p, inv_keep);
          #pragma unroll
          for (int e = 0; e < 4; ++e)
            acc[j][e] = lr_mfma(l.small[j], v[e], acc[j][e]);
        }
      });
}

// the four waves' partials of one output tile, summed in wave order: thread
// (q = wid, lane) receives Out[4g + q][col .. col + 3].  Block-wide; red is
// free again on return
__device__ __forceinline__ f32x4 lqw_wave_sum(float (&red)[4][4][4][64],
                                              const f32x4 (&acc)[4]) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  #pragma unroll
  for (int e = 0; e < 4; ++e) {
    #pragma unroll
    for (int q = 0; q < 4; ++q) red[wid][e][q][lane] = acc[e][q];
  }
  __syncthreads();
  f32x4 s;
  #pragma unroll
  for (int e = 0; e < 4; ++e)
    s[e] = ((red[0][e][wid][lane] + red[1][e][wid][lane]) +
            red[2][e][wid][lane]) + red[3][e][wid][lane];
  __syncthreads();
  return s;
}

template <bool DROPOUT>
__global__ __launch_bounds__(256) void lora_qkv_wgrad_kernel(LoraQkvWgradArgs a) {
  __shared__ float red[4][4][4][64];   // [wave][e][q][lane]

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int r = a.r;
  const int chunks_k = (a.K + LW_COLS - 1) / LW_COLS;
  const int chunks_n = (a.N + LW_COLS - 1) / LW_COLS;
  const bool job_a = (int)blockIdx.x < chunks_k;          // block-uniform
  const int m_lo = blockIdx.y * a.rows_per_slab;
  const int m_hi = min(a.M, m_lo + a.rows_per_slab);
  const long mr = (long)a.M * r;
  const int jr = 4 * g + wid;           // the output row lqw_wave_sum hands over

  if (job_a) {
    const int col = LW_COLS * blockIdx.x + 4 * c;
    const bool col_ok = col < a.K;
    uint64_t offset = 0;
    if (DROPOUT) offset = (uint64_t)a.offset[0];
    f32x4 acc[LQ][4] = {};
    lqw_accumulate<LQ, DROPOUT>(a.x, a.K, a.K, col_ok ? col : 0, col_ok, a.gxa,
                                mr, r, m_lo, m_hi, a.seed, offset, a.p,
                                a.inv_keep, acc);
    #pragma unroll
    for (int j = 0; j < LQ; ++j) {
      const f32x4 s = lqw_wave_sum(red, acc[j]);
      if (jr < r && col_ok)
        *reinterpret_cast<f32x4*>(
            a.slab_a + (((long)blockIdx.y * LQ + j) * r + jr) * a.K + col) = s;
    }
  } else {
    const int chunk = blockIdx.x - chunks_k;
    const int j = chunk / chunks_n;
    const int col = LW_COLS * (chunk - j * chunks_n) + 4 * c;
    const bool col_ok = col < a.N;
    f32x4 acc[1][4] = {};
    lqw_accumulate<1, false>(a.g + (long)j * a.N, a.ld_g, a.N, col_ok ? col : 0,
                             col_ok, a.xa + j * mr, 0, r, m_lo, m_hi, 0, 0, 0.f,
                             1.f, acc);
    const f32x4 s = lqw_wave_sum(red, acc[0]);
    if (jr < r && col_ok) {
      float* o = a.slab_b + (((long)blockIdx.y * LQ + j) * a.N + col) * r + jr;
      #pragma unroll
      for (int e = 0; e < 4; ++e) o[(long)e * r] = s[e] * a.scaling;
    }
  }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------

// slabs of M for the weight-gradient grid: enough blocks to fill the chip, at
// least 64 rows (four k-steps a wave) per slab, a multiple of 16 rows each.
// The QKV grid takes the same count although it has 3 * ceil(N/64) gB
// chunks: its time is its gA blocks', which draw three masks an element, and
// with the slabs cut to 512 / all chunks (10 at K = N = 768) only 120 of them
// shared that work: 58.1 us measured against 3 * 14.0 us for three single
// launches at M = 4096.  Sized by one adapter's chunks there are 252.
static int lw_rows_per_slab(long M, long K, long N) {
  const long chunks = ceil_div(K, LW_COLS) + ceil_div(N, LW_COLS);
  long slabs = std::max<long>(1, LW_TARGET / chunks);
  slabs = std::min<long>(slabs, std::max<long>(1, (M + 63) / 64));
  const long rows = (M + slabs - 1) / slabs;
  return (int)std::max<long>(16, (rows + 15) / 16 * 16);
}

int lora_wgrad_slabs(int64_t M, int64_t K, int64_t N) {
  TORCH_CHECK(M >= 1 && K >= 1 && N >= 1, "lora_wgrad_slabs: M, K, N >= 1");
  return ceil_div(M, lw_rows_per_slab(M, K, N));
}

// a float32 cuda tensor of exactly this shape, contiguous and 16-byte aligned
// (the kernels move float4s and index rows themselves)
static void lr_operand(const at::Tensor& t, const at::Tensor& like,
                       at::IntArrayRef shape, const char* who, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat, who, ": ", name,
              " must be a float32 cuda tensor");
  TORCH_CHECK(t.device() == like.device(), who, ": ", name,
              " must be on x's device");
  TORCH_CHECK(t.sizes() == shape, who, ": ", name, " must have shape ", shape,
              " (got ", t.sizes(), ")");
  TORCH_CHECK(t.is_contiguous(), who, ": ", name, " must be contiguous");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0, who, ": ",
              name, " must be 16-byte aligned");
}

struct LoraProblem {
  long M, K, N, r;
  bool drop;
};

static LoraProblem lora_check(const at::Tensor& x, const at::Tensor& A,
                              const at::Tensor& B, double p,
                              const c10::optional<at::Tensor>& offset,
                              const char* who) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.dim() == 2, who,
              ": x must be a float32 cuda tensor [M,K]");
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2, who, ": lora_A [r,K], lora_B [N,r]");
  LoraProblem pr;
  pr.M = x.size(0);
  pr.K = x.size(1);
  pr.r = A.size(0);
  pr.N = B.size(0);
  TORCH_CHECK(pr.r >= 1 && pr.r <= LR_RMAX, who, ": r=", pr.r,
              " outside 1..", LR_RMAX);
  TORCH_CHECK(pr.K >= 4 && pr.K % 4 == 0 && pr.N >= 4 && pr.N % 4 == 0, who,
              ": K=", pr.K, " and N=", pr.N, " must be multiples of 4");
  TORCH_CHECK(pr.M < (1l << 31) - LR_ROWS && pr.K < (1 << 24) && pr.N < (1 << 24),
              who, ": M, K or N out of range");
  lr_operand(x, x, {pr.M, pr.K}, who, "x");
  lr_operand(A, x, {pr.r, pr.K}, who, "lora_A");
  lr_operand(B, x, {pr.N, pr.r}, who, "lora_B");
  TORCH_CHECK(p >= 0.0 && p < 1.0, who, ": p in [0,1) (got ", p, ")");
  pr.drop = p > 0.0;
  if (pr.drop) {
    TORCH_CHECK(offset.has_value() && offset->is_cuda() &&
                    offset->device() == x.device() &&
                    offset->scalar_type() == at::kLong && offset->numel() == 1 &&
                    offset->is_contiguous(),
                who, ": p > 0 needs a one-element int64 offset tensor on x's "
                     "device");
  }
  return pr;
}

template <bool BWD>
static void lora_row_launch(const LoraRowArgs& a, bool drop, hipStream_t stream) {
  const dim3 grid(ceil_div(a.M, LR_ROWS));
  if (drop)
    hipLaunchKernelGGL((lora_row_kernel<BWD, true>), grid, dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL((lora_row_kernel<BWD, false>), grid, dim3(256), 0, stream, a);
}

// y [M,N] (= x W^T + b) += scaling * (dropout(x) A^T) B^T, in place
// -> {xa [M,r], offset_used [1] int64 (empty when p == 0)}
std::vector<at::Tensor> lora_fwd(at::Tensor y, const at::Tensor& x,
                                 const at::Tensor& A, const at::Tensor& B,
                                 double scaling, double p, int64_t seed,
                                 c10::optional<at::Tensor> offset) {
  const char* who = "lora_fwd";
  const LoraProblem pr = lora_check(x, A, B, p, offset, who);
  lr_operand(y, x, {pr.M, pr.N}, who, "y");
  auto xa = at::empty({pr.M, pr.r}, x.options());
  auto used = at::empty({pr.drop ? 1 : 0}, x.options().dtype(at::kLong));
  if (pr.M == 0) return {xa, used};
  LoraRowArgs a = {};
  a.in = x.data_ptr<float>();
  a.wd = A.data_ptr<float>();
  a.wu = B.data_ptr<float>();
  a.t = xa.data_ptr<float>();
  a.out = y.data_ptr<float>();
  a.offset_in = pr.drop ? offset->data_ptr<long>() : nullptr;
  a.offset_out = pr.drop ? used.data_ptr<long>() : nullptr;
  a.seed = pr.drop ? (uint64_t)seed : 0;
  a.M = (int)pr.M;
  a.C = (int)pr.K;
  a.D = (int)pr.N;
  a.r = (int)pr.r;
  a.tscale = 1.f;
  a.ucoef = (float)scaling;
  a.p = pr.drop ? (float)p : 0.f;
  a.inv_keep = pr.drop ? 1.0f / (1.0f - (float)p) : 1.f;   // = dropout_fwd_dev
  lora_row_launch<false>(a, pr.drop, c10::hip::getCurrentHIPStream().stream());
  return {xa, used};
}

// gx [M,K] (= g W), when given, += keep/(1-p) o (gxa A) in place, with
// gxa = scaling * g B; -> {gA [r,K], gB [N,r]}.  offset: what lora_fwd returned
std::vector<at::Tensor> lora_bwd(const at::Tensor& g, const at::Tensor& x,
                                 const at::Tensor& A, const at::Tensor& B,
                                 const at::Tensor& xa,
                                 c10::optional<at::Tensor> gx, double scaling,
                                 double p, int64_t seed,
                                 c10::optional<at::Tensor> offset) {
  const char* who = "lora_bwd";
  if (offset.has_value() && offset->numel() == 0) offset = c10::nullopt;
  const LoraProblem pr = lora_check(x, A, B, p, offset, who);
  lr_operand(g, x, {pr.M, pr.N}, who, "g");
  lr_operand(xa, x, {pr.M, pr.r}, who, "xa");
  if (gx.has_value()) lr_operand(*gx, x, {pr.M, pr.K}, who, "gx");
  auto gA = at::empty({pr.r, pr.K}, x.options());
  auto gB = at::empty({pr.N, pr.r}, x.options());
  auto stream = c10::hip::getCurrentHIPStream().stream();
  if (pr.M == 0) {
    slk_zero_async(gA.data_ptr<float>(), gA.numel(), stream);
    slk_zero_async(gB.data_ptr<float>(), gB.numel(), stream);
    return {gA, gB};
  }
  auto gxa = at::empty({pr.M, pr.r}, x.options());
  const float inv_keep = pr.drop ? 1.0f / (1.0f - (float)p) : 1.f;

  LoraRowArgs a = {};
  a.in = g.data_ptr<float>();
  a.wd = B.data_ptr<float>();
  a.wu = A.data_ptr<float>();
  a.t = gxa.data_ptr<float>();
  a.out = gx.has_value() ? gx->data_ptr<float>() : nullptr;
  a.offset_in = pr.drop ? offset->data_ptr<long>() : nullptr;
  a.seed = pr.drop ? (uint64_t)seed : 0;
  a.M = (int)pr.M;
  a.C = (int)pr.N;
  a.D = (int)pr.K;
  a.r = (int)pr.r;
  a.tscale = (float)scaling;
  a.ucoef = 1.f;
  a.p = pr.drop ? (float)p : 0.f;
  a.inv_keep = inv_keep;
  lora_row_launch<true>(a, pr.drop, stream);

  const int rows = lw_rows_per_slab(pr.M, pr.K, pr.N);
  const int slabs = ceil_div(pr.M, rows);
  auto slab = at::empty({(long)slabs * pr.r * (pr.K + pr.N)}, x.options());
  LoraWgradArgs w = {};
  w.x = x.data_ptr<float>();
  w.g = g.data_ptr<float>();
  w.xa = xa.data_ptr<float>();
  w.gxa = gxa.data_ptr<float>();
  w.slab_a = slab.data_ptr<float>();
  w.slab_b = w.slab_a + (long)slabs * pr.r * pr.K;   // r*K % 4 == 0: aligned
  w.offset = a.offset_in;
  w.seed = a.seed;
  w.M = (int)pr.M;
  w.K = (int)pr.K;
  w.N = (int)pr.N;
  w.r = (int)pr.r;
  w.rows_per_slab = rows;
  w.scaling = (float)scaling;
  w.p = a.p;
  w.inv_keep = inv_keep;
  const dim3 grid(ceil_div(pr.K, LW_COLS) + ceil_div(pr.N, LW_COLS), slabs);
  // same stream: gxa is complete before the weight-gradient kernel starts
  if (pr.drop)
    hipLaunchKernelGGL(lora_wgrad_kernel<true>, grid, dim3(256), 0, stream, w);
  else
    hipLaunchKernelGGL(lora_wgrad_kernel<false>, grid, dim3(256), 0, stream, w);
  slab_reduce_pair(w.slab_a, slabs, gA.data_ptr<float>(), gA.numel(), w.slab_b,
                   slabs, gB.data_ptr<float>(), gB.numel(), stream);
  return {gA, gB};
}

// ---- QKV-grouped adapters ----

int lora_qkv_wgrad_slabs(int64_t M, int64_t K, int64_t N) {
  TORCH_CHECK(M >= 1 && K >= 1 && N >= 1, "lora_qkv_wgrad_slabs: M, K, N >= 1");
  return ceil_div(M, lw_rows_per_slab(M, K, N));
}

// x and the three identically shaped adapters, in q, k, v order
static LoraProblem lora_qkv_check(const at::Tensor& x,
                                  const std::vector<at::Tensor>& As,
                                  const std::vector<at::Tensor>& Bs, double p,
                                  const c10::optional<at::Tensor>& offset,
                                  const char* who) {
  TORCH_CHECK(As.size() == LQ && Bs.size() == LQ, who,
              ": three lora_A and three lora_B (query, key, value)");
  const LoraProblem pr = lora_check(x, As[0], Bs[0], p, offset, who);
  for (int j = 1; j < LQ; ++j) {
    lr_operand(As[j], x, {pr.r, pr.K}, who, "lora_A");
    lr_operand(Bs[j], x, {pr.N, pr.r}, who, "lora_B");
  }
  return pr;
}

template <bool BWD>
static void lora_qkv_row_launch(const LoraQkvRowArgs& a, bool drop,
                                hipStream_t stream) {
  const dim3 grid(ceil_div(a.M, LR_ROWS));
  if (drop)
    hipLaunchKernelGGL((lora_qkv_row_kernel<BWD, true>), grid, dim3(256), 0,
                       stream, a);
  else
    hipLaunchKernelGGL((lora_qkv_row_kernel<BWD, false>), grid, dim3(256), 0,
                       stream, a);
}

// out [M,3N]: third j = base[j] + scaling * (dropout_j(x) A_j^T) B_j^T, where
// base[j] [M,N] = x W_j^T + b_j and dropout_j draws at the counter value the
// j-th of three successive lora_fwd calls would have read: offset is the live
// counter, already advanced by 3.
// -> {xa [3,M,r], offset_used [1] int64: q's offset (empty when p == 0)}
std::vector<at::Tensor> lora_qkv_fwd(at::Tensor out,
                                     const std::vector<at::Tensor>& base,
                                     const at::Tensor& x,
                                     const std::vector<at::Tensor>& As,
                                     const std::vector<at::Tensor>& Bs,
                                     double scaling, double p, int64_t seed,
                                     c10::optional<at::Tensor> offset) {
  const char* who = "lora_qkv_fwd";
  const LoraProblem pr = lora_qkv_check(x, As, Bs, p, offset, who);
  TORCH_CHECK(base.size() == LQ, who, ": three base products");
  for (int j = 0; j < LQ; ++j) lr_operand(base[j], x, {pr.M, pr.N}, who, "base");
  lr_operand(out, x, {pr.M, LQ * pr.N}, who, "out");
  auto xa = at::empty({LQ, pr.M, pr.r}, x.options());
  auto used = at::empty({pr.drop ? 1 : 0}, x.options().dtype(at::kLong));
  if (pr.M == 0) return {xa, used};
  LoraQkvRowArgs a = {};
  a.in = x.data_ptr<float>();
  a.ld_in = pr.K;
  for (int j = 0; j < LQ; ++j) {
    a.wd[j] = As[j].data_ptr<float>();
    a.wu[j] = Bs[j].data_ptr<float>();
    a.base[j] = base[j].data_ptr<float>();
  }
  a.t = xa.data_ptr<float>();
  a.ld_base = pr.N;
  a.out = out.data_ptr<float>();
  a.ld_out = LQ * pr.N;
  a.offset_in = pr.drop ? offset->data_ptr<long>() : nullptr;
  a.offset_out = pr.drop ? used.data_ptr<long>() : nullptr;
  a.seed = pr.drop ? (uint64_t)seed : 0;
  a.M = (int)pr.M;
  a.C = (int)pr.K;
  a.D = (int)pr.N;
  a.r = (int)pr.r;
  a.tscale = 1.f;
  a.ucoef = (float)scaling;
  a.p = pr.drop ? (float)p : 0.f;
  a.inv_keep = pr.drop ? 1.0f / (1.0f - (float)p) : 1.f;   // = dropout_fwd_dev
  lora_qkv_row_launch<false>(a, pr.drop,
                             c10::hip::getCurrentHIPStream().stream());
  return {xa, used};
}

// g [M,3N]: the packed gradient, unit column stride, any row stride that is a
// multiple of 4 floats (attention's own buffer, or a view of a wider one).
// gx [M,K] (= sum_j g_j W_j), when given, += sum_j keep_j/(1-p) o (gxa_j A_j)
// in place, gxa_j = scaling * g_j B_j; -> {gA [3,r,K], gB [3,N,r]}.
// offset: what lora_qkv_fwd returned
std::vector<at::Tensor> lora_qkv_bwd(const at::Tensor& g, const at::Tensor& x,
                                     const std::vector<at::Tensor>& As,
                                     const std::vector<at::Tensor>& Bs,
                                     const at::Tensor& xa,
                                     c10::optional<at::Tensor> gx,
                                     double scaling, double p, int64_t seed,
                                     c10::optional<at::Tensor> offset) {
  const char* who = "lora_qkv_bwd";
  if (offset.has_value() && offset->numel() == 0) offset = c10::nullopt;
  const LoraProblem pr = lora_qkv_check(x, As, Bs, p, offset, who);
  TORCH_CHECK(g.is_cuda() && g.scalar_type() == at::kFloat &&
                  g.device() == x.device() && g.dim() == 2 &&
                  g.size(0) == pr.M && g.size(1) == LQ * pr.N,
              who, ": g must be a float32 cuda tensor [M,3N] on x's device");
  const long ld_g = pr.M > 1 ? g.stride(0) : LQ * pr.N;
  TORCH_CHECK(g.stride(1) == 1 && ld_g >= LQ * pr.N && ld_g % 4 == 0 &&
                  (reinterpret_cast<uintptr_t>(g.data_ptr()) & 15) == 0,
              who, ": g needs a unit column stride, a row stride >= 3N that is"
                   " a multiple of 4, and a 16-byte aligned base");
  lr_operand(xa, x, {LQ, pr.M, pr.r}, who, "xa");
  if (gx.has_value()) lr_operand(*gx, x, {pr.M, pr.K}, who, "gx");
  auto gA = at::empty({LQ, pr.r, pr.K}, x.options());
  auto gB = at::empty({LQ, pr.N, pr.r}, x.options());
  auto stream = c10::hip::getCurrentHIPStream().stream();
  if (pr.M == 0) {
    slk_zero_async(gA.data_ptr<float>(), gA.numel(), stream);
    slk_zero_async(gB.data_ptr<float>(), gB.numel(), stream);
    return {gA, gB};
  }
  auto gxa = at::empty({LQ, pr.M, pr.r}, x.options());
  const float inv_keep = pr.drop ? 1.0f / (1.0f - (float)p) : 1.f;

  LoraQkvRowArgs a = {};
  a.in = g.data_ptr<float>();
  a.ld_in = ld_g;
  for (int j = 0; j < LQ; ++j) {
    a.wd[j] = Bs[j].data_ptr<float>();
    a.wu[j] = As[j].data_ptr<float>();
  }
  a.t = gxa.data_ptr<float>();
  a.out = gx.has_value() ? gx->data_ptr<float>() : nullptr;
  a.base[0] = a.out;
  a.ld_base = a.ld_out = pr.K;
  a.offset_in = pr.drop ? offset->data_ptr<long>() : nullptr;
  a.seed = pr.drop ? (uint64_t)seed : 0;
  a.M = (int)pr.M;
  a.C = (int)pr.N;
  a.D = (int)pr.K;
  a.r = (int)pr.r;
  a.tscale = (float)scaling;
  a.ucoef = 1.f;
  a.p = pr.drop ? (float)p : 0.f;
  a.inv_keep = inv_keep;
  lora_qkv_row_launch<true>(a, pr.drop, stream);

  const int rows = lw_rows_per_slab(pr.M, pr.K, pr.N);
  const int slabs = ceil_div(pr.M, rows);
  auto slab = at::empty({(long)slabs * LQ * pr.r * (pr.K + pr.N)}, x.options());
  LoraQkvWgradArgs w = {};
  w.x = x.data_ptr<float>();
  w.g = a.in;
  w.ld_g = ld_g;
  w.xa = xa.data_ptr<float>();
  w.gxa = gxa.data_ptr<float>();
  w.slab_a = slab.data_ptr<float>();
  w.slab_b = w.slab_a + (long)slabs * LQ * pr.r * pr.K;   // r*K % 4 == 0: aligned
  w.offset = a.offset_in;
  w.seed = a.seed;
  w.M = (int)pr.M;
  w.K = (int)pr.K;
  w.N = (int)pr.N;
  w.r = (int)pr.r;
  w.rows_per_slab = rows;
  w.scaling = (float)scaling;
  w.p = a.p;
  w.inv_keep = inv_keep;
  const dim3 grid(ceil_div(pr.K, LW_COLS) + LQ * ceil_div(pr.N, LW_COLS), slabs);
  // same stream: gxa is complete before the weight-gradient kernel starts
  if (pr.drop)
    hipLaunchKernelGGL(lora_qkv_wgrad_kernel<true>, grid, dim3(256), 0, stream, w);
  else
    hipLaunchKernelGGL(lora_qkv_wgrad_kernel<false>, grid, dim3(256), 0, stream, w);
  slab_reduce_pair(w.slab_a, slabs, gA.data_ptr<float>(), gA.numel(), w.slab_b,
                   slabs, gB.data_ptr<float>(), gB.numel(), stream);
  return {gA, gB};
}

}  // namespace slk
