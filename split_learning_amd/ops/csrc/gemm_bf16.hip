// bf16-operand MFMA GEMM for the three products of a Linear layer (gfx950).
//
// Mixed precision as a training framework means it: every tensor stays fp32 in
// memory; the operands are rounded to bf16 (nearest even, NaN and inf kept) on
// their way into LDS, multiplied by v_mfma_f32_32x32x16_bf16 and accumulated,
// biased and stored in fp32.  bf16 x bf16 products are exact in fp32, so the
// result is an fp32 sum of the exact products of the rounded operands.
//
//   NT  y [M,N] = x [M,K] . W[N,K]^T (+ bias)   forward
//   NN  gx[M,K] = gy[M,N] . W[N,K]              input gradient, reduces over N
//   TN  gW[N,K] = gy[M,N]^T . x[M,K]            weight gradient, reduces over M
//
// One kernel template serves all three as C[Mc,Nc] = sum_r A(m,r) B(n,r): an
// operand is either r-contiguous in memory ([row][r]: both NT operands, NN's
// A) or r-major ([r][row]: NN's B, both TN operands).  Whatever the memory
// order, both operands sit in LDS as [row][r] bf16, so a lane's MFMA operand
// (8 consecutive r of row lane & 31, r-group lane >> 5) is one ds_read_b128.
//
// Geometry: 256 threads = 2 x 2 waves on a BM x BN tile, each wave
// (BM/2) x (BN/2) in 32x32 MFMA blocks; an LDS stage holds GB_BK = 32 of r
// (two MFMA steps).  Two LDS stages, one barrier per stage: the next stage's
// global float4 loads are issued before the current stage's MFMAs and are
// converted and stored to the other buffer after them.
//
// LDS banks.  A row is 32 bf16 + 8 pad = 20 dwords (GB_LD = 40 bf16).
//   * b128 operand reads: lanes of one r-group read rows i, i+1, ... at dword
//     20 i + const, i.e. 16-byte slot (5 i) mod 16 of a 64-dword window (or
//     (5 i) mod 8 of a 32-dword one).  5 is odd, so 16 consecutive rows take 16
//     distinct slots (8 rows: 8 distinct): conflict-free whether the array
//     serves 64 or 32 dwords per clock.
//   * r-contiguous staging (b64 writes, a lane holds 4 r of a row = 2 dwords,
//     8 lanes per row): the lane -> row map (gb_rk_row) gives 32 consecutive
//     lanes the rows i, i+4, i+8, i+12, at dwords 80 j = 16 j (mod 64) for
//     j = 0..3: four disjoint 16-dword runs; a 16-lane half has rows i, i+4
//     at 0 and 16 (mod 32).  Conflict-free.
//   * r-major staging (the transpose; b32 writes): a lane loads rows
//     4q .. 4q+3 at r = 2p and 2p+1 and writes dword p of four rows.  One
//     write instruction has a fixed row offset within the quad; its 64 lanes
//     are 4 quads q x 16 pairs p at dword 80 q + p = 16 q + p (mod 64): 64
//     distinct banks.  Halving to 32 banks, lanes 0-31 hold pairs 0-7 for
//     q = 0, 1 and pairs 8-15 for q = 2, 3 (gb_rm_pair), i.e. dwords
//     16 (q & 1) + 8 (q >> 1) + (p & 7): 32 distinct.  Conflict-free.
//
// Edges: a float4 past the last row, or past the end of the reduction range,
// is not loaded (the load is predicated) and stages as zero.  The
// precondition (N % 8 == 0, K % 8 == 0) makes every float4 whole: it never
// straddles an edge along its contiguous dimension.  M is free: it is TN's
// reduction length and only ever indexes whole rows.
//
// The accumulators are computed transposed (mfma(B, A)): a lane then holds,
// for C row lane & 31, four runs of four consecutive columns, which go out as
// float4 stores (+ float4 bias for NT).
//
// TN reduces over M into an output as small as 768 x 768: its reduction is
// split into slabs (gb_plan) that slab_reduce sums in slab order.  No atomics:
// the same bits on every run.
//
// Resource use (hipcc -O3 --offload-arch=gfx950
// -Rpass-analysis=kernel-resource-usage; no scratch, no spills in any):
// see the table at gb_launch.
#include "torch_util.h"

namespace slk {
namespace {

using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned;

constexpr int GB_BK = 32;   // r per LDS stage
constexpr int GB_LD = 40;   // bf16 per LDS row (20 dwords, see above)
constexpr int GB_CUS = 256; // MI355X compute units

// two floats -> one dword of two bf16 (v_cvt_pk_bf16_f32: nearest even, NaN
// stays NaN, inf stays inf); lo is the lower r
__device__ __forceinline__ unsigned gb_pack(float lo, float hi) {
  const bf16x2 v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(unsigned, v);
}

// r-contiguous staging: thread -> (row within a 32-row pass, float4 along r)
__device__ __forceinline__ int gb_rk_row(int tid) {
  const int g = tid >> 3;
  return ((g & 3) << 2) | ((g >> 2) & 3) | (g & 16);
}

// r-major staging: lane -> r pair (0..15) for its row quad q
__device__ __forceinline__ int gb_rm_pair(int lane, int q) {
  return ((lane >> 2) & 7) | ((((lane >> 5) ^ (q >> 1)) & 1) << 3);
}

// One operand's stage: ROWS x GB_BK elements as ROWS / 32 float4 per thread.
// RM: the memory is [r][row] (row contiguous), else [row][r].
template <int ROWS, bool RM>
struct GbStage {
  static constexpr int NV = ROWS / 32;
  f32x4 v[NV];

  // rows [row0, row0 + ROWS) of `rows`, r in [r0, r0 + GB_BK) below r_end
  __device__ __forceinline__ void load(const float* __restrict__ p, int ld,
                                       int row0, int rows, int r0, int r_end,
                                       int tid) {
    if constexpr (!RM) {
      const int r = r0 + 4 * (tid & 7);
      #pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int row = row0 + i * 32 + gb_rk_row(tid);
        v[i] = f32x4{};
        if (row < rows && r < r_end)
          v[i] = *reinterpret_cast<const f32x4*>(p + (long)row * ld + r);
      }
    } else {
      const int lane = tid & 63, wave = tid >> 6;
      #pragma unroll
      for (int i = 0; i < NV / 2; ++i) {
        const int q = i * 16 + wave * 4 + (lane & 3);
        const int row = row0 + 4 * q;
        const int r = r0 + 2 * gb_rm_pair(lane, q);
        v[2 * i] = f32x4{};
        v[2 * i + 1] = f32x4{};
        if (row < rows && r < r_end)
          v[2 * i] = *reinterpret_cast<const f32x4*>(p + (long)r * ld + row);
        if (row < rows && r + 1 < r_end)
          v[2 * i + 1] =
              *reinterpret_cast<const f32x4*>(p + (long)(r + 1) * ld + row);
      }
    }
  }

  // convert and store as [row][r] bf16
  __device__ __forceinline__ void store(__bf16* lds, int tid) const {
    if constexpr (!RM) {
      #pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int row = i * 32 + gb_rk_row(tid);
        const u32x2 w = {gb_pack(v[i].x, v[i].y), gb_pack(v[i].z, v[i].w)};
        *reinterpret_cast<u32x2*>(lds + row * GB_LD + 4 * (tid & 7)) = w;
      }
    } else {
      const int lane = tid & 63, wave = tid >> 6;
      unsigned* l32 = reinterpret_cast<unsigned*>(lds);
      #pragma unroll
      for (int i = 0; i < NV / 2; ++i) {
        const int q = i * 16 + wave * 4 + (lane & 3);
        const int pr = gb_rm_pair(lane, q);
        #pragma unroll
        for (int j = 0; j < 4; ++j)
          l32[(4 * q + j) * (GB_LD / 2) + pr] =
              gb_pack(v[2 * i][j], v[2 * i + 1][j]);
      }
    }
  }
};

// C[Mc,Nc] (dense) = sum over r in this block's slab of A(m,r) B(n,r).
// blockIdx: x = M tile, y = N tile, z = reduction slab (C + z * Mc * Nc).
template <int BM, int BN, bool A_RM, bool B_RM>
__global__ __launch_bounds__(256) void gemm_bf16_kernel(
    const float* __restrict__ A, const float* __restrict__ B,
    float* __restrict__ C, const float* __restrict__ bias, int Mc, int Nc,
    int R, int lda, int ldb, int r_per_slab) {
  static_assert(BM % 64 == 0 && BN % 64 == 0, "2 x 2 waves of 32x32 blocks");
  constexpr int TM = BM / 64, TN = BN / 64;   // MFMA blocks per wave
  __shared__ __align__(16) __bf16 ldsA[2][BM * GB_LD];
  __shared__ __align__(16) __bf16 ldsB[2][BN * GB_LD];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int r_begin = blockIdx.z * r_per_slab;
  const int r_end = min(R, r_begin + r_per_slab);
  C += (long)blockIdx.z * Mc * Nc;

  GbStage<BM, A_RM> sa;
  GbStage<BN, B_RM> sb;
  f32x16 acc[TM][TN];
  #pragma unroll
  for (int i = 0; i < TM; ++i)
    #pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x16{};

  // this lane's operand rows: row (lane & 31) of each 32-block, r-group lane>>5
  const int frag = (lane & 31) * GB_LD + (lane >> 5) * 8;
  const int wm = (wave >> 1) * (BM / 2), wn = (wave & 1) * (BN / 2);

  sa.load(A, lda, m0, Mc, r_begin, r_end, tid);
  sb.load(B, ldb, n0, Nc, r_begin, r_end, tid);
  sa.store(ldsA[0], tid);
  sb.store(ldsB[0], tid);
  __syncthreads();

  int buf = 0;
  for (int r0 = r_begin; r0 < r_end; r0 += GB_BK, buf ^= 1) {
    const bool has_next = r0 + GB_BK < r_end;
    if (has_next) {   // in flight under the MFMAs below
      sa.load(A, lda, m0, Mc, r0 + GB_BK, r_end, tid);
      sb.load(B, ldb, n0, Nc, r0 + GB_BK, r_end, tid);
    }
    // both MFMA steps' operands are read up front: step 1's reads complete
    // while step 0's MFMAs issue
    bf16x8 a[2][TM], b[2][TN];
    #pragma unroll
    for (int s = 0; s < 2; ++s) {
      #pragma unroll
      for (int i = 0; i < TM; ++i)
        a[s][i] = *reinterpret_cast<const bf16x8*>(
            &ldsA[buf][(wm + i * 32) * GB_LD + frag + s * 16]);
      #pragma unroll
      for (int j = 0; j < TN; ++j)
        b[s][j] = *reinterpret_cast<const bf16x8*>(
            &ldsB[buf][(wn + j * 32) * GB_LD + frag + s * 16]);
    }
    #pragma unroll
    for (int s = 0; s < 2; ++s)
      #pragma unroll
      for (int i = 0; i < TM; ++i)
        #pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              b[s][j], a[s][i], acc[i][j], 0, 0, 0);
    if (has_next) {
      sa.store(ldsA[buf ^ 1], tid);
      sb.store(ldsB[buf ^ 1], tid);
    }
    // one barrier per stage: the stores above went to the buffer nobody
    // reads in this iteration, and the next iteration's stores go to the
    // buffer every wave has finished reading here
    __syncthreads();
  }

  // acc[i][j][4 g + t] = C[m][n + t], m = lane & 31, n = 8 g + 4 (lane >> 5)
  #pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m = m0 + wm + i * 32 + (lane & 31);
    #pragma unroll
    for (int j = 0; j < TN; ++j) {
      #pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n0 + wn + j * 32 + 8 * g + 4 * (lane >> 5);
        if (m < Mc && n < Nc) {
          f32x4 o = {acc[i][j][4 * g], acc[i][j][4 * g + 1],
                     acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
          if (bias != nullptr)
            o += *reinterpret_cast<const f32x4*>(bias + n);
          *reinterpret_cast<f32x4*>(C + (long)m * Nc + n) = o;
        }
      }
    }
  }
}

// Tile and slab choice, settled on MI355X (profiles/SUMMARY.md "bf16 MFMA
// GEMM").  A grid wants two blocks per CU, so that one block's barrier and
// load waits sit under another's MFMAs: at M = 4096 the 768-column outputs
// (192 tiles of 128x128) run fastest as 768 tiles of 64x64, the 3072-column
// ones as 768 tiles of 128x128.  So: the biggest tile whose grid reaches
// 2 x CUs, where a reduction that may split counts the slabs it could split
// into (every slab keeps at least four LDS stages); then as many slabs as
// bring the grid to one block per CU (768 x 768 over M = 4096: 36 tiles of
// 128x128 in 8 slabs beat 144 of 64x64 in 2).
struct GbPlan { int tile, slabs, r_per_slab; };
constexpr int GB_TILES[3][2] = {{128, 128}, {64, 128}, {64, 64}};

GbPlan gb_plan(int Mc, int Nc, int R, bool may_split, int tile) {
  const int stages = ceil_div(R, GB_BK);
  const long max_slabs = may_split ? std::max(1, stages / 4) : 1;
  auto grid = [&](int t) {
    return (long)ceil_div(Mc, GB_TILES[t][0]) * ceil_div(Nc, GB_TILES[t][1]);
  };
  if (tile < 0)
    tile = grid(0) * max_slabs >= 2 * GB_CUS ? 0
         : grid(1) * max_slabs >= 2 * GB_CUS ? 1 : 2;
  const long slabs =
      std::min<long>(ceil_div(GB_CUS, grid(tile)), max_slabs);
  const int r_per_slab = ceil_div(stages, slabs) * GB_BK;
  return {tile, ceil_div(R, r_per_slab), r_per_slab};
}

// VGPR / AGPR / LDS bytes / waves per SIMD of each instantiation (scratch 0,
// spills 0 in all nine):
//            NT                  NN                  TN
//  128x128   88 / 64 / 40960 / 3   88 / 64 / 40960 / 3   80 / 64 / 40960 / 3
//  64x128    68 / 32 / 30720 / 4   70 / 32 / 30720 / 4   62 / 32 / 30720 / 5
//  64x64     52 / 16 / 20480 / 7   52 / 16 / 20480 / 7   48 / 16 / 20480 / 8
template <bool A_RM, bool B_RM>
void gb_launch(const float* A, const float* B, float* C, const float* bias,
               int Mc, int Nc, int R, int lda, int ldb, const GbPlan& p,
               hipStream_t stream) {
  const dim3 grid(ceil_div(Mc, GB_TILES[p.tile][0]),
                  ceil_div(Nc, GB_TILES[p.tile][1]), p.slabs);
  TORCH_CHECK(grid.y <= 65535, "linear_bf16: too many column tiles");
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, A, B, C, bias, Mc,
                       Nc, R, lda, ldb, p.r_per_slab);
  };
  if (p.tile == 0) go(gemm_bf16_kernel<128, 128, A_RM, B_RM>);
  else if (p.tile == 1) go(gemm_bf16_kernel<64, 128, A_RM, B_RM>);
  else go(gemm_bf16_kernel<64, 64, A_RM, B_RM>);
}

void gb_check(const at::Tensor& t, const char* who, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.dim() == 2 &&
                  t.is_contiguous() && t.numel() < (1ll << 31) &&
                  (uintptr_t)t.data_ptr() % 16 == 0,
              who, ": ", name, " must be a dense 2-D fp32 GPU tensor below "
              "2^31 elements at a 16-byte-aligned address");
}

void gb_check_dims(int M, int N, int K, const char* who) {
  TORCH_CHECK(M >= 1 && N >= 8 && K >= 8 && N % 8 == 0 && K % 8 == 0 &&
                  (long)M * N < (1ll << 31) && (long)M * K < (1ll << 31),
              who, ": needs M >= 1 and N, K positive multiples of 8 (M=", M,
              " N=", N, " K=", K, ")");
}

}  // namespace

// y[M,N] = bf16(x)[M,K] . bf16(w)[N,K]^T + bias; tile: -1 lets gb_plan choose,
// 0..2 names a row of GB_TILES (measurement and tests)
at::Tensor linear_bf16_fwd(const at::Tensor& x, const at::Tensor& w,
                           c10::optional<at::Tensor> bias, int64_t tile) {
  const char* who = "linear_bf16_fwd";
  gb_check(x, who, "x");
  gb_check(w, who, "weight");
  TORCH_CHECK(x.size(1) == w.size(1) && x.device() == w.device() && tile < 3,
              who, ": x [M,K] and weight [N,K] on one device");
  const int M = x.size(0), N = w.size(0), K = x.size(1);
  gb_check_dims(M, N, K, who);
  const float* bp = nullptr;
  if (bias.has_value()) {
    TORCH_CHECK(bias->is_cuda() && bias->scalar_type() == at::kFloat &&
                    bias->dim() == 1 && bias->size(0) == N &&
                    bias->is_contiguous() &&
                    (uintptr_t)bias->data_ptr() % 16 == 0,
                who, ": bias must be a dense fp32 GPU [N] tensor, 16-byte "
                "aligned");
    bp = bias->data_ptr<float>();
  }
  auto y = at::empty({M, N}, x.options());
  gb_launch<false, false>(x.data_ptr<float>(), w.data_ptr<float>(),
                          y.data_ptr<float>(), bp, M, N, K, K, K,
                          gb_plan(M, N, K, false, (int)tile),
                          c10::hip::getCurrentHIPStream().stream());
  return y;
}

// gx[M,K] = bf16(gy)[M,N] . bf16(w)[N,K]
at::Tensor linear_bf16_bwd_input(const at::Tensor& gy, const at::Tensor& w,
                                 int64_t tile) {
  const char* who = "linear_bf16_bwd_input";
  gb_check(gy, who, "gy");
  gb_check(w, who, "weight");
  TORCH_CHECK(gy.size(1) == w.size(0) && gy.device() == w.device() && tile < 3,
              who, ": gy [M,N] and weight [N,K] on one device");
  const int M = gy.size(0), N = w.size(0), K = w.size(1);
  gb_check_dims(M, N, K, who);
  auto gx = at::empty({M, K}, gy.options());
  gb_launch<false, true>(gy.data_ptr<float>(), w.data_ptr<float>(),
                         gx.data_ptr<float>(), nullptr, M, K, N, N, K,
                         gb_plan(M, K, N, false, (int)tile),
                         c10::hip::getCurrentHIPStream().stream());
  return gx;
}

// gw[N,K] = bf16(gy)[M,N]^T . bf16(x)[M,K], the reduction over M in slabs
at::Tensor linear_bf16_bwd_weight(const at::Tensor& gy, const at::Tensor& x,
                                  int64_t tile) {
  const char* who = "linear_bf16_bwd_weight";
  gb_check(gy, who, "gy");
  gb_check(x, who, "x");
  TORCH_CHECK(gy.size(0) == x.size(0) && gy.device() == x.device() && tile < 3,
              who, ": gy [M,N] and x [M,K] on one device");
  const int M = x.size(0), N = gy.size(1), K = x.size(1);
  gb_check_dims(M, N, K, who);
  TORCH_CHECK((long)N * K < (1ll << 31), who, ": weight too large");
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const GbPlan p = gb_plan(N, K, M, true, (int)tile);
  const long numel = (long)N * K;
  auto gw = at::empty({N, K}, x.options());
  at::Tensor slab;
  if (p.slabs > 1) slab = at::empty({p.slabs * numel}, x.options());
  gb_launch<true, true>(gy.data_ptr<float>(), x.data_ptr<float>(),
                        p.slabs > 1 ? slab.data_ptr<float>()
                                    : gw.data_ptr<float>(),
                        nullptr, N, K, M, N, K, p, stream);
  if (p.slabs > 1)
    slab_reduce(slab.data_ptr<float>(), p.slabs, gw.data_ptr<float>(), numel,
                stream);
  return gw;
}

}  // namespace slk
