// Winograd F(2x2, 3x3) convolution for stride-1 3x3 convs (fp32).
// Op sites replaced: every 3x3 s1 Conv2d of the partitioned model zoo
// (reference src/model/VGG16_CIFAR10.py:10-94,
// other/Vanilla_SL/src/model/MobileNetv1_CIFAR10.py:23-167).
//
// y = A^T [ (G g G^T) .* (B^T d B) ] A   per 2x2 output tile (4x4 input
// patch, overlap 2).  2.25x fewer MACs than direct: the elementwise product
// becomes 16 frequency-batched GEMMs  M[f] = U[f][Co,Ci] @ V[f][Ci,T]
// (T = B * OH/2 * OW/2).  Backward-data is the same conv of gy with the
// 180-degree-rotated, Co/Ci-transposed weights at pad' = KH-1-p (FLIP /
// flip=true below).  Backward-weight has its own frequency form
// (dU[f] = (A gy A^T)[f] @ V_x[f]^T, gw = G^T dU G).
//
// The forms in this file; routing between them is measured per shape
// (conv_route.h):
//   conv2d_wino             unfused, three launches: wino_wt_in_kernel (both
//                           operand transforms), the batched MFMA GEMM of
//                           gemm_f32.hip, wino_out_kernel (sums the GEMM's
//                           split-K slabs).  V/M round-trip through HBM, so it
//                           wins where the GEMM is compute-dominated (the
//                           high-Ci tail of VGG16) and takes the shapes the
//                           fused kernel's tiles do not divide.
//   conv2d_wino_bwdw        unfused bwd-weight: wino_gyA_kernel,
//                           wino_in_kernel, GEMM over the tile axis,
//                           wino_gw_kernel.
//   conv2d_wino_fused       wino_fused_kernel<FLIP>: transforms in-kernel, 16-
//                           frequency MFMA accumulation, no V/M round trip.
//   conv2d_wino_bwdw_fused  wino_bwdw_fused_kernel, its bwd-weight twin.
//   conv2d_bwd_pair         wino_bwd_pair_kernel: the bodies of the two fused
//                           backward kernels in one grid.
// Every transform's arithmetic is in wino_math.h, once, and each kernel here
// calls it: that is what keeps the forms bit-identical to each other.  Each
// fused kernel takes one argument struct (WinoFusedArgs, WinoBwdwArgs) that
// one host function fills for the standalone entry and for the pair.
#include <tuple>
#include <type_traits>

#include "torch_util.h"
#include "wino_math.h"

namespace slk {

// weight transform U[f] = (G g G^T)[f] over the weight's true dims
// (Cw0, Cw1) = (w.size(0), w.size(1)); FLIP writes U[f][Cw1][Cw0] with the
// taps rotated 180 degrees (the bwd-data weight), else U[f][Cw0][Cw1].
// (block, nblocks): the launch's blocks that work on this transform — a share
// of wino_wt_in_kernel's grid
template <bool FLIP>
__device__ __forceinline__ void wino_wt_body(const float* __restrict__ w,
                                             float* __restrict__ U, int Cw0,
                                             int Cw1, int block, int nblocks) {
  // thread per (channel pair, frequency ROW): 4x the threads of the obvious
  // per-pair mapping — the small conv weights (64x64: 4096 pairs) gave a
  // 16-BLOCK grid on a 256-CU chip and the launch ran latency-bound at 7-9
  // us; the 4x re-read of w is noise next to that
  const long total = (long)Cw0 * Cw1;
  const long tstride = (long)nblocks * blockDim.x;
  for (long e = (long)block * blockDim.x + threadIdx.x; e < 4 * total;
       e += tstride) {
    const int a = (int)(e & 3);          // frequency row
    const long i = e >> 2;
    const int cols = FLIP ? Cw0 : Cw1;
    const int c = (int)(i % cols);
    const int r = (int)(i / cols);
    const int co = FLIP ? c : r;   // index into w's dim 0
    const int ci = FLIP ? r : c;   // index into w's dim 1
    // row a of G g
    float t[3];
    #pragma unroll
    for (int b = 0; b < 3; ++b) {
      const float g0 = w[(((long)co * Cw1 + ci) * 3 + (FLIP ? 2 : 0)) * 3 +
                         (FLIP ? 2 - b : b)];
      const float g1 = w[(((long)co * Cw1 + ci) * 3 + 1) * 3 +
                         (FLIP ? 2 - b : b)];
      const float g2 = w[(((long)co * Cw1 + ci) * 3 + (FLIP ? 0 : 2)) * 3 +
                         (FLIP ? 2 - b : b)];
      t[b] = wino_G_row(a, g0, g1, g2);
    }
    const f32x4 u = wino_GgGt_row(t);
    #pragma unroll
    for (int b = 0; b < 4; ++b) U[((long)(a * 4 + b) * total) + i] = u[b];
  }
}

// input transform V[f][Ci][T], T = B*tH*tW, tile t = (b, th, tw); the 4x4
// patch starts at (th*2 - pad, tw*2 - pad), zero-padded at the borders
__device__ __forceinline__ void wino_in_body(
    const float* __restrict__ x, float* __restrict__ V, int B, int Ci, int H,
    int W, int tH, int tW, int pad, const FastDiv& d_T, const FastDiv& d_thw,
    const FastDiv& d_tw, int block, int nblocks) {
  const int T = B * tH * tW;
  const long total = (long)Ci * T;
  const long stride = (long)nblocks * blockDim.x;
  for (long i = (long)block * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    const unsigned cc = d_T.div((unsigned)i);
    const unsigned t = d_T.mod((unsigned)i, cc);
    const WinoTile tl = wino_tile(t, d_thw, d_tw);
    float d[4][4];
    wino_load_patch(d, x + ((long)tl.b * Ci + cc) * H * W, (int)tl.th * 2 - pad,
                    (int)tl.tw * 2 - pad, H, W);
    float u[4][4];
    wino_Bt_d(u, d);
    #pragma unroll
    for (int a = 0; a < 4; ++a) {
      const f32x4 v = wino_BtdB_row(u, a);
      #pragma unroll
      for (int bb = 0; bb < 4; ++bb)
        V[((long)(a * 4 + bb) * Ci + cc) * T + t] = v[bb];
    }
  }
}

__global__ void wino_in_kernel(const float* __restrict__ x,
                               float* __restrict__ V, int B, int Ci, int H,
                               int W, int tH, int tW, int pad, FastDiv d_T,
                               FastDiv d_thw, FastDiv d_tw) {
  wino_in_body(x, V, B, Ci, H, W, tH, tW, pad, d_T, d_thw, d_tw, blockIdx.x,
               gridDim.x);
}

// Both operand transforms of conv2d_wino in ONE launch: they are independent
// (U from w, V from x) and each alone underfills or barely fills the chip for
// a few microseconds, so as two launches the second waits out the first's
// drain.  The first in_blocks blocks run the input transform — the short
// one, so its blocks retire while the weight transform's stream in behind
// them — the rest the weight transform.
template <bool FLIP>
__global__ void wino_wt_in_kernel(const float* __restrict__ w,
                                  float* __restrict__ U, int Cw0, int Cw1,
                                  const float* __restrict__ x,
                                  float* __restrict__ V, int B, int Ci, int H,
                                  int W, int tH, int tW, int pad, FastDiv d_T,
                                  FastDiv d_thw, FastDiv d_tw, int in_blocks) {
  if ((int)blockIdx.x < in_blocks) {
    wino_in_body(x, V, B, Ci, H, W, tH, tW, pad, d_T, d_thw, d_tw, blockIdx.x,
                 in_blocks);
  } else {
    wino_wt_body<FLIP>(w, U, Cw0, Cw1, blockIdx.x - in_blocks,
                       gridDim.x - in_blocks);
  }
}

// output transform y[b][co][2th..][2tw..] = A^T M A (+bias), with the
// frequency GEMM's split-K sum folded in: M arrives as `splits` slabs
// (slab_stride floats apart) and each element is summed here in
// slab_reduce_body's order and form (0.f, then slab 0, 1, ...), so the
// separate reduce launch and the write and re-read of the summed M go away and
// the result keeps its bits.
//
// A block owns 64 consecutive (co, t) pairs; wave a sums frequency row a
// (f = 4a .. 4a+3) of each, so a pair's 16*splits loads spread over four
// threads — the 2x2 layers have only Co*T = 16 K pairs, a quarter of a block
// per CU at a thread per pair.  The sums meet in LDS and thread (pair, a) then
// forms output pixel (a >> 1, a & 1) with the expression order of a
// thread-per-pair transform.
__global__ __launch_bounds__(256) void wino_out_kernel(
    const float* __restrict__ Mm, int splits, long slab_stride,
    float* __restrict__ y, const float* __restrict__ bias, int B, int Co,
    int OH, int OW, int tH, int tW, FastDiv d_T, FastDiv d_thw, FastDiv d_tw) {
  __shared__ float ml[16][64];
  const int T = B * tH * tW;
  const long total = (long)Co * T;
  const int p = threadIdx.x & 63;
  const int a = threadIdx.x >> 6;
  for (long i0 = (long)blockIdx.x * 64; i0 < total; i0 += (long)gridDim.x * 64) {
    const long i = i0 + p;
    const bool live = i < total;
    const unsigned co = d_T.div((unsigned)(live ? i : total - 1));
    const unsigned t = d_T.mod((unsigned)(live ? i : total - 1), co);
    const float* mp = Mm + ((long)(a * 4) * Co + co) * T + t;
    const long fs = (long)Co * T;   // frequency stride
    float m[4];
    #pragma unroll
    for (int bb = 0; bb < 4; ++bb) m[bb] = mp[bb * fs];
    if (splits > 1) {
      #pragma unroll
      for (int bb = 0; bb < 4; ++bb) m[bb] = 0.f + m[bb];
      for (int k = 1; k < splits; ++k) {
        const float* mk = mp + (long)k * slab_stride;
        #pragma unroll
        for (int bb = 0; bb < 4; ++bb) m[bb] += mk[bb * fs];
      }
    }
    #pragma unroll
    for (int bb = 0; bb < 4; ++bb) ml[a * 4 + bb][p] = m[bb];
    __syncthreads();
    if (live) {
      float mf[4][4];
      #pragma unroll
      for (int f = 0; f < 16; ++f) mf[f >> 2][f & 3] = ml[f][p];
      const int oi = a >> 1, oj = a & 1;
      const float bv = bias != nullptr ? bias[co] : 0.f;
      const WinoTile tl = wino_tile(t, d_thw, d_tw);
      float* yp = y + ((long)tl.b * Co + co) * OH * OW +
                  (long)(tl.th * 2 + oi) * OW + tl.tw * 2 + oj;
      *yp = wino_AtmA(mf, oi, oj, bv);
    }
    __syncthreads();
  }
}

// ---- backward-weight --------------------------------------------------
// dY arrives per 2x2 output tile; dM = A dY A^T lifts it to the 4x4
// frequency domain, then
// dU[f][Co][Ci] = dM[f][Co,T] @ V_x[f][Ci,T]^T (16 frequency GEMMs over the
// tile axis — a far better GEMM shape than the direct gather's
// [Co, Ci*9, B*OH*OW] tall-K formulation), and gw = G^T dU G.
__global__ void wino_gyA_kernel(const float* __restrict__ gy,
                                float* __restrict__ Wg, int B, int Co, int OH,
                                int OW, int tH, int tW, FastDiv d_T,
                                FastDiv d_thw, FastDiv d_tw) {
  const int T = B * tH * tW;
  const long total = (long)Co * T;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    const unsigned co = d_T.div((unsigned)i);
    const unsigned t = d_T.mod((unsigned)i, co);
    const WinoTile tl = wino_tile(t, d_thw, d_tw);
    const float* gp = gy + ((long)tl.b * Co + co) * OH * OW
                      + (long)tl.th * 2 * OW + tl.tw * 2;
    const float g00 = gp[0], g01 = gp[1], g10 = gp[OW], g11 = gp[OW + 1];
    #pragma unroll
    for (int a = 0; a < 4; ++a) {
      const f32x4 m = wino_AgAt_row(a, g00, g01, g10, g11);
      #pragma unroll
      for (int bb = 0; bb < 4; ++bb)
        Wg[((long)(a * 4 + bb) * Co + co) * T + t] = m[bb];
    }
  }
}

__global__ void wino_gw_kernel(const float* __restrict__ dU,
                               float* __restrict__ gw, int Co, int Ci) {
  const long total = (long)Co * Ci;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    float u[4][4];
    #pragma unroll
    for (int f = 0; f < 16; ++f) u[f >> 2][f & 3] = dU[(long)f * total + i];
    float g[3][3];
    wino_GtuG(g, u);
    #pragma unroll
    for (int k = 0; k < 9; ++k) gw[i * 9 + k] = g[k / 3][k % 3];
  }
}

at::Tensor matmul_f32(const at::Tensor&, const at::Tensor&, bool, bool,
                      c10::optional<at::Tensor>, bool);
at::Tensor matmul_f32_slabs(const at::Tensor&, const at::Tensor&);
int matmul_f32_slab_count(int, int, int, int);

// split-K slabs wino_out_kernel sums for Co output and Ci input channels over
// T tiles (M[f] = U[f][Co,Ci] @ V[f][Ci,T], batch 16)
int conv2d_wino_slabs(int Co, int Ci, int T) {
  return matmul_f32_slab_count(16, Co, T, Ci);
}

// tile grid of a [B, *, OH, OW] output and the dividers that decode an index
// over it (wino_tile)
struct WinoTiles {
  int tH, tW, T;
  FastDiv d_T, d_thw, d_tw;
};

static WinoTiles wino_tiles(int B, int OH, int OW) {
  WinoTiles g;
  g.tH = OH / 2;
  g.tW = OW / 2;
  g.T = B * g.tH * g.tW;
  g.d_T.init(g.T);
  g.d_thw.init(g.tH * g.tW);
  g.d_tw.init(g.tW);
  return g;
}

// grid of a 256-thread grid-stride transform kernel over `threads` elements
static int wino_grid(long threads, int cap) {
  return (int)std::min<long>((threads + 255) / 256, cap);
}

// launch(std::true_type or std::false_type): the one place a run-time flip
// picks a kernel's FLIP instantiation
template <class Launch>
static void wino_dispatch_flip(bool flip, Launch&& launch) {
  if (flip) launch(std::true_type{});
  else launch(std::false_type{});
}

// host entry: 3x3 stride-1 conv via F(2x2,3x3); flip=true computes the
// bwd-data conv (weights rotated + Co/Ci transposed, pad' = 2 - pad)
at::Tensor conv2d_wino(const at::Tensor& x, const at::Tensor& w,
                       c10::optional<at::Tensor> bias, int pad, bool flip) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && x.scalar_type() == at::kFloat);
  TORCH_CHECK(w.size(2) == 3 && w.size(3) == 3, "wino: 3x3 only");
  auto xc = x.contiguous();
  auto wc = w.contiguous();
  const int B = x.size(0), H = x.size(2), W = x.size(3);
  const int Co = flip ? w.size(1) : w.size(0);
  const int Ci = flip ? w.size(0) : w.size(1);
  TORCH_CHECK(x.size(1) == Ci, "wino: channel mismatch");
  const int OH = H + 2 * pad - 2, OW = W + 2 * pad - 2;
  TORCH_CHECK(OH % 2 == 0 && OW % 2 == 0, "wino: even output dims only");
  const WinoTiles g = wino_tiles(B, OH, OW);
  auto stream = c10::hip::getCurrentHIPStream().stream();

  auto U = at::empty({16, Co, Ci}, x.options());
  auto V = at::empty({16, Ci, g.T}, x.options());
  // weight transform: thread per (pair, freq row), always over the WEIGHT's
  // own dims (FLIP handles the transpose internally); input transform:
  // thread per (ci, tile)
  const int wt_grid = wino_grid((long)Co * Ci * 4, 4096);
  const int in_grid = wino_grid((long)Ci * g.T, 8192);
  const int Cw0 = (int)w.size(0), Cw1 = (int)w.size(1);
  wino_dispatch_flip(flip, [&](auto F) {
    hipLaunchKernelGGL(wino_wt_in_kernel<decltype(F)::value>,
                       dim3(in_grid + wt_grid), dim3(256), 0, stream,
                       wc.data_ptr<float>(), U.data_ptr<float>(), Cw0, Cw1,
                       xc.data_ptr<float>(), V.data_ptr<float>(), B, Ci, H, W,
                       g.tH, g.tW, pad, g.d_T, g.d_thw, g.d_tw, in_grid);
  });
  // M[f] = U[f] @ V[f]: one batched MFMA GEMM launch (batch = 16); its
  // split-K slabs [splits, 16, Co, T] go to the output transform unreduced
  auto Mm = matmul_f32_slabs(U, V);
  auto y = at::empty({B, Co, OH, OW}, x.options());
  // 64 (co, t) pairs per block
  const int out_grid = (int)std::min<long>(((long)Co * g.T + 63) / 64, 8192);
  hipLaunchKernelGGL(wino_out_kernel, dim3(out_grid), dim3(256), 0, stream,
                     Mm.data_ptr<float>(), (int)Mm.size(0), 16l * Co * g.T,
                     y.data_ptr<float>(),
                     bias.has_value() ? bias->data_ptr<float>() : nullptr, B,
                     Co, OH, OW, g.tH, g.tW, g.d_T, g.d_thw, g.d_tw);
  return y;
}

at::Tensor conv2d_wino_bwdw(const at::Tensor& gy, const at::Tensor& x,
                            int pad) {
  TORCH_CHECK(gy.is_cuda() && x.is_cuda() && gy.dim() == 4 && x.dim() == 4);
  auto gyc = gy.contiguous();
  auto xc = x.contiguous();
  const int B = x.size(0), Ci = x.size(1), H = x.size(2), W = x.size(3);
  const int Co = gy.size(1), OH = gy.size(2), OW = gy.size(3);
  TORCH_CHECK(OH == H + 2 * pad - 2 && OW == W + 2 * pad - 2,
              "wino_bwdw geometry");
  TORCH_CHECK(OH % 2 == 0 && OW % 2 == 0, "wino_bwdw: even output dims only");
  const WinoTiles g = wino_tiles(B, OH, OW);
  auto stream = c10::hip::getCurrentHIPStream().stream();

  auto Wg = at::empty({16, Co, g.T}, x.options());
  auto Vx = at::empty({16, Ci, g.T}, x.options());
  hipLaunchKernelGGL(wino_gyA_kernel, dim3(wino_grid((long)Co * g.T, 8192)),
                     dim3(256), 0, stream, gyc.data_ptr<float>(),
                     Wg.data_ptr<float>(), B, Co, OH, OW, g.tH, g.tW, g.d_T,
                     g.d_thw, g.d_tw);
  hipLaunchKernelGGL(wino_in_kernel, dim3(wino_grid((long)Ci * g.T, 8192)),
                     dim3(256), 0, stream, xc.data_ptr<float>(),
                     Vx.data_ptr<float>(), B, Ci, H, W, g.tH, g.tW, pad, g.d_T,
                     g.d_thw, g.d_tw);
  // dU[f][Co][Ci] = Wg[f] @ Vx[f]^T : 16 frequency GEMMs, K = tiles
  auto dU = matmul_f32(Wg, Vx, false, true, c10::nullopt, false);
  auto gw = at::empty({Co, Ci, 3, 3}, x.options());
  hipLaunchKernelGGL(wino_gw_kernel, dim3(wino_grid((long)Co * Ci, 4096)),
                     dim3(256), 0, stream, dU.data_ptr<float>(),
                     gw.data_ptr<float>(), Co, Ci);
  return gw;
}


// ---- fused F(2x2,3x3) kernel ------------------------------------------
// One kernel: input transform in-register, 16-frequency MFMA accumulation,
// output transform in the epilogue — no V/M HBM round trip (the unfused
// pipeline's 4x data inflation).  A block owns a (32 co x 32 tile) output
// patch across ALL 16 frequencies, so each 4x4 input patch is read once and
// feeds every frequency.  Per wave: 16x16 (co, t) fragment x 16 freq = 16
// f32x4 accumulators (64 registers).  K-loop over ci in steps of 8.
// Weights arrive raw; U = G w G^T is computed while staging.
constexpr int WF_CO = 32;   // block co tile
constexpr int WF_T = 32;    // block tile-column tile
constexpr int WF_CK = 8;    // ci step
// LDS operand layout, both operands and all three fused kernels:
// [row 32][k 8][f 16] floats — the 16 frequency values of one (row, k) element
// are contiguous, so an MFMA lane fetches a frequency quad of its (row, k)
// with one ds_read_b128 (16 wide reads per wave per K-step).  Strides in
// floats: k 20, row 168.  ds_read_b128 is served in four 16-lane groups
// ({0-3,12-15,20-27}, {4-11,16-19,28-31}, +32) over 16 sixteen-byte slots;
// lane (r = lane>>4, c = lane&15) reads slot (42c + 5r + const) mod 16 =
// (10c + 5r) mod 16: within a group the r-even lanes take the eight even
// slots and the r-odd lanes the eight odd ones, each once — conflict-free.
// Staging stores are ds_write_b128 (8-lane groups, eight slots): k-fast
// threads (weights, both bwd-weight operands) hit slots 5k mod 8, all
// distinct; the row-fast V staging hits 42*row mod 8 = 2*row mod 8, a 2-way
// conflict on 4 of the 8 stores a thread makes per step.
constexpr int WF_KS = 20;                  // k stride
constexpr int WF_RS = 168;                 // row stride
constexpr int WF_OP = 32 * WF_RS;          // floats per staged operand (21 KB)

// The 32 MFMAs of one K-step for a wave, operands read from the layout above.
// pa / pb point at the lane's (row, k = lane>>4) element of each operand; the
// kk = 1 half sits 4 k-rows further.  Reads for frequency quad g+1 are issued
// before the MFMAs of quad g, and inside a quad the four kk = 0 MFMAs go
// before the four kk = 1 ones, so no MFMA waits on the one just issued.  Each
// acc[f] still receives kk = 0 then kk = 1 of its own frequency.
__device__ __forceinline__ void wino_kstep_mfma(const float* pa,
                                                const float* pb,
                                                f32x4 (&acc)[16]) {
  const f32x4* a0 = reinterpret_cast<const f32x4*>(pa);
  const f32x4* a1 = reinterpret_cast<const f32x4*>(pa + 4 * WF_KS);
  const f32x4* b0 = reinterpret_cast<const f32x4*>(pb);
  const f32x4* b1 = reinterpret_cast<const f32x4*>(pb + 4 * WF_KS);
  f32x4 ra0 = a0[0], rb0 = b0[0], ra1 = a1[0], rb1 = b1[0];
  #pragma unroll
  for (int g = 0; g < 4; ++g) {
    const f32x4 ca0 = ra0, cb0 = rb0, ca1 = ra1, cb1 = rb1;
    if (g < 3) {
      ra0 = a0[g + 1];
      rb0 = b0[g + 1];
      ra1 = a1[g + 1];
      rb1 = b1[g + 1];
    }
    // keep the reads above ahead of this quad's MFMAs: the scheduler
    // otherwise sinks them to just before their first use
    __builtin_amdgcn_sched_barrier(0);
    #pragma unroll
    for (int j = 0; j < 4; ++j)
      acc[g * 4 + j] = __builtin_amdgcn_mfma_f32_16x16x4f32(
          ca0[j], cb0[j], acc[g * 4 + j], 0, 0, 0);
    #pragma unroll
    for (int j = 0; j < 4; ++j)
      acc[g * 4 + j] = __builtin_amdgcn_mfma_f32_16x16x4f32(
          ca1[j], cb1[j], acc[g * 4 + j], 0, 0, 0);
  }
}

// wino_fused_kernel's arguments: the conv of x [B, Ci, H, W] with w into
// y [B, Co, OH, OW] over a [B][tH][tW] tile grid.  CW: w.size(1), the stride
// of w's dim 0 in 3x3 taps (Ci, or Co under FLIP).  Filled by
// wino_fused_args.
struct WinoFusedArgs {
  const float* x;
  const float* w;
  const float* bias;   // or nullptr
  float* y;            // [nz] slabs of B*Co*OH*OW when nz > 1
  int B, Ci, H, W, Co, OH, OW, tH, tW, pad;
  int ci_per;          // ci range of one grid.z slice
  int CW;
  FastDiv d_thw, d_tw;
  int nx, ny, nz;      // grid: T / 32, Co / 32, ci slices
};

// ci_per: the ci-range length per grid.z slice.  The output transform is
// LINEAR in M, so slices transform their PARTIAL sums, each into its own
// slab of y (y + blockIdx.z * B*Co*OH*OW), reduced in fixed order by
// slab_reduce — this fills the chip for small-T/high-Ci shapes
// whose natural grid is far below one block per CU, and unlike atomicAdd
// gives the same sum every run.  Slice 0 adds the bias.
//
// The body is a device function over a VIRTUAL block index (bx, by, bz) and
// the caller's two LDS operand arrays, so wino_bwd_pair_kernel can run it next
// to the bwd-weight body in one grid; wino_fused_kernel passes its blockIdx.
template <bool FLIP>
__device__ __forceinline__ void wino_fused_body(
    float (&Ul)[WF_OP], float (&Vl)[WF_OP], unsigned bx, unsigned by, unsigned bz,
    const WinoFusedArgs& p) {
  const float* __restrict__ x = p.x;
  const float* __restrict__ w = p.w;
  const int H = p.H, W = p.W, Co = p.Co, OH = p.OH, OW = p.OW;
  const int ci_begin = bz * p.ci_per;
  const int ci_end = min(p.Ci, ci_begin + p.ci_per);
  // Ul [co][ci][f], Vl [t][ci][f]

  const int T = p.B * p.tH * p.tW;
  const int co0 = by * WF_CO;
  const int t0 = bx * WF_T;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wco = (wid >> 1) * 16;   // wave offset in the 32-co tile
  const int wt = (wid & 1) * 16;     // wave offset in the 32-t tile
  const int frag_r = lane >> 4;      // k sub-index (0..3)
  const int frag_c = lane & 15;

  f32x4 acc[16];
  #pragma unroll
  for (int f = 0; f < 16; ++f) acc[f] = f32x4{};

  // staging assignments -----------------------------------------------
  // V: thread -> one (ci, t) pair: ci = tid >> 5 (8), t = tid & 31 (32)
  const int v_ci = tid >> 5;
  const int v_t = tid & 31;
  const WinoTile vt = wino_tile((unsigned)(t0 + v_t), p.d_thw, p.d_tw);
  const int ih0 = (int)vt.th * 2 - p.pad;
  const int iw0 = (int)vt.tw * 2 - p.pad;
  const long xplane = ((long)vt.b * p.Ci + v_ci) * H * W;
  // weights: thread -> one (co, ci) pair (32co x 8ci = 256); the 3x3 taps
  // load raw and transform IN-KERNEL (U = G w G^T, the exact wino_wt math) —
  // the separate wt launch and the 16*Co*Ci frequency tensor's HBM
  // write+read round trip disappear.  FLIP (bwd-data) swaps the channel
  // roles and rotates the taps 180 deg ((2-r, 2-s) == tap 8-k).
  const int w_co = tid >> 3;
  const int w_ci = tid & 7;

  // software pipeline: next step's 4x4 patch + 9 weight taps load into
  // registers UNDER the (long, 32-MFMA) compute phase; the transforms + LDS
  // stores run at the top of the next iteration
  // the 9 taps stay in the registers their (4+4+1)-dword loads fill: as nine
  // scalars the loop-carried copies out of those loads sat right behind them,
  // with the vmcnt wait that exposes the whole global latency every step
  float d[4][4];
  f32x4 wq0, wq1;
  float w8;

  auto load_regs = [&](int ci0) {
    wino_load_patch(d, x + xplane + (long)ci0 * H * W, ih0, iw0, H, W);
    const long wbase = FLIP
        ? ((long)(ci0 + w_ci) * p.CW + (co0 + w_co)) * 9
        : ((long)(co0 + w_co) * p.CW + (ci0 + w_ci)) * 9;
    using f32x4u = __attribute__((ext_vector_type(4), aligned(4))) float;
    wq0 = *reinterpret_cast<const f32x4u*>(w + wbase);
    wq1 = *reinterpret_cast<const f32x4u*>(w + wbase + 4);
    w8 = w[wbase + 8];
  };

  auto store_stage = [&]() {
    float u[4][4];
    wino_Bt_d(u, d);
    f32x4* vp = reinterpret_cast<f32x4*>(&Vl[v_t * WF_RS + v_ci * WF_KS]);
    #pragma unroll
    for (int a = 0; a < 4; ++a) vp[a] = wino_BtdB_row(u, a);
    // U = G w G^T for this thread's (co, ci) pair — the expressions of
    // wino_wt_body (wino_math.h), so the result is bit-identical to the
    // staged path
    const float raw[9] = {wq0[0], wq0[1], wq0[2], wq0[3], wq1[0],
                          wq1[1], wq1[2], wq1[3], w8};
    float wr[9];
    #pragma unroll
    for (int k = 0; k < 9; ++k) wr[k] = raw[FLIP ? 8 - k : k];
    f32x4* up = reinterpret_cast<f32x4*>(&Ul[w_co * WF_RS + w_ci * WF_KS]);
    #pragma unroll
    for (int a = 0; a < 4; ++a) {
      float t[3];
      #pragma unroll
      for (int bb = 0; bb < 3; ++bb)
        t[bb] = wino_G_row(a, wr[bb], wr[3 + bb], wr[6 + bb]);
      up[a] = wino_GgGt_row(t);
    }
  };

  const float* pa = &Ul[(wco + frag_c) * WF_RS + frag_r * WF_KS];
  const float* pb = &Vl[(wt + frag_c) * WF_RS + frag_r * WF_KS];

  load_regs(ci_begin);
  for (int ci0 = ci_begin; ci0 < ci_end; ci0 += WF_CK) {
    store_stage();
    __syncthreads();
    if (ci0 + WF_CK < ci_end) load_regs(ci0 + WF_CK);
    wino_kstep_mfma(pa, pb, acc);
    __syncthreads();
  }

  // epilogue: lane holds, per freq, rows co = wco + frag_r*4 + i (i<4) at
  // col t = wt + frag_c -> all 16 freqs of each (co, t): y = A^T M A + bias
  #pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int co = co0 + wco + frag_r * 4 + i;
    const int t = t0 + wt + frag_c;
    if (co >= Co || t >= T) continue;
    float m[4][4];
    #pragma unroll
    for (int f = 0; f < 16; ++f) m[f >> 2][f & 3] = acc[f][i];
    const float bv = (p.bias != nullptr && bz == 0) ? p.bias[co] : 0.f;
    const WinoTile tl = wino_tile((unsigned)t, p.d_thw, p.d_tw);
    float* yp = p.y + (long)bz * p.B * Co * OH * OW +
                ((long)tl.b * Co + co) * OH * OW + (long)tl.th * 2 * OW +
                tl.tw * 2;
    const float o00 = wino_AtmA(m, 0, 0, bv);
    const float o01 = wino_AtmA(m, 0, 1, bv);
    const float o10 = wino_AtmA(m, 1, 0, bv);
    const float o11 = wino_AtmA(m, 1, 1, bv);
    yp[0] = o00;
    yp[1] = o01;
    yp[OW] = o10;
    yp[OW + 1] = o11;
  }
}

template <bool FLIP>
__global__ __launch_bounds__(256, 3) void wino_fused_kernel(WinoFusedArgs p) {
  // single-buffer two-barrier loop: double buffering would cost 84 KB of
  // LDS (1 block/CU); at 42 KB three blocks fit, which is what the
  // launch bound allows anyway
  __shared__ __attribute__((aligned(16))) float Ul[WF_OP];   // [co][ci][f]
  __shared__ __attribute__((aligned(16))) float Vl[WF_OP];   // [t][ci][f]
  wino_fused_body<FLIP>(Ul, Vl, blockIdx.x, blockIdx.y, blockIdx.z, p);
}

// wino_bwdw_fused_kernel's arguments: gw slabs [nz][Co][Ci][3][3] of the
// layer x [B, Ci, H, W] -> gy [B, Co, OH, OW] over gy's [B][tH][tW] tile grid.
// Filled by wino_bwdw_args.
struct WinoBwdwArgs {
  const float* gy;
  const float* x;
  float* slab;
  int B, Ci, H, W, Co, OH, OW, tH, tW, pad;
  int t_per;           // tile range of one grid.z slice
  FastDiv d_thw, d_tw;
  int nx, ny, nz;      // grid: Co / 32, Ci / 32, tile slices
};

// ---- fused backward-weight --------------------------------------------
// Twin of wino_fused_kernel with the TILE axis as the reduction: block owns
// a (32co x 32ci) patch of gw across all 16 frequencies, K-loop over tiles
// staging (A gy A^T) and (B^T x B) patches transformed in-register, epilogue
// applies G^T dU G.  grid.z slices the tile range; slices write per-split
// slabs (non-atomic) reduced by slab_reduce (the 2.3M-atomicAdd alternative
// re-creates the split-K atomic pathology measured in round 2).
// As wino_fused_body: (bx, by, bz) is the virtual block index, Gl
// [co][tloc][f] and Xl [ci][tloc][f] the caller's LDS operand arrays.
__device__ __forceinline__ void wino_bwdw_fused_body(
    float (&Gl)[WF_OP], float (&Xl)[WF_OP], unsigned bx, unsigned by, unsigned bz,
    const WinoBwdwArgs& p) {
  const float* __restrict__ gy = p.gy;
  const float* __restrict__ x = p.x;
  const int Ci = p.Ci, H = p.H, W = p.W, Co = p.Co, OH = p.OH, OW = p.OW;
  const int T = p.B * p.tH * p.tW;
  const int ci0 = by * 32;
  const int co0 = bx * 32;
  const int t_begin = bz * p.t_per;
  const int t_end = min(T, t_begin + p.t_per);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wco = (wid >> 1) * 16;
  const int wci = (wid & 1) * 16;
  const int frag_r = lane >> 4;
  const int frag_c = lane & 15;

  f32x4 acc[16];
  #pragma unroll
  for (int f = 0; f < 16; ++f) acc[f] = f32x4{};

  // staging: thread -> (channel = tid>>3, tloc = tid&7) for BOTH sides
  const int s_ch = tid >> 3;          // 0..31
  const int s_t = tid & 7;            // 0..7

  float gg[2][2];     // gy 2x2 tile (for co0 + s_ch)
  float xd[4][4];     // x 4x4 patch (for ci0 + s_ch)

  auto load_regs = [&](int t0) {
    const int t = t0 + s_t;
    const int tc = t < T ? t : T - 1;
    const bool tv = t < t_end;
    const WinoTile tl = wino_tile((unsigned)tc, p.d_thw, p.d_tw);
    const float* gp = gy + ((long)tl.b * Co + co0 + s_ch) * OH * OW
                      + (long)tl.th * 2 * OW + tl.tw * 2;
    gg[0][0] = tv ? gp[0] : 0.f;
    gg[0][1] = tv ? gp[1] : 0.f;
    gg[1][0] = tv ? gp[OW] : 0.f;
    gg[1][1] = tv ? gp[OW + 1] : 0.f;
    wino_load_patch(xd, x + ((long)tl.b * Ci + ci0 + s_ch) * H * W,
                    (int)tl.th * 2 - p.pad, (int)tl.tw * 2 - p.pad, H, W, tv);
  };

  auto store_stage = [&]() {
    f32x4* gp4 = reinterpret_cast<f32x4*>(&Gl[s_ch * WF_RS + s_t * WF_KS]);
    f32x4* xp4 = reinterpret_cast<f32x4*>(&Xl[s_ch * WF_RS + s_t * WF_KS]);
    #pragma unroll
    for (int a = 0; a < 4; ++a)
      gp4[a] = wino_AgAt_row(a, gg[0][0], gg[0][1], gg[1][0], gg[1][1]);
    float u[4][4];
    wino_Bt_d(u, xd);
    #pragma unroll
    for (int a = 0; a < 4; ++a) xp4[a] = wino_BtdB_row(u, a);
  };

  const float* pa = &Gl[(wco + frag_c) * WF_RS + frag_r * WF_KS];
  const float* pb = &Xl[(wci + frag_c) * WF_RS + frag_r * WF_KS];

  load_regs(t_begin);
  for (int t0 = t_begin; t0 < t_end; t0 += 8) {
    store_stage();
    __syncthreads();
    if (t0 + 8 < t_end) load_regs(t0 + 8);
    wino_kstep_mfma(pa, pb, acc);
    __syncthreads();
  }

  // epilogue: lane holds per freq rows co = wco + frag_r*4 + i, col ci =
  // wci + frag_c; gw = G^T dU G per (co, ci), written to this slice's slab
  const long numel = (long)Co * Ci * 9;
  #pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int co = co0 + wco + frag_r * 4 + i;
    const int ci = ci0 + wci + frag_c;
    if (co >= Co || ci >= Ci) continue;
    float u[4][4];
    #pragma unroll
    for (int f = 0; f < 16; ++f) u[f >> 2][f & 3] = acc[f][i];
    float g[3][3];
    wino_GtuG(g, u);
    float* gp = p.slab + (long)bz * numel + ((long)co * Ci + ci) * 9;
    #pragma unroll
    for (int k = 0; k < 9; ++k) gp[k] = g[k / 3][k % 3];
  }
}

__global__ __launch_bounds__(256, 2) void wino_bwdw_fused_kernel(
    WinoBwdwArgs p) {
  __shared__ __attribute__((aligned(16))) float Gl[WF_OP];   // [co][tloc][f]
  __shared__ __attribute__((aligned(16))) float Xl[WF_OP];   // [ci][tloc][f]
  wino_bwdw_fused_body(Gl, Xl, blockIdx.x, blockIdx.y, blockIdx.z, p);
}

// ---- bwd-data + bwd-weight of one layer in ONE launch -------------------
// The two are independent given gy, and each alone is sized to about one
// block per CU of a kernel built for three (profiles/SUMMARY.md round 4: MFMA
// busy 0.24, waves parked 65-75 % of their life).  As one grid both roles'
// blocks are resident together and one role's stalls sit under the other's
// MFMAs.  Each block runs the body of the standalone kernel it replaces over
// the same virtual (bx, by, bz) and the same argument struct — same code, same
// bits — and the two LDS operand arrays are declared once, so LDS stays
// 43 008 B and three blocks still fit a CU.
//
// Block -> (role, linear index within the role): segregated puts the n_data
// bwd-data blocks first and the bwd-weight blocks behind them (as
// wino_wt_in_kernel does); interleaved alternates the roles by block index
// while both last and gives the longer role the remainder.  Within a role the
// linear index decodes x-fastest, the order of the standalone kernel's 3-D
// grid.
// The default is segregated (measured, tools/conv_bwd_pair_bench.py, the
// flagship's nine layers at B=32: 410 vs 422 us/step; interleaved gains 0.5 us
// at the 16x16 layers and loses 7 us at 64ch 32x32, 1.5 us at 256ch 8x8 and
// 512ch 4x4; separate launches: 526).
constexpr int WINO_PAIR_INTERLEAVE = 0;

// d: wino_fused_kernel<true>'s arguments, g: wino_bwdw_fused_kernel's
__global__ __launch_bounds__(256, 3) void wino_bwd_pair_kernel(
    WinoFusedArgs d, WinoBwdwArgs g, int interleave) {
  __shared__ __attribute__((aligned(16))) float Al[WF_OP];
  __shared__ __attribute__((aligned(16))) float Bl[WF_OP];
  // wave-uniform: everything below depends on blockIdx and arguments only
  const int b = blockIdx.x;
  const int dn = d.nx * d.ny * d.nz, gn = g.nx * g.ny * g.nz;
  bool data;
  int idx;
  if (interleave) {
    const int m = min(dn, gn);
    if (b < 2 * m) {
      data = (b & 1) == 0;
      idx = b >> 1;
    } else {
      data = dn > gn;
      idx = b - m;
    }
  } else {
    data = b < dn;
    idx = data ? b : b - dn;
  }
  const int nx = data ? d.nx : g.nx;
  const int plane = nx * (data ? d.ny : g.ny);
  const int bz = idx / plane;
  const int r = idx - bz * plane;
  const int by = r / nx;
  const int bx = r - by * nx;
  if (data) wino_fused_body<true>(Al, Bl, bx, by, bz, d);
  else wino_bwdw_fused_body(Al, Bl, bx, by, bz, g);
}

// Grid-filling splits of the two fused kernels, computed where their argument
// structs are filled, so the slab shapes of the standalone entries and of the
// pair cannot drift apart (profiles/SUMMARY.md round 2 item 5 was such a
// drift).  per: the reduction range of one grid.z slice.
struct WinoSplit { int splits, per; };

// wino_fused_kernel: ci-split so the grid reaches ~1 block/CU (output
// transform is linear in M: slices store partial y tiles into per-slice
// slabs; slice count keeps ci chunks at multiples of the CK=8 step).  Co, Ci:
// the kernel's output and reduction channels (swapped for bwd-data).
static WinoSplit wino_fused_split(int Co, int Ci, int T) {
  const long base_blocks = (long)(T / 32) * (Co / 32);
  int splits = 1;
  if (base_blocks < 256) {
    splits = (int)((256 + base_blocks - 1) / base_blocks);
    const int max_splits = Ci / WF_CK;
    if (splits > max_splits) splits = max_splits;
  }
  const int ci_per = ((Ci / splits + WF_CK - 1) / WF_CK) * WF_CK;
  splits = (Ci + ci_per - 1) / ci_per;
  return {splits, ci_per};
}

// wino_bwdw_fused_kernel: the same over tiles, in steps of 8
static WinoSplit wino_bwdw_split(int Co, int Ci, int T) {
  const long base_blocks = (long)(Co / 32) * (Ci / 32);
  int splits = 1;
  if (base_blocks < 256) {
    splits = (int)((256 + base_blocks - 1) / base_blocks);
    const int max_splits = (T + 7) / 8;
    if (splits > max_splits) splits = max_splits;
  }
  int t_per = ((T / splits + 7) / 8) * 8;
  if (t_per < 8) t_per = 8;
  splits = (T + t_per - 1) / t_per;
  return {splits, t_per};
}

// Geometry, split and grid of wino_fused_kernel for a conv of [B, Ci, H, W]
// into Co channels at padding `pad`, in the KERNEL's roles; CW = w.size(1).
// The pointers are the caller's to fill.  Shape requirements: Co % 32 == 0,
// T % 32 == 0, Ci % 8 == 0.  who: the public entry, for the error text.
static WinoFusedArgs wino_fused_args(int B, int Ci, int H, int W, int Co,
                                     int pad, int CW, const char* who) {
  WinoFusedArgs a{};
  a.B = B; a.Ci = Ci; a.H = H; a.W = W; a.Co = Co; a.pad = pad; a.CW = CW;
  a.OH = H + 2 * pad - 2;
  a.OW = W + 2 * pad - 2;
  const WinoTiles g = wino_tiles(B, a.OH, a.OW);
  TORCH_CHECK(Co % 32 == 0 && g.T % 32 == 0 && Ci % 8 == 0 && a.OH % 2 == 0 &&
              a.OW % 2 == 0 && g.T > 0, who, " shape requirements");
  a.tH = g.tH; a.tW = g.tW; a.d_thw = g.d_thw; a.d_tw = g.d_tw;
  const WinoSplit sp = wino_fused_split(Co, Ci, g.T);
  a.ci_per = sp.per;
  a.nx = g.T / 32; a.ny = Co / 32; a.nz = sp.splits;
  return a;
}

// the bwd-data conv of the layer x [B, Ci, H, W] -> [B, Co, OH, OW] as
// wino_fused_kernel<true> sees it: gy's Co channels at OH x OW into Ci
// channels at H x W with padding 2 - pad; w stays [Co, Ci, 3, 3]
static WinoFusedArgs wino_bwd_data_args(int B, int Ci, int H, int W, int Co,
                                        int pad, const char* who) {
  return wino_fused_args(B, Co, H + 2 * pad - 2, W + 2 * pad - 2, Ci, 2 - pad,
                         Ci, who);
}

// the same for wino_bwdw_fused_kernel and the layer x [B, Ci, H, W] ->
// [B, Co, OH, OW].  Shape requirements: Co % 32 == 0, Ci % 32 == 0.
static WinoBwdwArgs wino_bwdw_args(int B, int Ci, int H, int W, int Co, int pad,
                                   const char* who) {
  WinoBwdwArgs a{};
  a.B = B; a.Ci = Ci; a.H = H; a.W = W; a.Co = Co; a.pad = pad;
  a.OH = H + 2 * pad - 2;
  a.OW = W + 2 * pad - 2;
  TORCH_CHECK(a.OH % 2 == 0 && a.OW % 2 == 0 && Co % 32 == 0 && Ci % 32 == 0 &&
              Co > 0 && Ci > 0, who, " shape requirements");
  const WinoTiles g = wino_tiles(B, a.OH, a.OW);
  a.tH = g.tH; a.tW = g.tW; a.d_thw = g.d_thw; a.d_tw = g.d_tw;
  const WinoSplit sp = wino_bwdw_split(Co, Ci, g.T);
  a.t_per = sp.per;
  a.nx = Co / 32; a.ny = Ci / 32; a.nz = sp.splits;
  return a;
}

at::Tensor conv2d_wino_bwdw_fused(const at::Tensor& gy, const at::Tensor& x,
                                  int pad) {
  TORCH_CHECK(gy.is_cuda() && x.is_cuda() && gy.dim() == 4 && x.dim() == 4);
  auto gyc = gy.contiguous();
  auto xc = x.contiguous();
  const int Co = gy.size(1), Ci = x.size(1);
  WinoBwdwArgs a = wino_bwdw_args(x.size(0), Ci, x.size(2), x.size(3), Co, pad,
                                  "wino_bwdw_fused");
  TORCH_CHECK(gy.size(2) == a.OH && gy.size(3) == a.OW,
              "wino_bwdw_fused geometry");
  auto stream = c10::hip::getCurrentHIPStream().stream();

  auto slab = at::empty({a.nz, Co, Ci, 3, 3}, x.options());
  a.gy = gyc.data_ptr<float>();
  a.x = xc.data_ptr<float>();
  a.slab = slab.data_ptr<float>();
  hipLaunchKernelGGL(wino_bwdw_fused_kernel, dim3(a.nx, a.ny, a.nz), dim3(256),
                     0, stream, a);
  if (a.nz == 1) {
    return slab.view({Co, Ci, 3, 3});
  }
  auto gw = at::empty({Co, Ci, 3, 3}, x.options());
  slab_reduce(slab.data_ptr<float>(), a.nz, gw.data_ptr<float>(), gw.numel(),
              stream);
  return gw;
}

// fully-fused variant: transforms in-kernel, no V/M round trip.  Shape
// requirements: Co % 32 == 0, T % 32 == 0, Ci % 8 == 0.
at::Tensor conv2d_wino_fused(const at::Tensor& x, const at::Tensor& w,
                             c10::optional<at::Tensor> bias, int pad,
                             bool flip) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && x.scalar_type() == at::kFloat);
  TORCH_CHECK(w.size(2) == 3 && w.size(3) == 3, "wino_fused: 3x3 only");
  auto xc = x.contiguous();
  auto wc = w.contiguous();
  const int B = x.size(0);
  const int Co = flip ? w.size(1) : w.size(0);
  const int Ci = flip ? w.size(0) : w.size(1);
  TORCH_CHECK(x.size(1) == Ci, "wino_fused: channel mismatch");
  // the weight transform runs IN-KERNEL (one (co,ci) pair per thread per
  // staging step) — no wt launch, no 16*Co*Ci frequency tensor
  WinoFusedArgs a = wino_fused_args(B, Ci, x.size(2), x.size(3), Co, pad,
                                    (int)w.size(1), "wino_fused");
  auto stream = c10::hip::getCurrentHIPStream().stream();

  // every slice covers a non-empty ci range and T, Co are tile multiples, so
  // each slab is written in full
  auto y = at::empty({B, Co, a.OH, a.OW}, x.options());
  at::Tensor slab;
  if (a.nz > 1) slab = at::empty({a.nz, B, Co, a.OH, a.OW}, x.options());
  a.x = xc.data_ptr<float>();
  a.w = wc.data_ptr<float>();
  a.bias = bias.has_value() ? bias->data_ptr<float>() : nullptr;
  a.y = a.nz > 1 ? slab.data_ptr<float>() : y.data_ptr<float>();
  wino_dispatch_flip(flip, [&](auto F) {
    hipLaunchKernelGGL(wino_fused_kernel<decltype(F)::value>,
                       dim3(a.nx, a.ny, a.nz), dim3(256), 0, stream, a);
  });
  if (a.nz > 1) {
    slab_reduce(slab.data_ptr<float>(), a.nz, y.data_ptr<float>(), y.numel(),
                stream);
  }
  return y;
}

// (bwd-data ci slices, ci per slice, bwd-weight tile slices, tiles per slice)
// of the layer x [B, Ci, H, W] -> [B, Co, OH, OW]: what
// conv2d_wino_fused(flip) and conv2d_wino_bwdw_fused use, alone or paired
std::tuple<int, int, int, int> conv2d_bwd_pair_splits(int B, int Ci, int H,
                                                      int W, int Co, int pad) {
  const WinoFusedArgs d = wino_bwd_data_args(B, Ci, H, W, Co, pad,
                                             "bwd_pair_splits");
  const WinoBwdwArgs g = wino_bwdw_args(B, Ci, H, W, Co, pad, "bwd_pair_splits");
  return {d.nz, d.ci_per, g.nz, g.t_per};
}

// gx and gw of a 3x3 stride-1 layer from one wino_bwd_pair_kernel launch
// (plus one reduce launch when either side is split): what
// conv2d_wino_fused(gy, w, none, 2 - pad, flip) and
// conv2d_wino_bwdw_fused(gy, x, pad) return, bit for bit.  interleave: the
// block assignment (see the kernel); < 0 takes the default.
std::tuple<at::Tensor, at::Tensor> conv2d_bwd_pair(const at::Tensor& gy,
                                                   const at::Tensor& x,
                                                   const at::Tensor& w, int pad,
                                                   int interleave) {
  TORCH_CHECK(gy.is_cuda() && x.is_cuda() && w.is_cuda() && gy.dim() == 4 &&
              x.dim() == 4 && w.dim() == 4 && gy.scalar_type() == at::kFloat);
  TORCH_CHECK(w.size(2) == 3 && w.size(3) == 3, "bwd_pair: 3x3 only");
  auto gyc = gy.contiguous();
  auto xc = x.contiguous();
  auto wc = w.contiguous();
  const int B = x.size(0), Ci = x.size(1), H = x.size(2), W = x.size(3);
  const int Co = gy.size(1), OH = gy.size(2), OW = gy.size(3);
  TORCH_CHECK(gy.size(0) == B && w.size(0) == Co && w.size(1) == Ci &&
              OH == H + 2 * pad - 2 && OW == W + 2 * pad - 2 && pad <= 2,
              "bwd_pair geometry");
  WinoFusedArgs d = wino_bwd_data_args(B, Ci, H, W, Co, pad, "bwd_pair");
  WinoBwdwArgs g = wino_bwdw_args(B, Ci, H, W, Co, pad, "bwd_pair");
  auto stream = c10::hip::getCurrentHIPStream().stream();

  auto gx = at::empty({B, Ci, H, W}, x.options());
  at::Tensor gx_slab;
  if (d.nz > 1) gx_slab = at::empty({d.nz, B, Ci, H, W}, x.options());
  auto gw_slab = at::empty({g.nz, Co, Ci, 3, 3}, x.options());

  d.x = gyc.data_ptr<float>();
  d.w = wc.data_ptr<float>();
  d.y = d.nz > 1 ? gx_slab.data_ptr<float>() : gx.data_ptr<float>();
  g.gy = gyc.data_ptr<float>();
  g.x = xc.data_ptr<float>();
  g.slab = gw_slab.data_ptr<float>();
  if (interleave < 0) interleave = WINO_PAIR_INTERLEAVE;
  hipLaunchKernelGGL(wino_bwd_pair_kernel,
                     dim3(d.nx * d.ny * d.nz + g.nx * g.ny * g.nz), dim3(256),
                     0, stream, d, g, interleave);

  at::Tensor gw = g.nz > 1 ? at::empty({Co, Ci, 3, 3}, x.options())
                           : gw_slab.view({Co, Ci, 3, 3});
  if (d.nz > 1 || g.nz > 1) {
    // a side with one slice was written in place: no job for it
    slab_reduce_pair(d.nz > 1 ? gx_slab.data_ptr<float>() : nullptr, d.nz,
                     gx.data_ptr<float>(), d.nz > 1 ? gx.numel() : 0,
                     g.nz > 1 ? gw_slab.data_ptr<float>() : nullptr, g.nz,
                     gw.data_ptr<float>(), g.nz > 1 ? gw.numel() : 0, stream);
  }
  return {gx, gw};
}

}  // namespace slk
