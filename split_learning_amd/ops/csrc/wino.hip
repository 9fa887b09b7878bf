// Winograd F(2x2, 3x3) convolution for stride-1 3x3 convs (fp32).
// Op sites replaced: every 3x3 s1 Conv2d of the partitioned model zoo
// (reference src/model/VGG16_CIFAR10.py:10-94,
// other/Vanilla_SL/src/model/MobileNetv1_CIFAR10.py:23-167).
//
// y = A^T [ (G g G^T) .* (B^T d B) ] A   per 2x2 output tile (4x4 input
// patch, overlap 2).  2.25x fewer MACs than direct: the elementwise product
// becomes 16 frequency-batched GEMMs  M[f] = U[f][Co,Ci] @ V[f][Ci,T]
// (T = B * OH/2 * OW/2) which run on the existing MFMA tile framework as ONE
// batched launch.  Unfused (transforms round-trip V/M through HBM; the GEMM's
// split-K slabs are summed by the output transform), so it
// wins where the GEMM is compute-dominated — the high-Ci tail of VGG16 —
// and loses to the direct implicit-GEMM kernel on the big-spatial low-Ci
// layers where the 4x data inflation of V/M eats the MAC savings
// (measured routing in conv_route.h; MIOpen's advantage on those layers is a
// FUSED Winograd with in-kernel transforms).
//
// Backward-data reuses the whole machinery: gx = winograd-conv of gy with
// the 180-degree-rotated, Co/Ci-transposed weights at pad' = KH-1-p.
// Backward-weight has its own frequency form (dU[f] = (A gy A^T)[f] @
// V_x[f]^T, gw = G^T dU G) in both a transform+GEMM pipeline and a fully
// FUSED kernel (wino_bwdw_fused_kernel).  The fully fused forward
// (wino_fused_kernel) keeps the transforms in-kernel; routing between the
// three forms is measured per shape (conv_route.h).
#include <tuple>

#include "torch_util.h"

namespace slk {

// weight transform U[f] = (G g G^T)[f] over the weight's true dims
// (Cw0, Cw1) = (w.size(0), w.size(1)); FLIP writes U[f][Cw1][Cw0] with the
// taps rotated 180 degrees (the bwd-data weight), else U[f][Cw0][Cw1].
// (block, nblocks): the launch's blocks that work on this transform — the
// whole grid of wino_wt_kernel, a share of wino_wt_in_kernel's
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
    // row a of G g (G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]])
    float t[3];
    #pragma unroll
    for (int b = 0; b < 3; ++b) {
      const float g0 = w[(((long)co * Cw1 + ci) * 3 + (FLIP ? 2 : 0)) * 3 +
                         (FLIP ? 2 - b : b)];
      const float g1 = w[(((long)co * Cw1 + ci) * 3 + 1) * 3 +
                         (FLIP ? 2 - b : b)];
      const float g2 = w[(((long)co * Cw1 + ci) * 3 + (FLIP ? 0 : 2)) * 3 +
                         (FLIP ? 2 - b : b)];
      t[b] = a == 0 ? g0
           : a == 1 ? 0.5f * (g0 + g1 + g2)
           : a == 2 ? 0.5f * (g0 - g1 + g2)
           : g2;
    }
    U[((long)(a * 4 + 0) * total) + i] = t[0];
    U[((long)(a * 4 + 1) * total) + i] = 0.5f * (t[0] + t[1] + t[2]);
    U[((long)(a * 4 + 2) * total) + i] = 0.5f * (t[0] - t[1] + t[2]);
    U[((long)(a * 4 + 3) * total) + i] = t[2];
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
    const unsigned b = d_thw.div(t);
    const unsigned rem = d_thw.mod(t, b);
    const unsigned th = d_tw.div(rem);
    const unsigned tw = d_tw.mod(rem, th);
    const int ih0 = (int)th * 2 - pad;
    const int iw0 = (int)tw * 2 - pad;
    const float* xp = x + ((long)b * Ci + cc) * H * W;
    float d[4][4];
    #pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int ih = ih0 + a;
      const bool hv = (unsigned)ih < (unsigned)H;
      #pragma unroll
      for (int bb = 0; bb < 4; ++bb) {
        const int iw = iw0 + bb;
        const bool v = hv && (unsigned)iw < (unsigned)W;
        d[a][bb] = v ? xp[(long)ih * W + iw] : 0.f;
      }
    }
    // B^T d: rows [d0-d2, d1+d2, d2-d1, d1-d3]
    float u[4][4];
    #pragma unroll
    for (int bb = 0; bb < 4; ++bb) {
      u[0][bb] = d[0][bb] - d[2][bb];
      u[1][bb] = d[1][bb] + d[2][bb];
      u[2][bb] = d[2][bb] - d[1][bb];
      u[3][bb] = d[1][bb] - d[3][bb];
    }
    #pragma unroll
    for (int a = 0; a < 4; ++a) {
      const float v0 = u[a][0] - u[a][2];
      const float v1 = u[a][1] + u[a][2];
      const float v2 = u[a][2] - u[a][1];
      const float v3 = u[a][1] - u[a][3];
      V[((long)(a * 4 + 0) * Ci + cc) * T + t] = v0;
      V[((long)(a * 4 + 1) * Ci + cc) * T + t] = v1;
      V[((long)(a * 4 + 2) * Ci + cc) * T + t] = v2;
      V[((long)(a * 4 + 3) * Ci + cc) * T + t] = v3;
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

template <bool FLIP>
__global__ void wino_wt_kernel(const float* __restrict__ w,
                               float* __restrict__ U, int Cw0, int Cw1) {
  wino_wt_body<FLIP>(w, U, Cw0, Cw1, blockIdx.x, gridDim.x);
}

// Both operand transforms of conv2d_wino in ONE launch: they are independent
// (U from w, V from x) and each alone underfills or barely fills the chip for
// a few microseconds, so as two launches the second waits out the first's
// drain.  The first in_blocks blocks run the input transform — the short
// one, so its blocks retire while the weight transform's stream in behind
// them — the rest the weight transform; each element is computed by the same
// code as in the separate kernels.
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
// gemm_slab_reduce_kernel's order and form (0.f, then slab 0, 1, ...), so the
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
      // row oi of A^T m: [m0+m1+m2, m1-m2-m3]; then the same across columns
      const int oi = a >> 1, oj = a & 1;
      float u[4];
      #pragma unroll
      for (int bb = 0; bb < 4; ++bb) {
        u[bb] = oi == 0 ? ml[0 + bb][p] + ml[4 + bb][p] + ml[8 + bb][p]
                        : ml[4 + bb][p] - ml[8 + bb][p] - ml[12 + bb][p];
      }
      const float bv = bias != nullptr ? bias[co] : 0.f;
      const unsigned b = d_thw.div(t);
      const unsigned rem = d_thw.mod(t, b);
      const unsigned th = d_tw.div(rem);
      const unsigned tw = d_tw.mod(rem, th);
      float* yp = y + ((long)b * Co + co) * OH * OW + (long)(th * 2 + oi) * OW
                  + tw * 2 + oj;
      *yp = oj == 0 ? u[0] + u[1] + u[2] + bv : u[1] - u[2] - u[3] + bv;
    }
    __syncthreads();
  }
}

// ---- backward-weight --------------------------------------------------
// dY arrives per 2x2 output tile; dM = A dY A^T lifts it to the 4x4
// frequency domain (A = [[1,0],[1,1],[1,-1],[0,-1]]), then
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
    const unsigned b = d_thw.div(t);
    const unsigned rem = d_thw.mod(t, b);
    const unsigned th = d_tw.div(rem);
    const unsigned tw = d_tw.mod(rem, th);
    const float* gp = gy + ((long)b * Co + co) * OH * OW
                      + (long)th * 2 * OW + tw * 2;
    const float g00 = gp[0], g01 = gp[1], g10 = gp[OW], g11 = gp[OW + 1];
    // rows of A gy (4x2): [g0j], [g0j+g1j], [g0j-g1j], [-g1j]
    float r0c0 = g00, r0c1 = g01;
    float r1c0 = g00 + g10, r1c1 = g01 + g11;
    float r2c0 = g00 - g10, r2c1 = g01 - g11;
    float r3c0 = -g10, r3c1 = -g11;
    // columns: dM[a][.] = [c0], [c0+c1], [c0-c1], [-c1]
    #pragma unroll
    for (int a = 0; a < 4; ++a) {
      const float c0 = a == 0 ? r0c0 : a == 1 ? r1c0 : a == 2 ? r2c0 : r3c0;
      const float c1 = a == 0 ? r0c1 : a == 1 ? r1c1 : a == 2 ? r2c1 : r3c1;
      Wg[((long)(a * 4 + 0) * Co + co) * T + t] = c0;
      Wg[((long)(a * 4 + 1) * Co + co) * T + t] = c0 + c1;
      Wg[((long)(a * 4 + 2) * Co + co) * T + t] = c0 - c1;
      Wg[((long)(a * 4 + 3) * Co + co) * T + t] = -c1;
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
    // t = G^T u (3x4), G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]]
    float t[3][4];
    #pragma unroll
    for (int b = 0; b < 4; ++b) {
      t[0][b] = u[0][b] + 0.5f * (u[1][b] + u[2][b]);
      t[1][b] = 0.5f * (u[1][b] - u[2][b]);
      t[2][b] = 0.5f * (u[1][b] + u[2][b]) + u[3][b];
    }
    #pragma unroll
    for (int r = 0; r < 3; ++r) {
      gw[i * 9 + r * 3 + 0] = t[r][0] + 0.5f * (t[r][1] + t[r][2]);
      gw[i * 9 + r * 3 + 1] = 0.5f * (t[r][1] - t[r][2]);
      gw[i * 9 + r * 3 + 2] = 0.5f * (t[r][1] + t[r][2]) + t[r][3];
    }
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

// SLK_WINO_PIPE (A/B and bisection only, read once), default 3: bit 0 = both
// operand transforms in one launch (wino_wt_in_kernel), bit 1 = the output
// transform sums the GEMM's split-K slabs.  0 is the five-launch form: wt, in,
// GEMM, its slab reduce (as matmul_f32 does for every other caller), out.
// Every value gives the same bits.
static int wino_pipe_mode() {
  static int v = [] {
    const char* e = std::getenv("SLK_WINO_PIPE");
    return e ? atoi(e) : 3;
  }();
  return v;
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
  const int tH = OH / 2, tW = OW / 2;
  const int T = B * tH * tW;
  auto stream = c10::hip::getCurrentHIPStream().stream();
  FastDiv d_T, d_thw, d_tw;
  d_T.init(T);
  d_thw.init(tH * tW);
  d_tw.init(tW);

  const int mode = wino_pipe_mode();
  auto U = at::empty({16, Co, Ci}, x.options());
  auto V = at::empty({16, Ci, T}, x.options());
  // weight transform: thread per (pair, freq row), always over the WEIGHT's
  // own dims (FLIP handles the transpose internally); input transform:
  // thread per (ci, tile)
  const int wt_grid =
      (int)std::min<long>(((long)Co * Ci * 4 + 255) / 256, 4096);
  const int in_grid = (int)std::min<long>(((long)Ci * T + 255) / 256, 8192);
  const int Cw0 = (int)w.size(0), Cw1 = (int)w.size(1);
  if (mode & 1) {
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(in_grid + wt_grid), dim3(256), 0,
                         stream, wc.data_ptr<float>(), U.data_ptr<float>(),
                         Cw0, Cw1, xc.data_ptr<float>(), V.data_ptr<float>(),
                         B, Ci, H, W, tH, tW, pad, d_T, d_thw, d_tw, in_grid);
    };
    if (flip) launch(wino_wt_in_kernel<true>);
    else launch(wino_wt_in_kernel<false>);
  } else {
    if (flip) {
      hipLaunchKernelGGL(wino_wt_kernel<true>, dim3(wt_grid), dim3(256), 0,
                         stream, wc.data_ptr<float>(), U.data_ptr<float>(),
                         Cw0, Cw1);
    } else {
      hipLaunchKernelGGL(wino_wt_kernel<false>, dim3(wt_grid), dim3(256), 0,
                         stream, wc.data_ptr<float>(), U.data_ptr<float>(),
                         Cw0, Cw1);
    }
    hipLaunchKernelGGL(wino_in_kernel, dim3(in_grid), dim3(256), 0, stream,
                       xc.data_ptr<float>(), V.data_ptr<float>(), B, Ci, H, W,
                       tH, tW, pad, d_T, d_thw, d_tw);
  }
  // M[f] = U[f] @ V[f]: one batched MFMA GEMM launch (batch = 16); its
  // split-K slabs [splits, 16, Co, T] go to the output transform unreduced
  auto Mm = (mode & 2)
      ? matmul_f32_slabs(U, V)
      : matmul_f32(U, V, false, false, c10::nullopt, false).unsqueeze(0);
  auto y = at::empty({B, Co, OH, OW}, x.options());
  {
    const long blocks = ((long)Co * T + 63) / 64;   // 64 (co, t) pairs each
    const int grid = (int)std::min<long>(blocks, 8192);
    hipLaunchKernelGGL(wino_out_kernel, dim3(grid), dim3(256), 0, stream,
                       Mm.data_ptr<float>(), (int)Mm.size(0), 16l * Co * T,
                       y.data_ptr<float>(),
                       bias.has_value() ? bias->data_ptr<float>() : nullptr,
                       B, Co, OH, OW, tH, tW, d_T, d_thw, d_tw);
  }
  return y;
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
    const float* __restrict__ x, const float* __restrict__ w,
    const float* __restrict__ bias, float* __restrict__ y, int B, int Ci,
    int H, int W, int Co, int OH, int OW, int tH, int tW, int pad,
    int ci_per, int CW, const FastDiv& d_thw, const FastDiv& d_tw) {
  const int ci_begin = bz * ci_per;
  const int ci_end = min(Ci, ci_begin + ci_per);
  // Ul [co][ci][f], Vl [t][ci][f]

  const int T = B * tH * tW;
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
  const int tg = t0 + v_t;
  const unsigned vb = d_thw.div((unsigned)tg);
  const unsigned vrem = d_thw.mod((unsigned)tg, vb);
  const unsigned vth = d_tw.div(vrem);
  const unsigned vtw = d_tw.mod(vrem, vth);
  const int ih0 = (int)vth * 2 - pad;
  const int iw0 = (int)vtw * 2 - pad;
  const long xplane = ((long)vb * Ci + v_ci) * H * W;
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
    const float* xp = x + xplane + (long)ci0 * H * W;
    #pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int ih = ih0 + a;
      const bool hv = (unsigned)ih < (unsigned)H;
      #pragma unroll
      for (int bb = 0; bb < 4; ++bb) {
        const int iw = iw0 + bb;
        const bool v = hv && (unsigned)iw < (unsigned)W;
        d[a][bb] = v ? xp[(long)ih * W + iw] : 0.f;
      }
    }
    const long wbase = FLIP
        ? ((long)(ci0 + w_ci) * CW + (co0 + w_co)) * 9
        : ((long)(co0 + w_co) * CW + (ci0 + w_ci)) * 9;
    using f32x4u = __attribute__((ext_vector_type(4), aligned(4))) float;
    wq0 = *reinterpret_cast<const f32x4u*>(w + wbase);
    wq1 = *reinterpret_cast<const f32x4u*>(w + wbase + 4);
    w8 = w[wbase + 8];
  };

  auto store_stage = [&]() {
    float u[4][4];
    #pragma unroll
    for (int bb = 0; bb < 4; ++bb) {
      u[0][bb] = d[0][bb] - d[2][bb];
      u[1][bb] = d[1][bb] + d[2][bb];
      u[2][bb] = d[2][bb] - d[1][bb];
      u[3][bb] = d[1][bb] - d[3][bb];
    }
    f32x4* vp = reinterpret_cast<f32x4*>(&Vl[v_t * WF_RS + v_ci * WF_KS]);
    #pragma unroll
    for (int a = 0; a < 4; ++a) {
      vp[a] = f32x4{u[a][0] - u[a][2], u[a][1] + u[a][2],
                    u[a][2] - u[a][1], u[a][1] - u[a][3]};
    }
    // U = G w G^T for this thread's (co, ci) pair — same op order as
    // wino_wt_kernel, so the result is bit-identical to the staged path
    const float raw[9] = {wq0[0], wq0[1], wq0[2], wq0[3], wq1[0],
                          wq1[1], wq1[2], wq1[3], w8};
    float wr[9];
    #pragma unroll
    for (int k = 0; k < 9; ++k) wr[k] = raw[FLIP ? 8 - k : k];
    float t0[3], t1[3], t2[3], t3[3];
    #pragma unroll
    for (int bb = 0; bb < 3; ++bb) {
      const float g0 = wr[bb], g1 = wr[3 + bb], g2 = wr[6 + bb];
      t0[bb] = g0;
      t1[bb] = 0.5f * (g0 + g1 + g2);
      t2[bb] = 0.5f * (g0 - g1 + g2);
      t3[bb] = g2;
    }
    const float* tr[4] = {t0, t1, t2, t3};
    f32x4* up = reinterpret_cast<f32x4*>(&Ul[w_co * WF_RS + w_ci * WF_KS]);
    #pragma unroll
    for (int a = 0; a < 4; ++a) {
      const float* t = tr[a];
      up[a] = f32x4{t[0], 0.5f * (t[0] + t[1] + t[2]),
                    0.5f * (t[0] - t[1] + t[2]), t[2]};
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
    float u0[4], u1[4];
    #pragma unroll
    for (int bb = 0; bb < 4; ++bb) {
      u0[bb] = m[0][bb] + m[1][bb] + m[2][bb];
      u1[bb] = m[1][bb] - m[2][bb] - m[3][bb];
    }
    const float bv = (bias != nullptr && bz == 0) ? bias[co] : 0.f;
    const unsigned b = d_thw.div((unsigned)t);
    const unsigned rem = d_thw.mod((unsigned)t, b);
    const unsigned th = d_tw.div(rem);
    const unsigned tw = d_tw.mod(rem, th);
    float* yp = y + (long)bz * B * Co * OH * OW +
                ((long)b * Co + co) * OH * OW + (long)th * 2 * OW + tw * 2;
    const float o00 = u0[0] + u0[1] + u0[2] + bv;
    const float o01 = u0[1] - u0[2] - u0[3] + bv;
    const float o10 = u1[0] + u1[1] + u1[2] + bv;
    const float o11 = u1[1] - u1[2] - u1[3] + bv;
    yp[0] = o00;
    yp[1] = o01;
    yp[OW] = o10;
    yp[OW + 1] = o11;
  }
}

template <bool FLIP>
__global__ __launch_bounds__(256, 3) void wino_fused_kernel(
    const float* __restrict__ x, const float* __restrict__ w,
    const float* __restrict__ bias, float* __restrict__ y, int B, int Ci,
    int H, int W, int Co, int OH, int OW, int tH, int tW, int pad,
    int ci_per, int CW, FastDiv d_thw, FastDiv d_tw) {
  // single-buffer two-barrier loop: double buffering would cost 84 KB of
  // LDS (1 block/CU); at 42 KB three blocks fit, which is what the
  // launch bound allows anyway
  __shared__ __attribute__((aligned(16))) float Ul[WF_OP];   // [co][ci][f]
  __shared__ __attribute__((aligned(16))) float Vl[WF_OP];   // [t][ci][f]
  wino_fused_body<FLIP>(Ul, Vl, blockIdx.x, blockIdx.y, blockIdx.z, x, w, bias,
                        y, B, Ci, H, W, Co, OH, OW, tH, tW, pad, ci_per, CW,
                        d_thw, d_tw);
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
  const int tH = OH / 2, tW = OW / 2;
  const int T = B * tH * tW;
  auto stream = c10::hip::getCurrentHIPStream().stream();
  FastDiv d_T, d_thw, d_tw;
  d_T.init(T);
  d_thw.init(tH * tW);
  d_tw.init(tW);

  auto Wg = at::empty({16, Co, T}, x.options());
  auto Vx = at::empty({16, Ci, T}, x.options());
  {
    const long tot = (long)Co * T;
    const int grid = (int)std::min<long>((tot + 255) / 256, 8192);
    hipLaunchKernelGGL(wino_gyA_kernel, dim3(grid), dim3(256), 0, stream,
                       gyc.data_ptr<float>(), Wg.data_ptr<float>(), B, Co, OH,
                       OW, tH, tW, d_T, d_thw, d_tw);
  }
  {
    const long tot = (long)Ci * T;
    const int grid = (int)std::min<long>((tot + 255) / 256, 8192);
    hipLaunchKernelGGL(wino_in_kernel, dim3(grid), dim3(256), 0, stream,
                       xc.data_ptr<float>(), Vx.data_ptr<float>(), B, Ci, H, W,
                       tH, tW, pad, d_T, d_thw, d_tw);
  }
  // dU[f][Co][Ci] = Wg[f] @ Vx[f]^T : 16 frequency GEMMs, K = tiles
  auto dU = matmul_f32(Wg, Vx, false, true, c10::nullopt, false);
  auto gw = at::empty({Co, Ci, 3, 3}, x.options());
  {
    const long tot = (long)Co * Ci;
    const int grid = (int)std::min<long>((tot + 255) / 256, 4096);
    hipLaunchKernelGGL(wino_gw_kernel, dim3(grid), dim3(256), 0, stream,
                       dU.data_ptr<float>(), gw.data_ptr<float>(), Co, Ci);
  }
  return gw;
}

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
    const float* __restrict__ gy, const float* __restrict__ x,
    float* __restrict__ slab, int B, int Ci, int H, int W, int Co, int OH,
    int OW, int tH, int tW, int pad, int t_per, const FastDiv& d_thw,
    const FastDiv& d_tw) {
  const int T = B * tH * tW;
  const int ci0 = by * 32;
  const int co0 = bx * 32;
  const int t_begin = bz * t_per;
  const int t_end = min(T, t_begin + t_per);

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
    const unsigned b = d_thw.div((unsigned)tc);
    const unsigned rem = d_thw.mod((unsigned)tc, b);
    const unsigned th = d_tw.div(rem);
    const unsigned tw = d_tw.mod(rem, th);
    {
      const float* gp = gy + ((long)b * Co + co0 + s_ch) * OH * OW
                        + (long)th * 2 * OW + tw * 2;
      gg[0][0] = tv ? gp[0] : 0.f;
      gg[0][1] = tv ? gp[1] : 0.f;
      gg[1][0] = tv ? gp[OW] : 0.f;
      gg[1][1] = tv ? gp[OW + 1] : 0.f;
    }
    {
      const int ih0 = (int)th * 2 - pad;
      const int iw0 = (int)tw * 2 - pad;
      const float* xp = x + ((long)b * Ci + ci0 + s_ch) * H * W;
      #pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int ih = ih0 + a;
        const bool hv = tv && (unsigned)ih < (unsigned)H;
        #pragma unroll
        for (int bb = 0; bb < 4; ++bb) {
          const int iw = iw0 + bb;
          const bool v = hv && (unsigned)iw < (unsigned)W;
          xd[a][bb] = v ? xp[(long)ih * W + iw] : 0.f;
        }
      }
    }
  };

  auto store_stage = [&]() {
    // dM = A gy A^T (A = [[1,0],[1,1],[1,-1],[0,-1]])
    const float r0c0 = gg[0][0], r0c1 = gg[0][1];
    const float r1c0 = gg[0][0] + gg[1][0], r1c1 = gg[0][1] + gg[1][1];
    const float r2c0 = gg[0][0] - gg[1][0], r2c1 = gg[0][1] - gg[1][1];
    const float r3c0 = -gg[1][0], r3c1 = -gg[1][1];
    f32x4* gp4 = reinterpret_cast<f32x4*>(&Gl[s_ch * WF_RS + s_t * WF_KS]);
    f32x4* xp4 = reinterpret_cast<f32x4*>(&Xl[s_ch * WF_RS + s_t * WF_KS]);
    #pragma unroll
    for (int a = 0; a < 4; ++a) {
      const float c0 = a == 0 ? r0c0 : a == 1 ? r1c0 : a == 2 ? r2c0 : r3c0;
      const float c1 = a == 0 ? r0c1 : a == 1 ? r1c1 : a == 2 ? r2c1 : r3c1;
      gp4[a] = f32x4{c0, c0 + c1, c0 - c1, -c1};
    }
    // B^T d B
    float u[4][4];
    #pragma unroll
    for (int bb = 0; bb < 4; ++bb) {
      u[0][bb] = xd[0][bb] - xd[2][bb];
      u[1][bb] = xd[1][bb] + xd[2][bb];
      u[2][bb] = xd[2][bb] - xd[1][bb];
      u[3][bb] = xd[1][bb] - xd[3][bb];
    }
    #pragma unroll
    for (int a = 0; a < 4; ++a) {
      xp4[a] = f32x4{u[a][0] - u[a][2], u[a][1] + u[a][2],
                     u[a][2] - u[a][1], u[a][1] - u[a][3]};
    }
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
    float t3[3][4];
    #pragma unroll
    for (int bb = 0; bb < 4; ++bb) {
      t3[0][bb] = u[0][bb] + 0.5f * (u[1][bb] + u[2][bb]);
      t3[1][bb] = 0.5f * (u[1][bb] - u[2][bb]);
      t3[2][bb] = 0.5f * (u[1][bb] + u[2][bb]) + u[3][bb];
    }
    float* gp = slab + (long)bz * numel + ((long)co * Ci + ci) * 9;
    #pragma unroll
    for (int r = 0; r < 3; ++r) {
      gp[r * 3 + 0] = t3[r][0] + 0.5f * (t3[r][1] + t3[r][2]);
      gp[r * 3 + 1] = 0.5f * (t3[r][1] - t3[r][2]);
      gp[r * 3 + 2] = 0.5f * (t3[r][1] + t3[r][2]) + t3[r][3];
    }
  }
}

__global__ __launch_bounds__(256, 2) void wino_bwdw_fused_kernel(
    const float* __restrict__ gy, const float* __restrict__ x,
    float* __restrict__ slab, int B, int Ci, int H, int W, int Co, int OH,
    int OW, int tH, int tW, int pad, int t_per, FastDiv d_thw, FastDiv d_tw) {
  __shared__ __attribute__((aligned(16))) float Gl[WF_OP];   // [co][tloc][f]
  __shared__ __attribute__((aligned(16))) float Xl[WF_OP];   // [ci][tloc][f]
  wino_bwdw_fused_body(Gl, Xl, blockIdx.x, blockIdx.y, blockIdx.z, gy, x, slab,
                       B, Ci, H, W, Co, OH, OW, tH, tW, pad, t_per, d_thw,
                       d_tw);
}

// ---- bwd-data + bwd-weight of one layer in ONE launch -------------------
// The two are independent given gy, and each alone is sized to about one
// block per CU of a kernel built for three (profiles/SUMMARY.md round 4: MFMA
// busy 0.24, waves parked 65-75 % of their life).  As one grid both roles'
// blocks are resident together and one role's stalls sit under the other's
// MFMAs.  Each block runs the body of the standalone kernel it replaces over
// the same virtual (bx, by, bz) — same code, same bits — and the two LDS
// operand arrays are declared once, so LDS stays 43 008 B and three blocks
// still fit a CU.
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
struct WinoPairData {     // wino_fused_kernel<true>'s arguments
  const float* x; const float* w; float* y;
  int B, Ci, H, W, Co, OH, OW, tH, tW, pad, ci_per, CW;
  FastDiv d_thw, d_tw;
  int gx, gy, n;          // grid.x, grid.y, blocks
};
struct WinoPairWeight {   // wino_bwdw_fused_kernel's arguments
  const float* gy; const float* x; float* slab;
  int B, Ci, H, W, Co, OH, OW, tH, tW, pad, t_per;
  FastDiv d_thw, d_tw;
  int gx, gy_, n;
};

__global__ __launch_bounds__(256, 3) void wino_bwd_pair_kernel(
    WinoPairData d, WinoPairWeight g, int interleave) {
  __shared__ __attribute__((aligned(16))) float Al[WF_OP];
  __shared__ __attribute__((aligned(16))) float Bl[WF_OP];
  // wave-uniform: everything below depends on blockIdx and arguments only
  const int b = blockIdx.x;
  bool data;
  int idx;
  if (interleave) {
    const int m = min(d.n, g.n);
    if (b < 2 * m) {
      data = (b & 1) == 0;
      idx = b >> 1;
    } else {
      data = d.n > g.n;
      idx = b - m;
    }
  } else {
    data = b < d.n;
    idx = data ? b : b - d.n;
  }
  if (data) {
    const int plane = d.gx * d.gy;
    const int bz = idx / plane;
    const int r = idx - bz * plane;
    const int by = r / d.gx;
    wino_fused_body<true>(Al, Bl, r - by * d.gx, by, bz, d.x, d.w, nullptr,
                          d.y, d.B, d.Ci, d.H, d.W, d.Co, d.OH, d.OW, d.tH,
                          d.tW, d.pad, d.ci_per, d.CW, d.d_thw, d.d_tw);
  } else {
    const int plane = g.gx * g.gy_;
    const int bz = idx / plane;
    const int r = idx - bz * plane;
    const int by = r / g.gx;
    wino_bwdw_fused_body(Al, Bl, r - by * g.gx, by, bz, g.gy, g.x, g.slab,
                         g.B, g.Ci, g.H, g.W, g.Co, g.OH, g.OW, g.tH, g.tW,
                         g.pad, g.t_per, g.d_thw, g.d_tw);
  }
}

// Grid-filling splits of the two fused kernels, shared by their standalone
// host entries and the pair entry so the slab shapes cannot drift apart
// (profiles/SUMMARY.md round 2 item 5 was such a drift).  per: the reduction
// range of one grid.z slice.
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

at::Tensor conv2d_wino_bwdw_fused(const at::Tensor& gy, const at::Tensor& x,
                                  int pad) {
  TORCH_CHECK(gy.is_cuda() && x.is_cuda() && gy.dim() == 4 && x.dim() == 4);
  auto gyc = gy.contiguous();
  auto xc = x.contiguous();
  const int B = x.size(0), Ci = x.size(1), H = x.size(2), W = x.size(3);
  const int Co = gy.size(1), OH = gy.size(2), OW = gy.size(3);
  TORCH_CHECK(OH == H + 2 * pad - 2 && OW == W + 2 * pad - 2,
              "wino_bwdw_fused geometry");
  TORCH_CHECK(OH % 2 == 0 && OW % 2 == 0 && Co % 32 == 0 && Ci % 32 == 0,
              "wino_bwdw_fused shape requirements");
  const int tH = OH / 2, tW = OW / 2;
  const int T = B * tH * tW;
  auto stream = c10::hip::getCurrentHIPStream().stream();

  const WinoSplit sp = wino_bwdw_split(Co, Ci, T);
  const int splits = sp.splits;

  auto slab = at::empty({splits, Co, Ci, 3, 3}, x.options());
  FastDiv d_thw, d_tw;
  d_thw.init(tH * tW);
  d_tw.init(tW);
  dim3 grid(Co / 32, Ci / 32, splits);
  hipLaunchKernelGGL(wino_bwdw_fused_kernel, grid, dim3(256), 0, stream,
                     gyc.data_ptr<float>(), xc.data_ptr<float>(),
                     slab.data_ptr<float>(), B, Ci, H, W, Co, OH, OW, tH, tW,
                     pad, sp.per, d_thw, d_tw);
  if (splits == 1) {
    return slab.view({Co, Ci, 3, 3});
  }
  auto gw = at::empty({Co, Ci, 3, 3}, x.options());
  slab_reduce(slab.data_ptr<float>(), splits, gw.data_ptr<float>(), gw.numel(),
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
  const int B = x.size(0), H = x.size(2), W = x.size(3);
  const int Co = flip ? w.size(1) : w.size(0);
  const int Ci = flip ? w.size(0) : w.size(1);
  TORCH_CHECK(x.size(1) == Ci, "wino_fused: channel mismatch");
  const int OH = H + 2 * pad - 2, OW = W + 2 * pad - 2;
  const int tH = OH / 2, tW = OW / 2;
  const int T = B * tH * tW;
  TORCH_CHECK(Co % 32 == 0 && T % 32 == 0 && Ci % 8 == 0 && OH % 2 == 0
              && OW % 2 == 0, "wino_fused shape requirements");
  auto stream = c10::hip::getCurrentHIPStream().stream();
  // the weight transform runs IN-KERNEL (one (co,ci) pair per thread per
  // staging step) — no wt launch, no 16*Co*Ci frequency tensor
  const int CW = (int)w.size(1);
  const WinoSplit sp = wino_fused_split(Co, Ci, T);
  const int splits = sp.splits, ci_per = sp.per;

  // every slice covers a non-empty ci range and T, Co are tile multiples, so
  // each slab is written in full
  auto y = at::empty({B, Co, OH, OW}, x.options());
  at::Tensor slab;
  if (splits > 1) slab = at::empty({splits, B, Co, OH, OW}, x.options());
  float* yw = splits > 1 ? slab.data_ptr<float>() : y.data_ptr<float>();
  FastDiv d_thw, d_tw;
  d_thw.init(tH * tW);
  d_tw.init(tW);
  dim3 grid(T / 32, Co / 32, splits);
  if (flip) {
    hipLaunchKernelGGL(wino_fused_kernel<true>, grid, dim3(256), 0, stream,
                       xc.data_ptr<float>(), wc.data_ptr<float>(),
                       bias.has_value() ? bias->data_ptr<float>() : nullptr,
                       yw, B, Ci, H, W, Co, OH, OW, tH, tW,
                       pad, ci_per, CW, d_thw, d_tw);
  } else {
    hipLaunchKernelGGL(wino_fused_kernel<false>, grid, dim3(256), 0, stream,
                       xc.data_ptr<float>(), wc.data_ptr<float>(),
                       bias.has_value() ? bias->data_ptr<float>() : nullptr,
                       yw, B, Ci, H, W, Co, OH, OW, tH, tW,
                       pad, ci_per, CW, d_thw, d_tw);
  }
  if (splits > 1) {
    slab_reduce(slab.data_ptr<float>(), splits, y.data_ptr<float>(), y.numel(),
                stream);
  }
  return y;
}

// (bwd-data ci slices, ci per slice, bwd-weight tile slices, tiles per slice)
// of the layer x [B, Ci, H, W] -> [B, Co, OH, OW]: what
// conv2d_wino_fused(flip) and conv2d_wino_bwdw_fused use, alone or paired
std::tuple<int, int, int, int> conv2d_bwd_pair_splits(int B, int Ci, int H,
                                                      int W, int Co, int pad) {
  const int OH = H + 2 * pad - 2, OW = W + 2 * pad - 2;
  const WinoSplit ds = wino_fused_split(Ci, Co, B * (H / 2) * (W / 2));
  const WinoSplit ws = wino_bwdw_split(Co, Ci, B * (OH / 2) * (OW / 2));
  return {ds.splits, ds.per, ws.splits, ws.per};
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
  // bwd-data: a fused conv of gy (Co channels, OH x OW) into Ci channels at
  // H x W with pad 2 - pad; bwd-weight: tiles of gy
  const int dtH = H / 2, dtW = W / 2, dT = B * dtH * dtW;
  const int wtH = OH / 2, wtW = OW / 2, wT = B * wtH * wtW;
  TORCH_CHECK(H % 2 == 0 && W % 2 == 0 && OH % 2 == 0 && OW % 2 == 0 &&
              Ci % 32 == 0 && Co % 32 == 0 && dT % 32 == 0,
              "bwd_pair shape requirements");
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const WinoSplit ds = wino_fused_split(Ci, Co, dT);
  const WinoSplit ws = wino_bwdw_split(Co, Ci, wT);

  auto gx = at::empty({B, Ci, H, W}, x.options());
  at::Tensor gx_slab;
  if (ds.splits > 1) gx_slab = at::empty({ds.splits, B, Ci, H, W}, x.options());
  auto gw_slab = at::empty({ws.splits, Co, Ci, 3, 3}, x.options());

  WinoPairData d;
  d.x = gyc.data_ptr<float>();
  d.w = wc.data_ptr<float>();
  d.y = ds.splits > 1 ? gx_slab.data_ptr<float>() : gx.data_ptr<float>();
  d.B = B; d.Ci = Co; d.H = OH; d.W = OW; d.Co = Ci; d.OH = H; d.OW = W;
  d.tH = dtH; d.tW = dtW; d.pad = 2 - pad; d.ci_per = ds.per; d.CW = Ci;
  d.d_thw.init(dtH * dtW);
  d.d_tw.init(dtW);
  d.gx = dT / 32; d.gy = Ci / 32; d.n = d.gx * d.gy * ds.splits;
  WinoPairWeight g;
  g.gy = gyc.data_ptr<float>();
  g.x = xc.data_ptr<float>();
  g.slab = gw_slab.data_ptr<float>();
  g.B = B; g.Ci = Ci; g.H = H; g.W = W; g.Co = Co; g.OH = OH; g.OW = OW;
  g.tH = wtH; g.tW = wtW; g.pad = pad; g.t_per = ws.per;
  g.d_thw.init(wtH * wtW);
  g.d_tw.init(wtW);
  g.gx = Co / 32; g.gy_ = Ci / 32; g.n = g.gx * g.gy_ * ws.splits;
  if (interleave < 0) interleave = WINO_PAIR_INTERLEAVE;
  hipLaunchKernelGGL(wino_bwd_pair_kernel, dim3(d.n + g.n), dim3(256), 0,
                     stream, d, g, interleave);

  at::Tensor gw = ws.splits > 1 ? at::empty({Co, Ci, 3, 3}, x.options())
                                : gw_slab.view({Co, Ci, 3, 3});
  if (ds.splits > 1 || ws.splits > 1) {
    // a side with one slice was written in place: no job for it
    slab_reduce_pair(ds.splits > 1 ? gx_slab.data_ptr<float>() : nullptr,
                     ds.splits, gx.data_ptr<float>(),
                     ds.splits > 1 ? gx.numel() : 0,
                     ws.splits > 1 ? gw_slab.data_ptr<float>() : nullptr,
                     ws.splits, gw.data_ptr<float>(),
                     ws.splits > 1 ? gw.numel() : 0, stream);
  }
  return {gx, gw};
}

}  // namespace slk
