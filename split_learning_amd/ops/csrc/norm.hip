// BatchNorm2d (train/eval, fwd/bwd) and LayerNorm (fwd/bwd) for fp32 NCHW /
// row-major tensors.  BatchNorm keeps exact torch semantics (biased batch var
// for normalisation, unbiased for running stats — done host-side in
// ops/functional.py) so state_dict running stats stay .pth-compatible
// (SURVEY.md §7 hard-part 2).
#include "torch_util.h"

namespace slk {

// ---------------- BatchNorm2d ----------------

// Per-element expressions shared by every BN kernel below (chunked, one-
// kernel, pooled): one definition each, so the separate-launch and the
// single-launch forms of a layer compute bit-identical values.  Contraction
// is spelled out rather than left to the compiler: where a block holds a
// channel's sums as loop invariants it hoisted sum_gy * inv_n and fused the
// OTHER product instead, a last-bit difference from the per-element kernels
// whenever 1/n is not a power of two.  The explicit forms are the ones the
// per-element kernels (bn_fwd_kernel, bn_bwd_dx_kernel) have always compiled
// to: y = fma(xhat, gamma, beta); dx = gamma*is*(fma(-inv_n, sum_gy, g) -
// xhat*sum_gy_xhat*inv_n).
__device__ __forceinline__ float bn_apply(float xv, float m, float is, float g,
                                          float b, bool relu) {
#pragma clang fp contract(off)
  float v = __builtin_fmaf((xv - m) * is, g, b);
  if (relu) v = slk_relu(v);
  return v;
}

__device__ __forceinline__ float bn_dx(float xv, float g, float m, float is,
                                       float gamma, float sum_gy,
                                       float sum_gy_xhat, float inv_n) {
#pragma clang fp contract(off)
  const float xhat = (xv - m) * is;
  const float t = __builtin_fmaf(-inv_n, sum_gy, g);
  return gamma * is * (t - xhat * sum_gy_xhat * inv_n);
}

// Geometry of the MaxPool2d(2,2) folded behind BN+ReLU (H and W even):
// W is the full-resolution row length, OH x OW the pooled plane.
struct PoolGeom {
  int W, OH, OW;
  FastDiv d_w, d_ow, d_ohow;
};

static inline PoolGeom pool_geom(int H, int W) {
  PoolGeom pg;
  pg.W = W;
  pg.OH = H / 2;
  pg.OW = W / 2;
  pg.d_w.init(W);
  pg.d_ow.init(pg.OW);
  pg.d_ohow.init(pg.OH * pg.OW);
  return pg;
}

// BN+ReLU of the 2x2 window at xp, then maxpool_fwd_kernel's selection rule:
// start from position 0, replace on slk_pool_takes in the order 1, 2, 3.
__device__ __forceinline__ float bn_relu_pool_window(const float* __restrict__ xp,
                                                     int W, float m, float is,
                                                     float g, float b, int& bi) {
  float best = bn_apply(xp[0], m, is, g, b, true);
  bi = 0;
  float v = bn_apply(xp[1], m, is, g, b, true);
  if (slk_pool_takes(v, best)) { best = v; bi = 1; }
  v = bn_apply(xp[W], m, is, g, b, true);
  if (slk_pool_takes(v, best)) { best = v; bi = 2; }
  v = bn_apply(xp[W + 1], m, is, g, b, true);
  if (slk_pool_takes(v, best)) { best = v; bi = 3; }
  return best;
}

// The 2x2 window of pooled output `rem` (= oh*OW + ow) of one (b, c) plane,
// fetched ahead of its use: w is the window as a plane of row length 2, which
// is how bn_relu_pool_window is then called on it; o is where the pooled
// output goes.
struct BnWindow {
  float w[4];
  long o;
};

__device__ __forceinline__ BnWindow bn_window_load(const float* __restrict__ plane,
                                                   unsigned rem, long o,
                                                   const PoolGeom& pg) {
  const unsigned oh = pg.d_ow.div(rem);
  const unsigned ow = pg.d_ow.mod(rem, oh);
  const float* xp = plane + (long)(oh * 2) * pg.W + ow * 2;
  return BnWindow{{xp[0], xp[1], xp[pg.W], xp[pg.W + 1]}, o};
}

// batch depth of the loop that fetches a window (four loads) per iteration
constexpr int BN_POOL_U = 4;

// Gradient arriving at full-resolution element (bc, r), r = h*W + w.
// !POOL: gy/relu_y are full resolution; RELU fuses the ReLU backward mask
// (g = y>0 ? gy : 0).  POOL: gy, relu_y (the pooled output) and idx are at
// pooled resolution — the element gets the pooled gradient iff it was the
// window's argmax and the pooled value passed the ReLU, which is what
// maxpool_bwd followed by the full-resolution mask yields.  The test is
// !(y <= 0) so a NaN behaves as in the full-resolution mask.
// Fetch and selection are apart so that a loop can issue the fetches of
// several elements before the first selection (slk_batched): bn_gy_load reads
// every operand unconditionally (all three addresses are valid for every
// in-range element; a short-circuit here was up to three serial round trips
// per element), bn_gy_select applies the predicates.
struct BnGy {
  float gy, ry;
  uint8_t idx, pos;
};

template <bool POOL, bool RELU>
__device__ __forceinline__ BnGy bn_gy_load(const float* __restrict__ gy,
                                           const float* __restrict__ relu_y,
                                           const uint8_t* __restrict__ idx,
                                           long off, unsigned bc, unsigned r,
                                           const PoolGeom& pg) {
  BnGy v{};
  if (POOL) {
    const unsigned h = pg.d_w.div(r);
    const unsigned w = pg.d_w.mod(r, h);
    const long o = ((long)bc * pg.OH + (h >> 1)) * pg.OW + (w >> 1);
    v.pos = (uint8_t)(((h & 1) << 1) | (w & 1));
    v.idx = idx[o];
    v.ry = relu_y[o];
    v.gy = gy[o];
  } else {
    v.gy = gy[off];
    if (RELU) v.ry = relu_y[off];
  }
  return v;
}

template <bool POOL, bool RELU>
__device__ __forceinline__ float bn_gy_select(const BnGy& v) {
  if (POOL) return (v.idx == v.pos && !(v.ry <= 0.f)) ? v.gy : 0.f;
  if (RELU) return v.ry <= 0.f ? 0.f : v.gy;
  return v.gy;
}

// relu_y == nullptr is uniform over the launch: one branch around a loop, not
// one per element.  f(std::true_type / std::false_type) gets RELU.
template <bool POOL, class F>
__device__ __forceinline__ void bn_relu_dispatch(const float* relu_y, F&& f) {
  if (POOL || relu_y != nullptr) f(std::true_type{});
  else f(std::false_type{});
}

// The short-circuit form of load + select, one element at a time: what
// bn_bwd_dx_kernel, which gained nothing from batching, still uses.
template <bool POOL>
__device__ __forceinline__ float bn_gy_at(const float* __restrict__ gy,
                                          const float* __restrict__ relu_y,
                                          const uint8_t* __restrict__ idx,
                                          long off, unsigned bc, unsigned r,
                                          const PoolGeom& pg) {
  if (POOL) {
    const unsigned h = pg.d_w.div(r);
    const unsigned w = pg.d_w.mod(r, h);
    const long o = ((long)bc * pg.OH + (h >> 1)) * pg.OW + (w >> 1);
    const unsigned pos = ((h & 1) << 1) | (w & 1);
    return (idx[o] == (uint8_t)pos && !(relu_y[o] <= 0.f)) ? gy[o] : 0.f;
  } else {
    float g = gy[off];
    if (relu_y != nullptr && relu_y[off] <= 0.f) g = 0.f;
    return g;
  }
}

// sum(x) and sum(x^2) of channel c over the linear (b, hw) range [lo, hi):
// thread t accumulates lo+t, lo+t+blockDim, ... in double, one s and one s2
// per thread, then the block sum.  Result valid in thread 0.
__device__ __forceinline__ void bn_stat_sums(const float* __restrict__ x, int c,
                                             int lo, int hi, int C, int HW,
                                             const FastDiv& d_hw, double* scratch,
                                             double& ts, double& ts2) {
  double s = 0.0, s2 = 0.0;
  slk_batched<SLK_BN_U, float>(
      lo + (int)threadIdx.x, hi, (int)blockDim.x,
      [&](int i) {
        // FastDiv: the plain i / HW was a ~25-VALU runtime division PER ELEMENT
        const unsigned b = d_hw.div((unsigned)i);
        const unsigned r = d_hw.mod((unsigned)i, b);
        return x[((long)b * C + c) * HW + r];
      },
      [&](int, float xv) {
        // one add, one fma: what `s += v; s2 += v * v` has always compiled to
        const double v = (double)xv;
        s += v;
        s2 = __builtin_fma(v, v, s2);
      });
  ts = slk_block_sum(s, scratch);
  __syncthreads();
  ts2 = slk_block_sum(s2, scratch);
}

// mean / invstd / running-stat update of one channel.  sf, s2f are the sums
// as float (float-cast chunk sums added in float), s, s2 the same sums in
// double.  E[x^2] - E[x]^2 formed from the float sums cancels mean^2/var
// leading digits: a channel with mean 1000 and std 1 lost all but two digits
// of invstd.  The double variance is the yardstick, and taking it always
// would be the simplest finalize.  It is not taken always because it moves
// the statistics of well-conditioned channels by an ulp, one ReLU mask flips
// somewhere in a deep net, and within a few steps a training run no longer
// reproduces its earlier self (VGG16: gradients 2e-2 apart after one step).
// So where the float expression lands within BN_KEEP_FLOAT of the double
// variance, its mean and variance are kept bit for bit; beyond that the
// double results, rounded once, replace both.  2^-19 is the smallest power of
// two at which 544 steps of the VGG16 benchmark keep every bit (2^-20 does
// not).  What this costs: a kept invstd may be up to 2^-20 (1e-6) relative
// off, about twice the 4-ulp band that the double branch and torch stay
// within; that happens for mean^2/var from ~5 to ~100, above which the float
// expression never qualifies.  A NaN sum fails the comparison and stays NaN
// through the double branch.
// Only multiplies and subtractions run in double: every block of the
// one-kernel forward waits on this thread.  1/n comes from the host.
constexpr double BN_KEEP_FLOAT = 1.0 / 524288.0;

struct BnCount {
  double inv_n;
  float n;
};

static inline BnCount bn_count(long n) {
  return {1.0 / (double)n, (float)n};
}

__device__ __forceinline__ void bn_finalize_channel(
    float sf, float s2f, double s, double s2, BnCount cnt, int c,
    float* __restrict__ mean, float* __restrict__ invstd,
    float* __restrict__ running_mean, float* __restrict__ running_var,
    float momentum, float eps, float& m_out, float& is_out) {
  const float n = cnt.n;
  float m = sf / n;
  float v = fmaxf(s2f / n - m * m, 0.f);
  const double md = s * cnt.inv_n;
  double vd = s2 * cnt.inv_n - md * md;
  if (vd < 0.0) vd = 0.0;
  if (!(fabs((double)v - vd) <= BN_KEEP_FLOAT * vd)) {
    m = (float)md;
    v = (float)vd;
  }
  const float is = rsqrtf(v + eps);
  mean[c] = m;
  invstd[c] = is;
  if (running_mean != nullptr) {
    const float unbiased = v * (n / fmaxf(n - 1.f, 1.f));
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * m;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * unbiased;
  }
  m_out = m;
  is_out = is;
}

// chunked partial sums (grid.y chunks per channel) followed by a finalize
// kernel that also folds invstd and the running-stat update in-kernel (the
// previous host-side rsqrt/mul_/add_ chain was 5 extra kernel launches per
// BN call).
// slab layout [2][chunks][C], double (see bn_finalize_channel; a few KB):
// every slot plainly written (no zero-init, no atomics); the finalize kernel
// reduces over chunks
__global__ void bn_partial_kernel(const float* __restrict__ x,
                                  double* __restrict__ slab,
                                  int B, int C, int HW, FastDiv d_hw) {
  __shared__ double scratch[16];
  const int c = blockIdx.x;
  const int total = B * HW;
  const int per = (total + gridDim.y - 1) / gridDim.y;
  const int lo = blockIdx.y * per;
  const int hi = min(total, lo + per);
  double ts, ts2;
  bn_stat_sums(x, c, lo, hi, C, HW, d_hw, scratch, ts, ts2);
  if (threadIdx.x == 0) {
    const long chunks = gridDim.y;
    slab[(long)blockIdx.y * C + c] = ts;
    slab[chunks * C + (long)blockIdx.y * C + c] = ts2;
  }
}

__global__ void bn_finalize_kernel(const double* __restrict__ slab, int chunks,
                                   float* __restrict__ mean,
                                   float* __restrict__ invstd,
                                   float* __restrict__ running_mean,
                                   float* __restrict__ running_var,
                                   long* __restrict__ nbt, int C, BnCount cnt,
                                   float momentum, float eps) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  // num_batches_tracked rides along (was a separate aten long-add launch)
  if (c == 0 && nbt != nullptr) nbt[0] += 1;
  if (c >= C) return;
  double s = 0.0, s2 = 0.0;
  float sf = 0.f, s2f = 0.f;
  for (int k = 0; k < chunks; ++k) {
    const double a = slab[(long)k * C + c];
    const double b = slab[(long)chunks * C + (long)k * C + c];
    s += a;
    s2 += b;
    sf += (float)a;
    s2f += (float)b;
  }
  float m, is;
  bn_finalize_channel(sf, s2f, s, s2, cnt, c, mean, invstd, running_mean,
                      running_var, momentum, eps, m, is);
}

// chunks==1 (B*HW <= 8191: the 8x8-and-smaller VGG layers at B=32): ONE
// block per channel does the whole reduction AND the finalize — no slab
// tensor, no second launch.  Same math as partial+finalize (the double-
// precision block sum feeds the finalize directly).
__global__ void bn_stats_one_kernel(const float* __restrict__ x,
                                    float* __restrict__ mean,
                                    float* __restrict__ invstd,
                                    float* __restrict__ running_mean,
                                    float* __restrict__ running_var,
                                    long* __restrict__ nbt, int B, int C,
                                    int HW, float momentum, float eps,
                                    FastDiv d_hw, BnCount cnt) {
  __shared__ double scratch[16];
  const int c = blockIdx.x;
  if (c == 0 && threadIdx.x == 0 && nbt != nullptr) nbt[0] += 1;
  const int total = B * HW;
  double ts, ts2;
  bn_stat_sums(x, c, 0, total, C, HW, d_hw, scratch, ts, ts2);
  if (threadIdx.x == 0) {
    float m, is;
    bn_finalize_channel((float)ts, (float)ts2, ts, ts2, cnt, c, mean, invstd,
                        running_mean, running_var, momentum, eps, m, is);
  }
}

// Single-launch training forward for chunks==1: phase 1 is
// bn_stats_one_kernel; phase 2 applies the result to the channel the block
// has just reduced (re-read from cache: at most 8191 floats) and writes y,
// or — POOL — the 2x2-pooled y and its argmax index, one thread per pooled
// output, with no full-resolution y at all.
template <bool POOL>
__global__ void bn_fwd_one_kernel(const float* __restrict__ x,
                                  float* __restrict__ y,
                                  uint8_t* __restrict__ idx,
                                  float* __restrict__ mean,
                                  float* __restrict__ invstd,
                                  float* __restrict__ running_mean,
                                  float* __restrict__ running_var,
                                  long* __restrict__ nbt,
                                  const float* __restrict__ gamma,
                                  const float* __restrict__ beta, int B, int C,
                                  int HW, float momentum, float eps, bool relu,
                                  FastDiv d_hw, PoolGeom pg, BnCount cnt) {
  __shared__ double scratch[16];
  __shared__ float s_stat[2];
  const int c = blockIdx.x;
  if (c == 0 && threadIdx.x == 0 && nbt != nullptr) nbt[0] += 1;
  const int total = B * HW;
  double ts, ts2;
  bn_stat_sums(x, c, 0, total, C, HW, d_hw, scratch, ts, ts2);
  if (threadIdx.x == 0) {
    bn_finalize_channel((float)ts, (float)ts2, ts, ts2, cnt, c, mean, invstd,
                        running_mean, running_var, momentum, eps, s_stat[0],
                        s_stat[1]);
  }
  __syncthreads();
  const float m = s_stat[0], is = s_stat[1], g = gamma[c], bt = beta[c];
  if (POOL) {
    const int ohow = pg.OH * pg.OW;
    const int ptotal = B * ohow;
    slk_batched<BN_POOL_U, BnWindow>(
        (int)threadIdx.x, ptotal, (int)blockDim.x,
        [&](int j) {
          const unsigned b = pg.d_ohow.div((unsigned)j);
          const unsigned rem = pg.d_ohow.mod((unsigned)j, b);
          const long bc = (long)b * C + c;
          return bn_window_load(x + bc * HW, rem, bc * ohow + rem, pg);
        },
        [&](int, const BnWindow& v) {
          int bi;
          y[v.o] = bn_relu_pool_window(v.w, 2, m, is, g, bt, bi);
          idx[v.o] = (uint8_t)bi;
        });
  } else {
    struct Elem {
      float x;
      long off;
    };
    slk_batched<SLK_BN_U, Elem>(
        (int)threadIdx.x, total, (int)blockDim.x,
        [&](int i) {
          const unsigned b = d_hw.div((unsigned)i);
          const unsigned r = d_hw.mod((unsigned)i, b);
          const long off = ((long)b * C + c) * HW + r;
          return Elem{x[off], off};
        },
        [&](int, const Elem& v) { y[v.off] = bn_apply(v.x, m, is, g, bt, relu); });
  }
}

__global__ void bn_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                              const float* __restrict__ mean,
                              const float* __restrict__ invstd,
                              const float* __restrict__ gamma,
                              const float* __restrict__ beta, long total, int C,
                              int HW, bool relu, FastDiv d_hw, FastDiv d_c) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const unsigned bc = d_hw.div((unsigned)i);
    const int c = (int)(bc - d_c.div(bc) * (unsigned)C);
    y[i] = bn_apply(x[i], mean[c], invstd[c], gamma[c], beta[c], relu);
  }
}

// chunked-stats layers with a pool behind them: BN+ReLU+MaxPool apply, one
// thread per POOLED output (ptotal = B*C*OH*OW); writes pooled y + argmax
__global__ void bn_pool_fwd_kernel(const float* __restrict__ x,
                                   float* __restrict__ y,
                                   uint8_t* __restrict__ idx,
                                   const float* __restrict__ mean,
                                   const float* __restrict__ invstd,
                                   const float* __restrict__ gamma,
                                   const float* __restrict__ beta, long ptotal,
                                   int C, int HW, PoolGeom pg, FastDiv d_c) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < ptotal;
       i += (long)gridDim.x * blockDim.x) {
    const unsigned bc = pg.d_ohow.div((unsigned)i);
    const unsigned rem = pg.d_ohow.mod((unsigned)i, bc);
    const unsigned oh = pg.d_ow.div(rem);
    const unsigned ow = pg.d_ow.mod(rem, oh);
    const int c = (int)(bc - d_c.div(bc) * (unsigned)C);
    const float* xp = x + (long)bc * HW + (long)(oh * 2) * pg.W + ow * 2;
    int bi;
    y[i] = bn_relu_pool_window(xp, pg.W, mean[c], invstd[c], gamma[c], beta[c],
                               bi);
    idx[i] = (uint8_t)bi;
  }
}

// x and the incoming gradient's operands of element i of channel c's linear
// (b, hw) range, as the backward loops fetch them
struct BnElem {
  float x;
  BnGy g;
  long off;
};

template <bool POOL, bool RELU>
__device__ __forceinline__ BnElem bn_elem_load(
    const float* __restrict__ x, const float* __restrict__ gy,
    const float* __restrict__ relu_y, const uint8_t* __restrict__ idx, int i,
    int c, int C, int HW, const FastDiv& d_hw, const PoolGeom& pg) {
  const unsigned b = d_hw.div((unsigned)i);
  const unsigned r = d_hw.mod((unsigned)i, b);
  const unsigned bc = b * (unsigned)C + c;
  BnElem v;
  v.off = (long)bc * HW + r;
  v.x = x[v.off];
  v.g = bn_gy_load<POOL, RELU>(gy, relu_y, idx, v.off, bc, r, pg);
  return v;
}

// reductions for backward: sum(gy) and sum(gy * xhat) of channel c over the
// linear (b, hw) range [lo, hi), same per-thread order as bn_stat_sums.
// The incoming gradient is fetched through bn_gy_load, so the preceding ReLU's
// mask (and, POOL, the max-pool scatter) ride inside the reduction — no
// standalone relu_bwd / maxpool_bwd launch, no extra full tensor pass.
template <bool POOL>
__device__ __forceinline__ void bn_bwd_sums(
    const float* __restrict__ x, const float* __restrict__ gy,
    const float* __restrict__ relu_y, const uint8_t* __restrict__ idx, float m,
    float is, int c, int lo, int hi, int C, int HW, const FastDiv& d_hw,
    const PoolGeom& pg, double* scratch, double& ts, double& tsx) {
  double s = 0.0, sx = 0.0;
  bn_relu_dispatch<POOL>(relu_y, [&](auto R) {
    constexpr bool RELU = decltype(R)::value;
    slk_batched<SLK_BN_U, BnElem>(
        lo + (int)threadIdx.x, hi, (int)blockDim.x,
        [&](int i) {
          return bn_elem_load<POOL, RELU>(x, gy, relu_y, idx, i, c, C, HW, d_hw,
                                          pg);
        },
        [&](int, const BnElem& v) {
          // float xhat, then one add and one fma in double: what
          // `s += g; sx += g * (double)((x - m) * is)` has always compiled to
          const double g = (double)bn_gy_select<POOL, RELU>(v.g);
          s += g;
          sx = __builtin_fma(g, (double)((v.x - m) * is), sx);
        });
  });
  ts = slk_block_sum(s, scratch);
  __syncthreads();
  tsx = slk_block_sum(sx, scratch);
}

// chunked over grid.y like the forward stats (one block per channel leaves
// most CUs idle at C=64)
template <bool POOL>
__global__ void bn_bwd_reduce_kernel(const float* __restrict__ x,
                                     const float* __restrict__ gy,
                                     const float* __restrict__ relu_y,
                                     const uint8_t* __restrict__ idx,
                                     const float* __restrict__ mean,
                                     const float* __restrict__ invstd,
                                     float* __restrict__ slab, int B, int C,
                                     int HW, FastDiv d_hw, PoolGeom pg) {
  __shared__ double scratch[16];
  const int c = blockIdx.x;
  const int total = B * HW;
  const int per = (total + gridDim.y - 1) / gridDim.y;
  const int lo = blockIdx.y * per;
  const int hi = min(total, lo + per);
  double ts, tsx;
  bn_bwd_sums<POOL>(x, gy, relu_y, idx, mean[c], invstd[c], c, lo, hi, C, HW,
                    d_hw, pg, scratch, ts, tsx);
  if (threadIdx.x == 0) {
    const long chunks = gridDim.y;
    slab[(long)blockIdx.y * C + c] = (float)ts;
    slab[chunks * C + (long)blockIdx.y * C + c] = (float)tsx;
  }
}

// chunks==1 twin of bn_bwd_reduce: per-channel block writes the two sums
// directly (no slab, no bn_bwd_finalize launch)
__global__ void bn_bwd_reduce_one_kernel(const float* __restrict__ x,
                                         const float* __restrict__ gy,
                                         const float* __restrict__ relu_y,
                                         const float* __restrict__ mean,
                                         const float* __restrict__ invstd,
                                         float* __restrict__ sum_gy,
                                         float* __restrict__ sum_gy_xhat,
                                         int B, int C, int HW, FastDiv d_hw) {
  __shared__ double scratch[16];
  const int c = blockIdx.x;
  double ts, tsx;
  bn_bwd_sums<false>(x, gy, relu_y, nullptr, mean[c], invstd[c], c, 0, B * HW,
                     C, HW, d_hw, PoolGeom{}, scratch, ts, tsx);
  if (threadIdx.x == 0) {
    sum_gy[c] = (float)ts;
    sum_gy_xhat[c] = (float)tsx;
  }
}

// Single-launch training backward for chunks==1: phase 1 is
// bn_bwd_reduce_one_kernel, phase 2 the bn_bwd_dx math for the channel the
// block has just reduced.  Writes gx and the two sums (ggamma, gbeta).
template <bool POOL>
__global__ void bn_bwd_one_kernel(const float* __restrict__ x,
                                  const float* __restrict__ gy,
                                  const float* __restrict__ relu_y,
                                  const uint8_t* __restrict__ idx,
                                  const float* __restrict__ mean,
                                  const float* __restrict__ invstd,
                                  const float* __restrict__ gamma,
                                  float* __restrict__ sum_gy,
                                  float* __restrict__ sum_gy_xhat,
                                  float* __restrict__ gx, int B, int C, int HW,
                                  float inv_n, FastDiv d_hw, PoolGeom pg) {
  __shared__ double scratch[16];
  __shared__ float s_sum[2];
  const int c = blockIdx.x;
  const float m = mean[c], is = invstd[c];
  const int total = B * HW;
  double ts, tsx;
  bn_bwd_sums<POOL>(x, gy, relu_y, idx, m, is, c, 0, total, C, HW, d_hw, pg,
                    scratch, ts, tsx);
  if (threadIdx.x == 0) {
    s_sum[0] = (float)ts;
    s_sum[1] = (float)tsx;
    sum_gy[c] = (float)ts;
    sum_gy_xhat[c] = (float)tsx;
  }
  __syncthreads();
  const float sgy = s_sum[0], sgx = s_sum[1], gm = gamma[c];
  bn_relu_dispatch<POOL>(relu_y, [&](auto R) {
    constexpr bool RELU = decltype(R)::value;
    slk_batched<SLK_BN_U, BnElem>(
        (int)threadIdx.x, total, (int)blockDim.x,
        [&](int i) {
          return bn_elem_load<POOL, RELU>(x, gy, relu_y, idx, i, c, C, HW, d_hw,
                                          pg);
        },
        [&](int, const BnElem& v) {
          gx[v.off] = bn_dx(v.x, bn_gy_select<POOL, RELU>(v.g), m, is, gm, sgy,
                            sgx, inv_n);
        });
  });
}

__global__ void bn_bwd_finalize_kernel(const float* __restrict__ slab, int chunks,
                                       float* __restrict__ sum_gy,
                                       float* __restrict__ sum_gy_xhat, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float s = 0.f, sx = 0.f;
  for (int k = 0; k < chunks; ++k) {
    s += slab[(long)k * C + c];
    sx += slab[(long)chunks * C + (long)k * C + c];
  }
  sum_gy[c] = s;
  sum_gy_xhat[c] = sx;
}

template <bool POOL>
__global__ void bn_bwd_dx_kernel(const float* __restrict__ x,
                                 const float* __restrict__ gy,
                                 const float* __restrict__ relu_y,
                                 const uint8_t* __restrict__ idx,
                                 const float* __restrict__ mean,
                                 const float* __restrict__ invstd,
                                 const float* __restrict__ gamma,
                                 const float* __restrict__ sum_gy,
                                 const float* __restrict__ sum_gy_xhat,
                                 float* __restrict__ gx, long total, int C, int HW,
                                 float inv_n, bool training, FastDiv d_hw,
                                 FastDiv d_c, PoolGeom pg) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const unsigned bc = d_hw.div((unsigned)i);
    const unsigned r = d_hw.mod((unsigned)i, bc);
    const int c = (int)(bc - d_c.div(bc) * (unsigned)C);
    const float is = invstd[c];
    const float g = bn_gy_at<POOL>(gy, relu_y, idx, i, bc, r, pg);
    if (training) {
      gx[i] = bn_dx(x[i], g, mean[c], is, gamma[c], sum_gy[c], sum_gy_xhat[c],
                    inv_n);
    } else {
      gx[i] = g * gamma[c] * is;
    }
  }
}

template <typename T>
static inline T* opt_ptr(const c10::optional<at::Tensor>& t) {
  return t.has_value() ? t->data_ptr<T>() : nullptr;
}

std::vector<at::Tensor> bn2d_stats_fused(const at::Tensor& x,
                                         c10::optional<at::Tensor> running_mean,
                                         c10::optional<at::Tensor> running_var,
                                         c10::optional<at::Tensor> num_batches_tracked,
                                         double momentum, double eps) {
  const int B = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
  auto mean = at::empty({C}, x.options());
  auto invstd = at::empty({C}, x.options());
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const int chunks = reduce_chunks((long)B * HW);
  FastDiv d_hw;
  d_hw.init(HW);
  if (chunks == 1) {
    hipLaunchKernelGGL(bn_stats_one_kernel, dim3(C), dim3(256), 0, stream,
                       x.data_ptr<float>(), mean.data_ptr<float>(),
                       invstd.data_ptr<float>(), opt_ptr<float>(running_mean),
                       opt_ptr<float>(running_var),
                       opt_ptr<long>(num_batches_tracked),
                       B, C, HW, (float)momentum, (float)eps, d_hw,
                       bn_count((long)B * HW));
    return {mean, invstd};
  }
  auto slab = at::empty({2, chunks, C}, x.options().dtype(at::kDouble));
  hipLaunchKernelGGL(bn_partial_kernel, dim3(C, chunks), dim3(256), 0, stream,
                     x.data_ptr<float>(), slab.data_ptr<double>(), B, C, HW,
                     d_hw);
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(ceil_div(C, 256)), dim3(256), 0,
                     stream, slab.data_ptr<double>(), chunks,
                     mean.data_ptr<float>(), invstd.data_ptr<float>(),
                     opt_ptr<float>(running_mean), opt_ptr<float>(running_var),
                     opt_ptr<long>(num_batches_tracked),
                     C, bn_count((long)B * HW), (float)momentum, (float)eps);
  return {mean, invstd};
}

at::Tensor bn2d_fwd(const at::Tensor& x, const at::Tensor& mean,
                    const at::Tensor& invstd, const at::Tensor& gamma,
                    const at::Tensor& beta, bool relu) {
  auto y = at::empty_like(x);
  const long total = x.numel();
  const int C = x.size(1), HW = x.size(2) * x.size(3);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  int grid = (int)std::min<long>((total + 255) / 256, 2048);
  FastDiv d_hw, d_c;
  d_hw.init(HW);
  d_c.init(C);
  TORCH_CHECK(total <= (1l << 24), "bn_fwd: FastDiv range");
  hipLaunchKernelGGL(bn_fwd_kernel, dim3(grid), dim3(256), 0, stream,
                     x.data_ptr<float>(), y.data_ptr<float>(),
                     mean.data_ptr<float>(), invstd.data_ptr<float>(),
                     gamma.data_ptr<float>(), beta.data_ptr<float>(), total, C, HW,
                     relu, d_hw, d_c);
  return y;
}

// Training-mode forward of a whole BN block: statistics + running-stat update
// + apply (+ReLU) (+MaxPool 2x2).  chunks==1 layers run as ONE launch; larger
// layers keep the chunked statistics and get one apply launch.  With pool the
// output is the pooled y plus its uint8 argmax; no full-resolution y exists.
// Returns {y, mean, invstd} or {y, mean, invstd, idx}.
std::vector<at::Tensor> bn2d_train_fwd(const at::Tensor& x, const at::Tensor& gamma,
                                       const at::Tensor& beta,
                                       c10::optional<at::Tensor> running_mean,
                                       c10::optional<at::Tensor> running_var,
                                       c10::optional<at::Tensor> num_batches_tracked,
                                       double momentum, double eps, bool relu,
                                       bool pool) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && x.is_contiguous() &&
              x.scalar_type() == at::kFloat, "bn2d_train_fwd: x");
  const int B = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int HW = H * W;
  TORCH_CHECK(x.numel() <= (1l << 24), "bn2d_train_fwd: FastDiv range");
  TORCH_CHECK(!pool || (relu && H % 2 == 0 && W % 2 == 0 && HW > 0),
              "bn2d_train_fwd: pool needs relu and even H, W");
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const PoolGeom pg = pool ? pool_geom(H, W) : PoolGeom{};
  at::Tensor y, idx;
  if (pool) {
    y = at::empty({B, C, H / 2, W / 2}, x.options());
    idx = at::empty({B, C, H / 2, W / 2}, x.options().dtype(at::kByte));
  }
  if (reduce_chunks((long)B * HW) == 1) {
    auto mean = at::empty({C}, x.options());
    auto invstd = at::empty({C}, x.options());
    if (!pool) y = at::empty_like(x);
    FastDiv d_hw;
    d_hw.init(HW);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(C), dim3(256), 0, stream,
                         x.data_ptr<float>(), y.data_ptr<float>(),
                         pool ? idx.data_ptr<uint8_t>() : nullptr,
                         mean.data_ptr<float>(), invstd.data_ptr<float>(),
                         opt_ptr<float>(running_mean), opt_ptr<float>(running_var),
                         opt_ptr<long>(num_batches_tracked),
                         gamma.data_ptr<float>(), beta.data_ptr<float>(), B, C,
                         HW, (float)momentum, (float)eps, relu, d_hw, pg,
                         bn_count((long)B * HW));
    };
    if (pool) launch(bn_fwd_one_kernel<true>);
    else launch(bn_fwd_one_kernel<false>);
    if (pool) return {y, mean, invstd, idx};
    return {y, mean, invstd};
  }
  auto stats = bn2d_stats_fused(x, running_mean, running_var, num_batches_tracked,
                                momentum, eps);
  if (!pool) return {bn2d_fwd(x, stats[0], stats[1], gamma, beta, relu), stats[0],
                     stats[1]};
  const long ptotal = y.numel();
  int grid = (int)std::min<long>((ptotal + 255) / 256, 2048);
  FastDiv d_c;
  d_c.init(C);
  hipLaunchKernelGGL(bn_pool_fwd_kernel, dim3(grid), dim3(256), 0, stream,
                     x.data_ptr<float>(), y.data_ptr<float>(),
                     idx.data_ptr<uint8_t>(), stats[0].data_ptr<float>(),
                     stats[1].data_ptr<float>(), gamma.data_ptr<float>(),
                     beta.data_ptr<float>(), ptotal, C, HW, pg, d_c);
  return {y, stats[0], stats[1], idx};
}

// idx given: gy and relu_y are the POOLED gradient / output of a fused
// BN+ReLU+MaxPool block.  one_launch: chunks==1 training layers run
// reduce + dx as a single kernel.
static std::vector<at::Tensor> bn2d_bwd_impl(const at::Tensor& x, const at::Tensor& gy,
                                             const at::Tensor& gamma,
                                             const at::Tensor& mean,
                                             const at::Tensor& invstd, bool training,
                                             const c10::optional<at::Tensor>& relu_y,
                                             const c10::optional<at::Tensor>& idx,
                                             bool one_launch) {
  const float* ry = opt_ptr<float>(relu_y);
  const bool pool = idx.has_value();
  const uint8_t* ip = pool ? idx->data_ptr<uint8_t>() : nullptr;
  const int B = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
  const long total = x.numel();
  TORCH_CHECK(total <= (1l << 24), "bn_bwd: FastDiv range");
  PoolGeom pg{};
  if (pool) {
    const int H = x.size(2), W = x.size(3);
    TORCH_CHECK(training && ry != nullptr && H % 2 == 0 && W % 2 == 0,
                "bn_bwd: pooled form needs training mode, relu_y and even H, W");
    TORCH_CHECK(gy.numel() * 4 == total && relu_y->numel() * 4 == total &&
                idx->numel() * 4 == total, "bn_bwd: pooled operand shapes");
    pg = pool_geom(H, W);
  } else {
    TORCH_CHECK(gy.numel() == total && (ry == nullptr || relu_y->numel() == total),
                "bn_bwd: operand shapes");
  }
  auto sum_gy = at::empty({C}, x.options());
  auto sum_gy_xhat = at::empty({C}, x.options());
  auto gx = at::empty_like(x);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const int rchunks = reduce_chunks((long)B * HW);
  const float inv_n = 1.0f / (float)((long)B * HW);
  FastDiv d_hw;
  d_hw.init(HW);
  if (rchunks == 1 && one_launch && training) {
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(C), dim3(256), 0, stream,
                         x.data_ptr<float>(), gy.data_ptr<float>(), ry, ip,
                         mean.data_ptr<float>(), invstd.data_ptr<float>(),
                         gamma.data_ptr<float>(), sum_gy.data_ptr<float>(),
                         sum_gy_xhat.data_ptr<float>(), gx.data_ptr<float>(), B,
                         C, HW, inv_n, d_hw, pg);
    };
    if (pool) launch(bn_bwd_one_kernel<true>);
    else launch(bn_bwd_one_kernel<false>);
    return {gx, sum_gy_xhat, sum_gy};
  }
  if (rchunks == 1 && !pool) {
    hipLaunchKernelGGL(bn_bwd_reduce_one_kernel, dim3(C), dim3(256), 0, stream,
                       x.data_ptr<float>(), gy.data_ptr<float>(), ry,
                       mean.data_ptr<float>(), invstd.data_ptr<float>(),
                       sum_gy.data_ptr<float>(), sum_gy_xhat.data_ptr<float>(),
                       B, C, HW, d_hw);
  } else {
    auto slab = at::empty({2, rchunks, C}, x.options());
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(C, rchunks), dim3(256), 0, stream,
                         x.data_ptr<float>(), gy.data_ptr<float>(), ry, ip,
                         mean.data_ptr<float>(), invstd.data_ptr<float>(),
                         slab.data_ptr<float>(), B, C, HW, d_hw, pg);
    };
    if (pool) launch(bn_bwd_reduce_kernel<true>);
    else launch(bn_bwd_reduce_kernel<false>);
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(ceil_div(C, 256)), dim3(256), 0,
                       stream, slab.data_ptr<float>(), rchunks,
                       sum_gy.data_ptr<float>(), sum_gy_xhat.data_ptr<float>(), C);
  }
  int grid = (int)std::min<long>((total + 255) / 256, 2048);
  FastDiv d_c;
  d_c.init(C);
  auto launch_dx = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, stream,
                       x.data_ptr<float>(), gy.data_ptr<float>(), ry, ip,
                       mean.data_ptr<float>(), invstd.data_ptr<float>(),
                       gamma.data_ptr<float>(), sum_gy.data_ptr<float>(),
                       sum_gy_xhat.data_ptr<float>(), gx.data_ptr<float>(), total,
                       C, HW, inv_n, training, d_hw, d_c, pg);
  };
  if (pool) launch_dx(bn_bwd_dx_kernel<true>);
  else launch_dx(bn_bwd_dx_kernel<false>);
  // ggamma = sum_gy_xhat, gbeta = sum_gy
  return {gx, sum_gy_xhat, sum_gy};
}

std::vector<at::Tensor> bn2d_bwd(const at::Tensor& x, const at::Tensor& gy,
                                 const at::Tensor& gamma, const at::Tensor& mean,
                                 const at::Tensor& invstd,
                                 c10::optional<at::Tensor> relu_y) {
  return bn2d_bwd_impl(x, gy, gamma, mean, invstd, true, relu_y, c10::nullopt,
                       false);
}

std::vector<at::Tensor> bn2d_bwd_eval(const at::Tensor& x, const at::Tensor& gy,
                                      const at::Tensor& gamma, const at::Tensor& mean,
                                      const at::Tensor& invstd,
                                      c10::optional<at::Tensor> relu_y) {
  return bn2d_bwd_impl(x, gy, gamma, mean, invstd, false, relu_y, c10::nullopt,
                       false);
}

// Training-mode backward of a whole BN block (the counterpart of
// bn2d_train_fwd): one launch for chunks==1 layers; with idx, gy and relu_y
// are pooled and no full-resolution gradient is materialised.
std::vector<at::Tensor> bn2d_train_bwd(const at::Tensor& x, const at::Tensor& gy,
                                       const at::Tensor& gamma,
                                       const at::Tensor& mean,
                                       const at::Tensor& invstd,
                                       c10::optional<at::Tensor> relu_y,
                                       c10::optional<at::Tensor> idx) {
  TORCH_CHECK(x.is_contiguous() && gy.is_contiguous(), "bn2d_train_bwd: layout");
  return bn2d_bwd_impl(x, gy, gamma, mean, invstd, true, relu_y, idx, true);
}

// ---------------- fused transformer epilogue ------------------------------
// h = dropout(x) + residual;  y = LayerNorm(h)   in ONE kernel
// (SURVEY §2.4 fused bias-residual-LN row: the bias itself rides in the
// producing GEMM's epilogue, so the launches this removes are the dropout
// and the aten residual add — the BertSelfOutput/Output chain goes
// 4 launches -> 2 per sublayer).  h (the LN input) and the dropout mask are
// written out for the backward, which composes the existing ln_bwd +
// dropout_bwd + colsum kernels in Python.
template <bool DROPOUT>
__global__ void drop_res_ln_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ res,
    float* __restrict__ h, float* __restrict__ y,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    float* __restrict__ mean_out, float* __restrict__ invstd_out,
    unsigned char* __restrict__ mask, int D, float eps, float p,
    float inv_keep, uint64_t seed, const long* __restrict__ offset_ptr) {
  __shared__ float scratch[16];
  __shared__ float s_mean, s_invstd;
  const uint64_t offset = offset_ptr ? (uint64_t)offset_ptr[0] : 0;
  const long row = blockIdx.x;
  const float* xr = x + row * D;
  const float* rr = res + row * D;
  float* hr = h + row * D;
  float s = 0.f;
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    float v = xr[d];
    if (DROPOUT) {
      const bool keep = slk_uniform(seed, offset, row * D + d) >= p;
      v = keep ? v * inv_keep : 0.f;
      mask[row * D + d] = keep;
    }
    v += rr[d];
    hr[d] = v;
    s += v;
  }
  float total = slk_block_sum(s, scratch);
  if (threadIdx.x == 0) s_mean = total / D;
  __syncthreads();
  const float m = s_mean;
  float var = 0.f;
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    const float t = hr[d] - m;
    var += t * t;
  }
  float vtotal = slk_block_sum(var, scratch);
  if (threadIdx.x == 0) s_invstd = rsqrtf(vtotal / D + eps);
  __syncthreads();
  const float is = s_invstd;
  float* yr = y + row * D;
  for (int d = threadIdx.x; d < D; d += blockDim.x)
    yr[d] = (hr[d] - m) * is * gamma[d] + beta[d];
  if (threadIdx.x == 0) {
    mean_out[row] = m;
    invstd_out[row] = is;
  }
}

std::vector<at::Tensor> drop_res_ln_fwd(const at::Tensor& x,
                                        const at::Tensor& res,
                                        const at::Tensor& gamma,
                                        const at::Tensor& beta, double eps,
                                        double p, int64_t seed,
                                        c10::optional<at::Tensor> offset) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.scalar_type() == at::kFloat);
  const long R = x.size(0);
  const int D = x.size(1);
  auto h = at::empty_like(x);
  auto y = at::empty_like(x);
  auto mean = at::empty({R}, x.options());
  auto invstd = at::empty({R}, x.options());
  const bool drop = p > 0.0;
  auto mask = at::empty({drop ? R : 0, D}, x.options().dtype(at::kByte));
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const int threads = D >= 256 ? 256 : 64;
  if (drop) {
    hipLaunchKernelGGL(drop_res_ln_fwd_kernel<true>, dim3(R), dim3(threads), 0,
                       stream, x.data_ptr<float>(), res.data_ptr<float>(),
                       h.data_ptr<float>(), y.data_ptr<float>(),
                       gamma.data_ptr<float>(), beta.data_ptr<float>(),
                       mean.data_ptr<float>(), invstd.data_ptr<float>(),
                       mask.data_ptr<unsigned char>(), D, (float)eps, (float)p,
                       (float)(1.0 / (1.0 - p)), (uint64_t)seed,
                       offset.has_value() ? offset->data_ptr<long>() : nullptr);
  } else {
    hipLaunchKernelGGL(drop_res_ln_fwd_kernel<false>, dim3(R), dim3(threads), 0,
                       stream, x.data_ptr<float>(), res.data_ptr<float>(),
                       h.data_ptr<float>(), y.data_ptr<float>(),
                       gamma.data_ptr<float>(), beta.data_ptr<float>(),
                       mean.data_ptr<float>(), invstd.data_ptr<float>(),
                       nullptr, D, (float)eps, 0.f, 1.f, 0, nullptr);
  }
  return {y, h, mean, invstd, mask};
}

// ---------------- LayerNorm (last-dim) ----------------

// one block per row (rows up to ~4K cols; looping supports any D)
__global__ void ln_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                              const float* __restrict__ gamma,
                              const float* __restrict__ beta,
                              float* __restrict__ mean_out,
                              float* __restrict__ invstd_out, int D, float eps) {
  __shared__ float scratch[16];
  __shared__ float s_mean, s_invstd;
  const long row = blockIdx.x;
  const float* xr = x + row * D;
  float s = 0.f;
  for (int d = threadIdx.x; d < D; d += blockDim.x) s += xr[d];
  float total = slk_block_sum(s, scratch);
  if (threadIdx.x == 0) s_mean = total / D;
  __syncthreads();
  const float m = s_mean;
  float v = 0.f;
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    const float t = xr[d] - m;
    v += t * t;
  }
  float vtotal = slk_block_sum(v, scratch);
  if (threadIdx.x == 0) s_invstd = rsqrtf(vtotal / D + eps);
  __syncthreads();
  const float is = s_invstd;
  float* yr = y + row * D;
  for (int d = threadIdx.x; d < D; d += blockDim.x)
    yr[d] = (xr[d] - m) * is * gamma[d] + beta[d];
  if (threadIdx.x == 0) {
    mean_out[row] = m;
    invstd_out[row] = is;
  }
}

__global__ void ln_bwd_dx_kernel(const float* __restrict__ gy,
                                 const float* __restrict__ x,
                                 const float* __restrict__ gamma,
                                 const float* __restrict__ mean,
                                 const float* __restrict__ invstd,
                                 float* __restrict__ gx, int D) {
  __shared__ float scratch[16];
  __shared__ float s_a, s_b;
  const long row = blockIdx.x;
  const float* xr = x + row * D;
  const float* gr = gy + row * D;
  const float m = mean[row], is = invstd[row];
  float a = 0.f, b = 0.f;
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    const float gg = gr[d] * gamma[d];
    a += gg;
    b += gg * (xr[d] - m) * is;
  }
  float ta = slk_block_sum(a, scratch);
  if (threadIdx.x == 0) s_a = ta / D;
  __syncthreads();  // scratch reuse barrier between the two block sums
  float tb = slk_block_sum(b, scratch);
  if (threadIdx.x == 0) s_b = tb / D;
  __syncthreads();
  float* oxr = gx + row * D;
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    // no contraction: fma(gy, gamma, -s_a) keeps the product unrounded while
    // s_a holds its rounded sum, and the residual times invstd is not small
    // (D == 1: gx must be exactly 0, came out as invstd * ulp)
#pragma clang fp contract(off)
    const float xhat = (xr[d] - m) * is;
    const float gg = gr[d] * gamma[d];
    oxr[d] = is * (gg - s_a - xhat * s_b);
  }
}

// column reductions for dgamma/dbeta, CHUNKED over rows: grid.y row-chunks
// write partial slabs, a finalize pass sums them.  (The first version was a
// thread-per-column serial loop over ALL rows: at BERT shape [4096, 768]
// that is a 3-block launch — 1% of the chip — and profiled at 1.15 ms per
// call, 46% of the whole BERT step.)
__global__ void ln_bwd_dgamma_kernel(const float* __restrict__ gy,
                                     const float* __restrict__ x,
                                     const float* __restrict__ mean,
                                     const float* __restrict__ invstd,
                                     float* __restrict__ slab, long R, int D) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= D) return;
  const long per = (R + gridDim.y - 1) / gridDim.y;
  const long lo = (long)blockIdx.y * per;
  const long hi = min(R, lo + per);
  float sg = 0.f, sb = 0.f;
  for (long r = lo; r < hi; ++r) {
    const float g = gy[r * D + d];
    sg += g * (x[r * D + d] - mean[r]) * invstd[r];
    sb += g;
  }
  slab[(long)blockIdx.y * D + d] = sg;
  slab[(long)gridDim.y * D + (long)blockIdx.y * D + d] = sb;
}

__global__ void ln_bwd_dgamma_finalize_kernel(const float* __restrict__ slab,
                                              int chunks,
                                              float* __restrict__ dgamma,
                                              float* __restrict__ dbeta, int D) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= D) return;
  float sg = 0.f, sb = 0.f;
  for (int k = 0; k < chunks; ++k) {
    sg += slab[(long)k * D + d];
    sb += slab[(long)chunks * D + (long)k * D + d];
  }
  dgamma[d] = sg;
  dbeta[d] = sb;
}

std::vector<at::Tensor> layernorm_fwd(const at::Tensor& x, const at::Tensor& gamma,
                                      const at::Tensor& beta, double eps) {
  const long R = x.size(0);
  const int D = x.size(1);
  auto y = at::empty_like(x);
  auto mean = at::empty({R}, x.options());
  auto invstd = at::empty({R}, x.options());
  auto stream = c10::hip::getCurrentHIPStream().stream();
  int threads = D >= 256 ? 256 : 64;
  hipLaunchKernelGGL(ln_fwd_kernel, dim3(R), dim3(threads), 0, stream,
                     x.data_ptr<float>(), y.data_ptr<float>(),
                     gamma.data_ptr<float>(), beta.data_ptr<float>(),
                     mean.data_ptr<float>(), invstd.data_ptr<float>(), D,
                     (float)eps);
  return {y, mean, invstd};
}

std::vector<at::Tensor> layernorm_bwd(const at::Tensor& gy, const at::Tensor& x,
                                      const at::Tensor& gamma, const at::Tensor& mean,
                                      const at::Tensor& invstd) {
  const long R = x.size(0);
  const int D = x.size(1);
  auto gx = at::empty_like(x);
  auto dgamma = at::empty({D}, x.options());
  auto dbeta = at::empty({D}, x.options());
  auto stream = c10::hip::getCurrentHIPStream().stream();
  int threads = D >= 256 ? 256 : 64;
  hipLaunchKernelGGL(ln_bwd_dx_kernel, dim3(R), dim3(threads), 0, stream,
                     gy.data_ptr<float>(), x.data_ptr<float>(),
                     gamma.data_ptr<float>(), mean.data_ptr<float>(),
                     invstd.data_ptr<float>(), gx.data_ptr<float>(), D);
  // row-chunk count: fill the chip (ceil(D/256) column-blocks per chunk)
  int chunks = (int)std::min<long>(std::max<long>(R / 64, 1), 64);
  auto slab = at::empty({2, chunks, D}, x.options());
  hipLaunchKernelGGL(ln_bwd_dgamma_kernel,
                     dim3(ceil_div(D, 256), chunks), dim3(256), 0,
                     stream, gy.data_ptr<float>(), x.data_ptr<float>(),
                     mean.data_ptr<float>(), invstd.data_ptr<float>(),
                     slab.data_ptr<float>(), R, D);
  hipLaunchKernelGGL(ln_bwd_dgamma_finalize_kernel, dim3(ceil_div(D, 256)),
                     dim3(256), 0, stream, slab.data_ptr<float>(), chunks,
                     dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), D);
  return {gx, dgamma, dbeta};
}

}  // namespace slk
