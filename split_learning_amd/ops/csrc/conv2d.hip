// Implicit-GEMM NCHW fp32 convolution on the MFMA tile framework.
//
// Forward:     y[Co, (B,OH,OW)] = W[Co, (Ci,KH,KW)] @ im2col(x)
// Bwd-data:    gx[Ci, (B,H,W)]  = W^T-gather @ col(gy)   (stride-aware)
// Bwd-weight:  gw[Co, (Ci,KH,KW)] = gy-gather @ im2col(x)^T
//
// Round-2 findings (profiles/, conv_microbench + PMC on MI355X):
// * the round-1 hypothesis "gathers are issue-bound" was WRONG at kernel
//   grain: a bounds-free pre-padded gather tied the bounds-checked direct
//   gather within noise (42.2 vs 42.7 us on conv1_2) because the core is
//   barrier/latency-paced, not VALU-bound — while its pad/flipT prep kernels
//   cost ~0.27 ms/step.  The direct gather is the only one; the pre-padded
//   experiment has been removed (profiles/SUMMARY.md keeps the numbers).
// * the real levers are in tile_gemm.h (LDS ping-pong, batched reads) and
//   split-K slab stores (AtomicStore at split 64 = 4M atomicAdds on a 65 KB
//   output: the 512ch/2x2 tail layers ran 2x slower than MIOpen).
// * bwd-weight keeps one genuine round-2 win: the gy (A-side) per-lane k
//   decomposition collapses via the prepK window hoist — when OH*OW % 16
//   == 0 a BK=16 window stays inside one (b, rem0) row, so b/rem decompose
//   once per tile on the scalar unit and the per-lane address is
//   row_m + dk + kctx.a_off.
// Geometry (KH, KW, stride, pad) is a TEMPLATE specialisation for the model
// zoo's cases; runtime dims divide through FastDiv magics (common.h);
// gathers are BRANCHLESS (clamped addresses + cndmask selects).
// Which kernel a call runs (direct here, or a Winograd form in wino.hip) is
// decided by the routing table in conv_route.h.
#include <tuple>

#include "conv_route.h"
#include "tile_gemm.h"
#include "torch_util.h"

namespace slk {

// wino.hip
at::Tensor conv2d_wino(const at::Tensor&, const at::Tensor&,
                       c10::optional<at::Tensor>, int, bool);
at::Tensor conv2d_wino_bwdw(const at::Tensor&, const at::Tensor&, int);
at::Tensor conv2d_wino_fused(const at::Tensor&, const at::Tensor&,
                             c10::optional<at::Tensor>, int, bool);
at::Tensor conv2d_wino_bwdw_fused(const at::Tensor&, const at::Tensor&, int);
std::tuple<at::Tensor, at::Tensor> conv2d_bwd_pair(const at::Tensor&,
                                                   const at::Tensor&,
                                                   const at::Tensor&, int, int);

// SLK_WINO level for conv_route.h, read once per process
static int wino_level() {
  static const int v = [] {
    const char* e = std::getenv("SLK_WINO");
    return e ? atoi(e) : 1;
  }();
  return v;
}

struct ConvGeom {
  int B, Ci, H, W, Co, KH, KW, OH, OW, stride, pad;
  FastDiv d_ohow, d_ow, d_hw, d_w, d_khkw, d_kw;  // runtime-dim magics
};

// compile-time geometry: CKH=0 means runtime (generic fallback); pad is
// always runtime (one add in hoisted prep code — not worth a template axis)
template <int CKH, int CKW, int CS>
struct Geo {
  static constexpr bool fixed = CKH > 0;
  __device__ static int kh_kw(const ConvGeom& g) { return fixed ? CKH * CKW : g.KH * g.KW; }
  __device__ static int stride(const ConvGeom& g) { return fixed ? CS : g.stride; }
  // k -> (c, kh, kw) with strength-reduced division when fixed
  __device__ static void dk(const ConvGeom& g, int k, int& c, int& kh, int& kw) {
    if (fixed) {
      c = k / (CKH * CKW);
      const int r = k - c * (CKH * CKW);
      kh = r / CKW;
      kw = r - kh * CKW;
    } else {
      c = g.d_khkw.div(k);
      const int r = g.d_khkw.mod(k, c);
      kh = g.d_kw.div(r);
      kw = g.d_kw.mod(r, kh);
    }
  }
};

__device__ __forceinline__ float sel0(float v, bool keep) { return keep ? v : 0.f; }

// ---------------- forward ---------------------------------------------------
template <int CKH, int CKW, int CS>
struct ConvFwdGather {
  using G = Geo<CKH, CKW, CS>;
  const float* w;  // [Co, Ci, KH, KW]
  const float* x;  // [B, Ci, H, W]
  ConvGeom geo;

  struct KCtx {};
  __device__ KCtx prepK(int) const { return {}; }

  // int32 offsets against the functor's uniform (SGPR) base pointers: the
  // pointer-context form cost ~8 VGPR of the register budget (one wave/SIMD
  // of occupancy; see StridedGather).  Conv tensors are < 2^31 elements.
  struct ACtx { int off; bool valid; };
  struct BCtx { int boff, ihb, iwb; bool valid; };

  __device__ ACtx prepA(int, int m, bool valid, int) const {
    return {(int)((long)m * (geo.Ci * G::kh_kw(geo))), valid};
  }
  __device__ float loadA(const ACtx& c, const KCtx&, int k, bool kv) const {
    return sel0(w[c.off + k], c.valid & kv);
  }
  __device__ BCtx prepB(int, int n, bool valid, int) const {
    const unsigned b = geo.d_ohow.div(n);
    const unsigned rem = geo.d_ohow.mod(n, b);
    const unsigned oh = geo.d_ow.div(rem);
    const unsigned ow = geo.d_ow.mod(rem, oh);
    return {(int)((long)b * geo.Ci * geo.H * geo.W),
            (int)oh * G::stride(geo) - geo.pad,
            (int)ow * G::stride(geo) - geo.pad, valid};
  }
  __device__ float loadB(const BCtx& c, const KCtx&, int k, bool kv) const {
    int ci, kh, kw;
    G::dk(geo, k, ci, kh, kw);
    const int ih = c.ihb + kh;
    const int iw = c.iwb + kw;
    const bool in = (unsigned)ih < (unsigned)geo.H && (unsigned)iw < (unsigned)geo.W;
    const int ihc = in ? ih : 0;
    const int iwc = in ? iw : 0;
    const float v = x[c.boff + (ci * geo.H + ihc) * geo.W + iwc];
    return sel0(v, c.valid & kv & in);
  }
};

struct ConvFwdStore {
  float* y;  // [B, Co, OH, OW] (or a [split_k, ...] slab when slab_stride > 0)
  const float* bias;  // [Co] nullable
  int Co, OHOW;
  FastDiv d_ohow;
  bool accumulate;
  long slab_stride;   // 0: direct store; else per-split slab offset (numel)
  __device__ void store(int, int m, int n, float v, int ks) const {
    const unsigned b = d_ohow.div(n);
    const unsigned rem = d_ohow.mod(n, b);
    if (bias != nullptr && ks == 0) v += bias[m];
    float* p = y + (long)ks * slab_stride + ((long)b * Co + m) * OHOW + rem;
    if (accumulate) {
      atomicAdd(p, v);
    } else {
      *p = v;
    }
  }
};

// ---------------- backward data (direct stride-aware gather) ---------------
template <int CKH, int CKW, int CS>
struct ConvBwdDataGather {
  using G = Geo<CKH, CKW, CS>;
  const float* w;   // [Co, Ci, KH, KW]
  const float* gy;  // [B, Co, OH, OW]
  ConvGeom geo;

  struct KCtx {};
  __device__ KCtx prepK(int) const { return {}; }

  struct ACtx { int m; bool valid; };
  struct BCtx { int boff, ihp, iwp; bool valid; };

  __device__ ACtx prepA(int, int m, bool valid, int) const { return {m, valid}; }
  __device__ float loadA(const ACtx& c, const KCtx&, int k, bool kv) const {
    int co, kh, kw;
    G::dk(geo, k, co, kh, kw);
    const int khkw = G::kh_kw(geo);
    const float v = w[((long)co * geo.Ci + c.m) * khkw + kh * (G::fixed ? CKW : geo.KW) + kw];
    return sel0(v, c.valid & kv);
  }
  __device__ BCtx prepB(int, int n, bool valid, int) const {
    const unsigned b = geo.d_hw.div(n);
    const unsigned rem = geo.d_hw.mod(n, b);
    const unsigned ih = geo.d_w.div(rem);
    const unsigned iw = geo.d_w.mod(rem, ih);
    return {(int)((long)b * geo.Co * geo.OH * geo.OW),
            (int)ih + geo.pad, (int)iw + geo.pad, valid};
  }
  __device__ float loadB(const BCtx& c, const KCtx&, int k, bool kv) const {
    int co, kh, kw;
    G::dk(geo, k, co, kh, kw);
    const int s = G::stride(geo);
    const int oh_num = c.ihp - kh;
    const int ow_num = c.iwp - kw;
    int oh, ow;
    bool ok;
    if (s == 1) {
      oh = oh_num;
      ow = ow_num;
      ok = true;
    } else if (s == 2) {
      ok = ((oh_num | ow_num) & 1) == 0;
      oh = oh_num >> 1;
      ow = ow_num >> 1;
    } else if (s == 4) {
      ok = ((oh_num | ow_num) & 3) == 0;
      oh = oh_num >> 2;
      ow = ow_num >> 2;
    } else {
      ok = (oh_num % s) == 0 && (ow_num % s) == 0;
      oh = oh_num / s;
      ow = ow_num / s;
    }
    ok = ok && (unsigned)oh < (unsigned)geo.OH && (unsigned)ow < (unsigned)geo.OW;
    const int ohc = ok ? oh : 0;
    const int owc = ok ? ow : 0;
    const float v = gy[c.boff + (co * geo.OH + ohc) * geo.OW + owc];
    return sel0(v, c.valid & kv & ok);
  }
};

struct ConvBwdDataStore {
  float* gx;  // [B, Ci, H, W] (or slab)
  int Ci, HW;
  FastDiv d_hw;
  bool accumulate;
  long slab_stride;
  __device__ void store(int, int m, int n, float v, int ks) const {
    const unsigned b = d_hw.div(n);
    const unsigned rem = d_hw.mod(n, b);
    float* p = gx + (long)ks * slab_stride + ((long)b * Ci + m) * HW + rem;
    if (accumulate) {
      atomicAdd(p, v);
    } else {
      *p = v;
    }
  }
};

// ---------------- backward weight ------------------------------------------
// The gy A-side uses the prepK window hoist (fast flag).
template <int CKH, int CKW, int CS>
struct ConvBwdWeightGather {
  using G = Geo<CKH, CKW, CS>;
  const float* gy;  // [B, Co, OH, OW]
  const float* x;   // [B, Ci, H, W]
  ConvGeom geo;
  bool fast;        // OH*OW % 16 == 0: window-hoisted A addressing

  struct KCtx { int a_off; };
  __device__ KCtx prepK(int k0) const {
    if (!fast) return {0};
    const unsigned b0 = geo.d_ohow.div(k0);
    const unsigned rem0 = geo.d_ohow.mod(k0, b0);
    return {(int)((long)b0 * geo.Co * (geo.OH * geo.OW) + rem0)};
  }

  struct ACtx { int rowdk; int m; bool valid; };
  __device__ ACtx prepA(int, int m, bool valid, int dk) const {
    return {(int)((long)m * (geo.OH * geo.OW) + dk), m, valid};
  }
  __device__ float loadA(const ACtx& c, const KCtx& kc, int k, bool kv) const {
    float v;
    if (fast) {
      v = gy[c.rowdk + kc.a_off];  // per-lane hoisted row + per-tile scalar
    } else {
      const unsigned b = geo.d_ohow.div(k);
      const unsigned rem = geo.d_ohow.mod(k, b);
      v = gy[((long)b * geo.Co + c.m) * (geo.OH * geo.OW) + rem];
    }
    return sel0(v, c.valid & kv);
  }

  struct BCtx { int ciHW; short kh, kw; bool valid; };
  __device__ BCtx prepB(int, int n, bool valid, int) const {
    int ci, kh, kw;
    G::dk(geo, n, ci, kh, kw);
    return {ci * geo.H * geo.W, (short)kh, (short)kw, valid};
  }
  __device__ float loadB(const BCtx& c, const KCtx&, int k, bool kv) const {
    const unsigned b = geo.d_ohow.div(k);
    const unsigned rem = geo.d_ohow.mod(k, b);
    const unsigned oh = geo.d_ow.div(rem);
    const unsigned ow = geo.d_ow.mod(rem, oh);
    const int ih = (int)oh * G::stride(geo) - geo.pad + c.kh;
    const int iw = (int)ow * G::stride(geo) - geo.pad + c.kw;
    const bool in = (unsigned)ih < (unsigned)geo.H && (unsigned)iw < (unsigned)geo.W;
    const int ihc = in ? ih : 0;
    const int iwc = in ? iw : 0;
    const float v = x[(long)b * geo.Ci * geo.H * geo.W + c.ciHW
                      + ihc * geo.W + iwc];
    return sel0(v, c.valid & kv & in);
  }
};

struct AtomicStore {
  float* c;  // [M, N] contiguous (pre-zeroed when accumulate) or slab
  int N;
  bool accumulate;
  long slab_stride;
  __device__ void store(int, int m, int n, float v, int ks) const {
    float* p = c + (long)ks * slab_stride + (long)m * N + n;
    if (accumulate) {
      atomicAdd(p, v);
    } else {
      *p = v;
    }
  }
};

// ---------------- split-K slab finalize ------------------------------------
// out[i] = sum_s slab[s*numel + i]: replaces (zero + atomic accumulate) with
// streaming slab writes + one reduction pass — at split 64 on a 65 KB output
// the atomic path was 4M serialized RMWs.
// slab_reduce_body (common.h) forms each sum; a set whose length and bases
// allow it is summed four elements per thread with 16-byte loads
__device__ __forceinline__ void slab_reduce_set(const float* __restrict__ slab,
                                                int splits,
                                                float* __restrict__ out,
                                                long numel, bool vec4, int block,
                                                int nblocks) {
  if (vec4) {
    slab_reduce_body(reinterpret_cast<const f32x4*>(slab), splits,
                     reinterpret_cast<f32x4*>(out), numel / 4, block, nblocks);
  } else {
    slab_reduce_body(slab, splits, out, numel, block, nblocks);
  }
}

__global__ void slab_reduce_kernel(const float* __restrict__ slab, int splits,
                                   float* __restrict__ out, long numel,
                                   bool vec4) {
  slab_reduce_set(slab, splits, out, numel, vec4, blockIdx.x, gridDim.x);
}

// two independent slab sets in one launch (the gx and gw slabs of a paired
// conv backward): the first blocks_a blocks sum set a, the rest set b, each
// element as slab_reduce_kernel sums it
__global__ void slab_reduce_pair_kernel(const float* __restrict__ slab_a,
                                        int splits_a, float* __restrict__ out_a,
                                        long numel_a, bool vec4_a, int blocks_a,
                                        const float* __restrict__ slab_b,
                                        int splits_b, float* __restrict__ out_b,
                                        long numel_b, bool vec4_b) {
  if ((int)blockIdx.x < blocks_a) {
    slab_reduce_set(slab_a, splits_a, out_a, numel_a, vec4_a, blockIdx.x,
                    blocks_a);
  } else {
    slab_reduce_set(slab_b, splits_b, out_b, numel_b, vec4_b,
                    blockIdx.x - blocks_a, gridDim.x - blocks_a);
  }
}

// shared with wino.hip's ci-/tile-split slabs and gemm_f32.hip's split-K
// (declared in torch_util.h)
void slab_reduce(const float* slab, int splits, float* out, long numel,
                 hipStream_t stream) {
  hipLaunchKernelGGL(slab_reduce_kernel,
                     dim3(slab_reduce_grid(slab, out, numel)), dim3(256), 0,
                     stream, slab, splits, out, numel,
                     slab_is_vec4(slab, out, numel));
}

void slab_reduce_pair(const float* slab_a, int splits_a, float* out_a,
                      long numel_a, const float* slab_b, int splits_b,
                      float* out_b, long numel_b, hipStream_t stream) {
  const int blocks_a = slab_reduce_grid(slab_a, out_a, numel_a);   // 0 for an empty set
  const int blocks_b = slab_reduce_grid(slab_b, out_b, numel_b);
  if (blocks_a + blocks_b == 0) return;
  hipLaunchKernelGGL(slab_reduce_pair_kernel, dim3(blocks_a + blocks_b),
                     dim3(256), 0, stream, slab_a, splits_a, out_a, numel_a,
                     slab_is_vec4(slab_a, out_a, numel_a), blocks_a, slab_b,
                     splits_b, out_b, numel_b,
                     slab_is_vec4(slab_b, out_b, numel_b));
}

// slab mode threshold: slab stores beat atomics once MANY splits pile on
// one output; at mild splits (<8) the reduce pass's launch+ramp overhead
// loses slightly to cheap atomics (bench sweep, profiles/SUMMARY.md round 2).
// The default is still 3: atomic accumulation of three or more partial sums
// depends on arrival order, so results changed from run to run (two splits
// commute), and training amplifies that noise; slabs reduce in fixed order.
static inline int slab_min_splits() {
  static int v = [] {
    const char* e = std::getenv("SLK_SLAB_MIN");
    return e ? atoi(e) : 3;
  }();
  return v < 2 ? 2 : v;
}

// cap slab memory (splits * numel * 4B); above this stay with atomics — the
// reduce pass is traffic-proportional, and profiling shows big-output slabs
// (tens of MB) cost more in reduce than their atomics would
static constexpr long SLK_SLAB_MAX_BYTES = 32l << 20;

// ---------------- host wrappers ----------------

static ConvShape conv_shape(int B, int Ci, int H, int W, int Co, int KH, int KW,
                            int stride, int pad) {
  return {B, Ci, H, W, Co, KH, KW, stride, pad};
}

static ConvGeom make_geom(const ConvShape& s) {
  ConvGeom g;
  g.B = s.B; g.Ci = s.Ci; g.H = s.H; g.W = s.W; g.Co = s.Co; g.KH = s.KH;
  g.KW = s.KW; g.stride = s.stride; g.pad = s.pad;
  g.OH = s.OH();
  g.OW = s.OW();
  g.d_ohow.init(g.OH * g.OW);
  g.d_ow.init(g.OW);
  g.d_hw.init(g.H * g.W);
  g.d_w.init(g.W);
  g.d_khkw.init(g.KH * g.KW);
  g.d_kw.init(g.KW);
  return g;
}

// dispatch over the model zoo's conv geometries (stride/tap shape only; pad
// is runtime)
template <typename F>
static void dispatch_geom(const ConvGeom& g, F&& f) {
  if (g.KH == 3 && g.KW == 3 && g.stride == 1) {
    f(std::integral_constant<int, 0>{});  // 3x3 s1
  } else if (g.KH == 3 && g.KW == 3 && g.stride == 2) {
    f(std::integral_constant<int, 1>{});  // 3x3 s2
  } else if (g.KH == 1 && g.KW == 1 && g.stride == 1) {
    f(std::integral_constant<int, 2>{});  // 1x1
  } else if (g.KH == 4 && g.KW == 4 && g.stride == 4) {
    f(std::integral_constant<int, 3>{});  // ViT patch embed
  } else {
    f(std::integral_constant<int, 4>{});  // generic runtime geometry
  }
}

// the gather specialisation for dispatch_geom's case index
template <template <int, int, int> class Gather, int CASE>
using PickGather = std::tuple_element_t<
    CASE, std::tuple<Gather<3, 3, 1>, Gather<3, 3, 2>, Gather<1, 1, 1>,
                     Gather<4, 4, 4>, Gather<0, 0, 0>>>;

// split-K output plan: direct store (split 1), atomic accumulate (few
// splits), or per-split slab + reduce (many splits)
struct SplitPlan {
  int split_k;
  bool slab;
  at::Tensor buf;       // the tensor the GEMM writes (slab or the output)
  at::Tensor out;       // the real output
};

static SplitPlan plan_split(int split_k, at::IntArrayRef out_sizes,
                            const at::TensorOptions& opt) {
  SplitPlan p;
  p.split_k = split_k;
  long numel = 1;
  for (auto s : out_sizes) numel *= s;
  p.slab = split_k >= slab_min_splits() &&
           (long)split_k * numel * 4 <= SLK_SLAB_MAX_BYTES;
  if (p.slab) {
    p.out = at::empty(out_sizes, opt);
    std::vector<long> ss{p.split_k};
    for (auto s : out_sizes) ss.push_back(s);
    p.buf = at::empty(ss, opt);
  } else if (split_k > 1) {
    p.out = zeroed(out_sizes, opt);
    p.buf = p.out;
  } else {
    p.out = at::empty(out_sizes, opt);
    p.buf = p.out;
  }
  return p;
}

// The direct implicit-GEMM launch, shared by the three directions: pick the
// split, plan the output (store / atomics / slabs), launch the geometry's
// Gather{a, b, geo, extra...} and reduce the slabs.  make_store(buf,
// accumulate, slab_stride) returns the direction's store functor; its type is
// the kernel's Store parameter.  At split 1 a single block owns each output
// tile, so every direction (bwd-weight included) stores directly.
template <template <int, int, int> class Gather, typename MakeStore,
          typename... Extra>
static at::Tensor direct_gemm(const ConvGeom& geo, int M, int N, int K,
                              at::IntArrayRef out_sizes,
                              const at::TensorOptions& opt, const float* a,
                              const float* b, MakeStore make_store,
                              Extra... extra) {
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const int split_k = slk_effective_split(K, slk_pick_split_k(M, N, K, 1));
  auto plan = plan_split(split_k, out_sizes, opt);
  const auto st = make_store(plan.buf.data_ptr<float>(),
                             !plan.slab && split_k > 1,
                             plan.slab ? plan.out.numel() : 0);
  dispatch_geom(geo, [&](auto ic) {
    PickGather<Gather, decltype(ic)::value> g{a, b, geo, extra...};
    slk_launch_gemm(g, st, M, N, K, 1, split_k, stream);
  });
  if (plan.slab) {
    slab_reduce(plan.buf.data_ptr<float>(), split_k,
                plan.out.data_ptr<float>(), plan.out.numel(), stream);
  }
  return plan.out;
}

at::Tensor conv2d_fwd(const at::Tensor& x, const at::Tensor& w,
                      c10::optional<at::Tensor> bias, int stride, int pad) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && x.scalar_type() == at::kFloat);
  TORCH_CHECK(w.is_cuda() && w.dim() == 4 && w.size(1) == x.size(1));
  const ConvShape s = conv_shape(x.size(0), x.size(1), x.size(2), x.size(3),
                                 w.size(0), w.size(2), w.size(3), stride, pad);
  switch (route_fwd(s, wino_level())) {
    case ConvRoute::WinoFused:
      return conv2d_wino_fused(x, w, bias, pad, /*flip=*/false);
    case ConvRoute::Wino:
      return conv2d_wino(x, w, bias, pad, /*flip=*/false);
    default:
      break;
  }
  auto xc = x.contiguous();
  auto wc = w.contiguous();
  const ConvGeom geo = make_geom(s);
  const float* bp = bias.has_value() ? bias->data_ptr<float>() : nullptr;
  return direct_gemm<ConvFwdGather>(
      geo, geo.Co, geo.B * geo.OH * geo.OW, geo.Ci * geo.KH * geo.KW,
      {geo.B, geo.Co, geo.OH, geo.OW}, x.options(), wc.data_ptr<float>(),
      xc.data_ptr<float>(), [&](float* y, bool accumulate, long slab_stride) {
        return ConvFwdStore{y, bp, geo.Co, geo.OH * geo.OW, geo.d_ohow,
                            accumulate, slab_stride};
      });
}

at::Tensor conv2d_bwd_data(const at::Tensor& gy, const at::Tensor& w, int stride,
                           int pad, int H, int W) {
  TORCH_CHECK(gy.is_cuda() && gy.dim() == 4 && gy.scalar_type() == at::kFloat);
  const ConvShape s = conv_shape(gy.size(0), w.size(1), H, W, w.size(0),
                                 w.size(2), w.size(3), stride, pad);
  TORCH_CHECK(s.OH() == gy.size(2) && s.OW() == gy.size(3),
              "bwd-data geometry mismatch");
  // gx = winograd-conv of gy with rotated/transposed weights at pad' = 2-p
  switch (route_bwd_data(s, wino_level())) {
    case ConvRoute::WinoFused:
      return conv2d_wino_fused(gy, w, c10::nullopt, 2 - pad, /*flip=*/true);
    case ConvRoute::Wino:
      return conv2d_wino(gy, w, c10::nullopt, 2 - pad, /*flip=*/true);
    default:
      break;
  }
  auto gyc = gy.contiguous();
  auto wc = w.contiguous();
  const ConvGeom geo = make_geom(s);
  return direct_gemm<ConvBwdDataGather>(
      geo, geo.Ci, geo.B * H * W, geo.Co * geo.KH * geo.KW,
      {geo.B, geo.Ci, H, W}, gy.options(), wc.data_ptr<float>(),
      gyc.data_ptr<float>(), [&](float* gx, bool accumulate, long slab_stride) {
        return ConvBwdDataStore{gx, geo.Ci, H * W, geo.d_hw, accumulate,
                                slab_stride};
      });
}

at::Tensor conv2d_bwd_weight(const at::Tensor& gy, const at::Tensor& x, int KH,
                             int KW, int stride, int pad) {
  TORCH_CHECK(gy.is_cuda() && x.is_cuda() && gy.scalar_type() == at::kFloat);
  const ConvShape s = conv_shape(x.size(0), x.size(1), x.size(2), x.size(3),
                                 gy.size(1), KH, KW, stride, pad);
  TORCH_CHECK(s.OH() == gy.size(2) && s.OW() == gy.size(3),
              "bwd-weight geometry mismatch");
  switch (route_bwd_weight(s, wino_level())) {
    case ConvRoute::WinoBwdWFused:
      return conv2d_wino_bwdw_fused(gy, x, pad);
    case ConvRoute::WinoBwdW:
      return conv2d_wino_bwdw(gy, x, pad);
    default:
      break;
  }
  auto gyc = gy.contiguous();
  auto xc = x.contiguous();
  const ConvGeom geo = make_geom(s);
  const int N = geo.Ci * KH * KW;
  const bool fast = (geo.OH * geo.OW) % SLK_BK == 0;
  return direct_gemm<ConvBwdWeightGather>(
      geo, geo.Co, N, geo.B * geo.OH * geo.OW, {geo.Co, geo.Ci, KH, KW},
      gy.options(), gyc.data_ptr<float>(), xc.data_ptr<float>(),
      [&](float* gw, bool accumulate, long slab_stride) {
        return AtomicStore{gw, N, accumulate, slab_stride};
      },
      fast);
}

// both gradients of one conv layer.  The routes are conv_route.h's; where
// they are the two fused Winograd kernels, the pair is a way of LAUNCHING
// those two routes (wino_bwd_pair_kernel: one launch, the bits of the two),
// not a third route.  Every such pair is launched as one:
// all seven flagship shapes measured faster paired (B=32, us per layer,
// separate vs pair: 64ch 32x32 70.0 vs 62.7, 64->128 16x16 48.6 vs 38.9, 128ch
// 16x16 65.1 vs 51.4, 128->256 8x8 42.8 vs 34.0, 256ch 8x8 66.7 vs 51.1,
// 256->512 4x4 44.5 vs 31.0, 512ch 4x4 60.9 vs 45.1), so there is no win-set
// predicate.  An unwanted gradient comes back empty (None in Python).
std::tuple<c10::optional<at::Tensor>, c10::optional<at::Tensor>> conv2d_bwd(
    const at::Tensor& gy, const at::Tensor& x, const at::Tensor& w, int stride,
    int pad, bool need_gx, bool need_gw) {
  TORCH_CHECK(x.dim() == 4 && w.dim() == 4 && gy.dim() == 4);
  const int H = x.size(2), W = x.size(3), KH = w.size(2), KW = w.size(3);
  if (need_gx && need_gw) {
    const ConvShape s = conv_shape(x.size(0), x.size(1), H, W, w.size(0), KH,
                                   KW, stride, pad);
    if (s.OH() == gy.size(2) && s.OW() == gy.size(3) &&
        route_bwd_data(s, wino_level()) == ConvRoute::WinoFused &&
        route_bwd_weight(s, wino_level()) == ConvRoute::WinoBwdWFused) {
      auto r = conv2d_bwd_pair(gy, x, w, pad, -1);
      return {std::get<0>(r), std::get<1>(r)};
    }
  }
  c10::optional<at::Tensor> gx, gw;
  if (need_gx) gx = conv2d_bwd_data(gy, w, stride, pad, H, W);
  if (need_gw) gw = conv2d_bwd_weight(gy, x, KH, KW, stride, pad);
  return {gx, gw};
}

// which kernel the wrappers above would run for a conv shape, at this
// process's SLK_WINO level (launches nothing; tests pin the table with it)
std::string conv_route(const std::string& op, int B, int Ci, int H, int W,
                       int Co, int K, int stride, int pad) {
  const ConvShape s = conv_shape(B, Ci, H, W, Co, K, K, stride, pad);
  if (op == "fwd") return conv_route_name(route_fwd(s, wino_level()));
  if (op == "bwd_data") return conv_route_name(route_bwd_data(s, wino_level()));
  TORCH_CHECK(op == "bwd_weight", "conv_route: op must be fwd, bwd_data or "
              "bwd_weight, got ", op);
  return conv_route_name(route_bwd_weight(s, wino_level()));
}

// per-channel sum of gy over (B, OH, OW) -> conv bias gradient
// (chunk slabs + finalize reduce: no zero-init, no atomics)
__global__ void conv_bias_grad_kernel(const float* __restrict__ gy,
                                      float* __restrict__ slab, int B, int C,
                                      int HW) {
  __shared__ float scratch[16];
  const int c = blockIdx.x;
  const int total = B * HW;
  const int per = (total + gridDim.y - 1) / gridDim.y;
  const int lo = blockIdx.y * per;
  const int hi = min(total, lo + per);
  float acc = 0.f;
  for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    const int b = i / HW;
    const int r = i - b * HW;
    acc += gy[((long)b * C + c) * HW + r];
  }
  float total_s = slk_block_sum(acc, scratch);
  if (threadIdx.x == 0) slab[(long)blockIdx.y * C + c] = total_s;
}

__global__ void conv_bias_finalize_kernel(const float* __restrict__ slab,
                                          int chunks, float* __restrict__ gb,
                                          int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  for (int k = 0; k < chunks; ++k) s += slab[(long)k * C + c];
  gb[c] = s;
}

at::Tensor conv2d_bwd_bias(const at::Tensor& gy) {
  auto gyc = gy.contiguous();
  const int B = gy.size(0), C = gy.size(1), HW = gy.size(2) * gy.size(3);
  auto gb = at::empty({C}, gy.options());
  const int chunks = reduce_chunks((long)B * HW);
  auto slab = at::empty({chunks, C}, gy.options());
  auto stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(conv_bias_grad_kernel, dim3(C, (uint32_t)chunks), dim3(256),
                     0, stream, gyc.data_ptr<float>(), slab.data_ptr<float>(), B, C,
                     HW);
  hipLaunchKernelGGL(conv_bias_finalize_kernel, dim3(ceil_div(C, 256)), dim3(256),
                     0, stream, slab.data_ptr<float>(), chunks,
                     gb.data_ptr<float>(), C);
  return gb;
}

}  // namespace slk
