// Implicit-GEMM NCHW fp32 convolution on the MFMA tile framework.
//
// Forward:     y[Co, (B,OH,OW)] = W[Co, (Ci,KH,KW)] @ im2col(x)
// Bwd-data:    gx[Ci, (B,H,W)]  = W^T-gather @ col(gy)   (stride-aware)
// Bwd-weight:  gw[Co, (Ci,KH,KW)] = gy-gather @ im2col(x)^T
//
// Round-2 findings (profiles/, conv_microbench + PMC on MI355X):
// * the round-1 hypothesis "gathers are issue-bound" was WRONG at kernel
//   grain: a bounds-free pre-padded gather (SLK_CONV_PAD=1 path below) ties
//   the bounds-checked direct gather within noise (42.2 vs 42.7 us on
//   conv1_2) because the core is barrier/latency-paced, not VALU-bound —
//   while its pad/flipT prep kernels cost ~0.27 ms/step.  The DIRECT gather
//   is therefore the default; the padded path stays selectable for A/B as
//   the core gets faster.
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
#include <torch/extension.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include "tile_gemm.h"

namespace slk {

// empty + single fill-KERNEL launch instead of at::zeros (no aten dispatch;
// and never hipMemsetAsync — see slk_zero_async in common.h).
static inline at::Tensor zeroed(at::IntArrayRef sizes, const at::TensorOptions& opt) {
  auto t = at::empty(sizes, opt);
  slk_zero_async(t.data_ptr<float>(), t.numel(),
                 c10::hip::getCurrentHIPStream().stream());
  return t;
}

static inline bool conv_pad_mode() {
  static int v = [] {
    const char* e = std::getenv("SLK_CONV_PAD");
    return e ? atoi(e) : 0;
  }();
  return v != 0;
}

// wino.hip
at::Tensor conv2d_wino(const at::Tensor&, const at::Tensor&,
                       c10::optional<at::Tensor>, int, bool);
at::Tensor conv2d_wino_bwdw(const at::Tensor&, const at::Tensor&, int);
at::Tensor conv2d_wino_fused(const at::Tensor&, const at::Tensor&,
                             c10::optional<at::Tensor>, int, bool);
at::Tensor conv2d_wino_bwdw_fused(const at::Tensor&, const at::Tensor&, int);

// fused-Winograd eligibility: shape constraints + grid fill.  The fused
// kernel's base grid is (T/32) x (Cout/32); for FORWARD the measured
// win/lose line falls at >= 256 base blocks (1 per CU) — below it the
// ci-split can fill the grid but the forward still measured WORSE fused
// (8x8 tails: 52.4 vs 49.9 us), so forward keeps the 256 rule.
// BACKWARD-DATA additionally wins on the ci-split small-T tails and gets
// its own extension at the conv2d_bwd_data call site (profiles/SUMMARY.md).
static inline bool wino_fused_ok(int Cin, int Cout, int T, int OH, int OW) {
  static int v = [] {
    const char* e = std::getenv("SLK_WINO");
    return e ? atoi(e) : 1;
  }();
  if (v == 0) return false;
  if ((OH | OW) & 1) return false;
  if (Cout % 32 != 0 || T % 32 != 0 || Cin % 8 != 0) return false;
  if (v >= 3) return true;  // force: ci-split fills the grid (sweeps)
  return (long)(T / 32) * (Cout / 32) >= 256;
}

// Winograd routing (SLK_WINO=0 disables): F(2x2,3x3) beats the direct
// implicit-GEMM kernel on the MEASURED win set only — square channel counts
// at either end of the stack (64ch/32x32 and >=256ch tails); the 128ch
// middle loses to V/M HBM inflation (tools/wino_check.py table in
// profiles/SUMMARY.md).
static inline bool wino_env_on() {
  static int v = [] {
    const char* e = std::getenv("SLK_WINO");
    return e ? atoi(e) : 1;
  }();
  return v != 0;
}

static inline bool wino_wins_bwdw(int Ci, int Co, int H, int OH, int OW) {
  static int v = [] {
    const char* e = std::getenv("SLK_WINO");
    return e ? atoi(e) : 1;
  }();
  if (v == 0) return false;
  if ((OH | OW) & 1) return false;
  if (v >= 2) return true;
  // measured win set (tools/wino_check.py under SLK_WINO=0): square channel
  // counts win everywhere EXCEPT the 4x4 layers, where T = B*4 makes the
  // frequency GEMMs too small (512ch 4x4: 62 vs 48 us direct); the stem
  // (3ch 32x32) also wins mildly (44.9 vs 49.3 us) — its direct form is a
  // 9-n-tile tall-K pathology
  return (Ci == Co && H != 4) || (Ci <= 4 && H >= 32);
}

static inline bool wino_wins(int Ci, int Co, int H, int KH, int KW, int stride,
                             int OH, int OW) {
  static int v = [] {
    const char* e = std::getenv("SLK_WINO");
    return e ? atoi(e) : 1;
  }();
  if (v == 0 || KH != 3 || KW != 3 || stride != 1) return false;
  if ((OH | OW) & 1) return false;
  if (v >= 2) return true;  // force (sweeps)
  return Ci == Co && (Ci >= 256 || H >= 32);
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

// ---------------- forward: direct gather (default) ------------------------
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

// ---------------- forward: pre-padded bounds-free gather (SLK_CONV_PAD) ---
template <int CKH, int CKW, int CS>
struct ConvFwdGatherP {
  using G = Geo<CKH, CKW, CS>;
  const float* w;  // [Co, Ci, KH, KW] (or [Ci, Co, KHKW] flipT for bwd-data)
  const float* x;  // [B, Ci, Hp, Wp] pre-padded: every tap address in-bounds
  ConvGeom geo;    // H/W are the PADDED dims; geo.pad == 0

  struct KCtx {};
  __device__ KCtx prepK(int) const { return {}; }

  struct ACtx { const float* row; bool valid; };
  struct BCtx { const float* px; };

  __device__ ACtx prepA(int, int m, bool valid, int) const {
    return {w + (long)m * (geo.Ci * G::kh_kw(geo)), valid};
  }
  __device__ float loadA(const ACtx& c, const KCtx&, int k, bool kv) const {
    return sel0(c.row[k], c.valid & kv);
  }
  __device__ BCtx prepB(int, int n, bool, int) const {
    const unsigned b = geo.d_ohow.div(n);
    const unsigned rem = geo.d_ohow.mod(n, b);
    const unsigned oh = geo.d_ow.div(rem);
    const unsigned ow = geo.d_ow.mod(rem, oh);
    return {x + (long)b * geo.Ci * geo.H * geo.W
              + (long)(oh * G::stride(geo)) * geo.W + ow * G::stride(geo)};
  }
  __device__ float loadB(const BCtx& c, const KCtx&, int k, bool kv) const {
    int ci, kh, kw;
    G::dk(geo, k, ci, kh, kw);   // SALU (k wave-uniform)
    const int off = (ci * geo.H + kh) * geo.W + kw;
    return sel0(c.px[off], kv);
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
// Direct gather; the gy A-side uses the prepK window hoist (fast flag).
// PADDED=true additionally drops the x bounds math (SLK_CONV_PAD path).
template <int CKH, int CKW, int CS, bool PADDED>
struct ConvBwdWeightGather {
  using G = Geo<CKH, CKW, CS>;
  const float* gy;  // [B, Co, OH, OW]
  const float* x;   // [B, Ci, H, W] (padded dims when PADDED)
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
    if (PADDED) {
      const long sc = (long)b * geo.Ci * geo.H * geo.W
                    + (long)(oh * G::stride(geo)) * geo.W + ow * G::stride(geo);
      return sel0(x[c.ciHW + c.kh * geo.W + c.kw + sc], kv);
    }
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
__global__ void slab_reduce_kernel(const float* __restrict__ slab, int splits,
                                   float* __restrict__ out, long numel) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < numel;
       i += stride) {
    float s = 0.f;
    for (int k = 0; k < splits; ++k) s += slab[(long)k * numel + i];
    out[i] = s;
  }
}

static void slab_reduce(const at::Tensor& slab, int splits, at::Tensor& out,
                        hipStream_t stream) {
  const long numel = out.numel();
  const int grid = (int)std::min<long>((numel + 255) / 256, 4096);
  hipLaunchKernelGGL(slab_reduce_kernel, dim3(grid), dim3(256), 0, stream,
                     slab.data_ptr<float>(), splits, out.data_ptr<float>(),
                     numel);
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

// ---------------- padding / weight-flip prep kernels -----------------------

// x [BC, H, W] -> out [BC, H+2p, W+2p] zero-filled border, one coalesced
// pass: one blockIdx.y per (b, c) plane, blockIdx.x strides the padded plane
__global__ void pad_nchw_kernel(const float* __restrict__ x,
                                float* __restrict__ out, int H, int W, int p,
                                FastDiv d_wp) {
  const int Hp = H + 2 * p, Wp = W + 2 * p;
  const int plane = Hp * Wp;
  const float* __restrict__ xin = x + (long)blockIdx.y * H * W;
  float* __restrict__ po = out + (long)blockIdx.y * plane;
  const int stride = gridDim.x * blockDim.x;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < plane; i += stride) {
    const int hp = d_wp.div((unsigned)i);
    const int wp = d_wp.mod((unsigned)i, (unsigned)hp);
    const int ih = hp - p, iw = wp - p;
    const bool in = (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
    po[i] = in ? xin[ih * W + iw] : 0.f;
  }
}

// w [Co, Ci, KHKW] -> wt [Ci, Co, KHKW] with the tap index reversed
// (kh, kw) -> (KH-1-kh, KW-1-kw) == r -> KHKW-1-r; output-coalesced
__global__ void flipT_w_kernel(const float* __restrict__ w,
                               float* __restrict__ wt, int Co, int Ci, int KK) {
  const long total = (long)Co * Ci * KK;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    const int r = (int)(i % KK);
    const long t = i / KK;
    const int co = (int)(t % Co);
    const long ci = t / Co;
    wt[i] = w[((long)co * Ci + ci) * KK + (KK - 1 - r)];
  }
}

at::Tensor pad_nchw(const at::Tensor& x, int p) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && x.scalar_type() == at::kFloat);
  if (p == 0) return x.contiguous();
  auto xc = x.contiguous();
  const long BC = (long)x.size(0) * x.size(1);
  TORCH_CHECK(BC < 65536, "pad_nchw: B*C grid limit");
  const int H = x.size(2), W = x.size(3);
  auto out = at::empty({x.size(0), x.size(1), H + 2 * p, W + 2 * p}, x.options());
  FastDiv d_wp;
  d_wp.init(W + 2 * p);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const int plane = (H + 2 * p) * (W + 2 * p);
  const int gx = std::min(ceil_div(plane, 256), 16);
  hipLaunchKernelGGL(pad_nchw_kernel, dim3(gx, (uint32_t)BC), dim3(256), 0,
                     stream, xc.data_ptr<float>(), out.data_ptr<float>(), H, W,
                     p, d_wp);
  return out;
}

static at::Tensor flipT_w(const at::Tensor& w) {
  auto wc = w.contiguous();
  const int Co = w.size(0), Ci = w.size(1), KK = w.size(2) * w.size(3);
  auto wt = at::empty({Ci, Co, w.size(2), w.size(3)}, w.options());
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const long total = (long)Co * Ci * KK;
  const int grid = (int)std::min<long>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(flipT_w_kernel, dim3(grid), dim3(256), 0, stream,
                     wc.data_ptr<float>(), wt.data_ptr<float>(), Co, Ci, KK);
  return wt;
}

// ---------------- host wrappers ----------------

static ConvGeom make_geom(int B, int Ci, int H, int W, int Co, int KH, int KW,
                          int stride, int pad) {
  ConvGeom g;
  g.B = B; g.Ci = Ci; g.H = H; g.W = W; g.Co = Co; g.KH = KH; g.KW = KW;
  g.stride = stride; g.pad = pad;
  g.OH = (H + 2 * pad - KH) / stride + 1;
  g.OW = (W + 2 * pad - KW) / stride + 1;
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

template <template <int, int, int> class Gather, int CASE>
struct PickGather;
template <template <int, int, int> class Gather>
struct PickGather<Gather, 0> { using type = Gather<3, 3, 1>; };
template <template <int, int, int> class Gather>
struct PickGather<Gather, 1> { using type = Gather<3, 3, 2>; };
template <template <int, int, int> class Gather>
struct PickGather<Gather, 2> { using type = Gather<1, 1, 1>; };
template <template <int, int, int> class Gather>
struct PickGather<Gather, 3> { using type = Gather<4, 4, 4>; };
template <template <int, int, int> class Gather>
struct PickGather<Gather, 4> { using type = Gather<0, 0, 0>; };

// bwd-weight needs the extra PADDED axis
template <int A, int B, int C> using BwdWD = ConvBwdWeightGather<A, B, C, false>;
template <int A, int B, int C> using BwdWP = ConvBwdWeightGather<A, B, C, true>;

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

// x_is_padded: caller already ran pad_nchw (only meaningful under
// SLK_CONV_PAD=1, where functional.py saves x_pad from the forward)
at::Tensor conv2d_fwd(const at::Tensor& x, const at::Tensor& w,
                      c10::optional<at::Tensor> bias, int stride, int pad,
                      bool x_is_padded) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && x.scalar_type() == at::kFloat);
  TORCH_CHECK(w.is_cuda() && w.dim() == 4 && w.size(1) == x.size(1));
  if (!x_is_padded && !conv_pad_mode() && stride == 1 && w.size(2) == 3
      && w.size(3) == 3) {
    const int OHw = x.size(2) + 2 * pad - 2, OWw = x.size(3) + 2 * pad - 2;
    const int Tw = x.size(0) * (OHw / 2) * (OWw / 2);
    if (wino_fused_ok(x.size(1), w.size(0), Tw, OHw, OWw)) {
      return conv2d_wino_fused(x, w, bias, pad, /*flip=*/false);
    }
    if (wino_wins(x.size(1), w.size(0), x.size(2), 3, 3, 1, OHw, OWw)) {
      return conv2d_wino(x, w, bias, pad, /*flip=*/false);
    }
  }
  const bool padded = x_is_padded || conv_pad_mode();
  auto stream = c10::hip::getCurrentHIPStream().stream();
  auto wc = w.contiguous();

  at::Tensor xp = padded ? (x_is_padded ? x.contiguous() : pad_nchw(x, pad))
                         : x.contiguous();
  ConvGeom geo = padded
      ? make_geom(xp.size(0), xp.size(1), xp.size(2), xp.size(3), w.size(0),
                  w.size(2), w.size(3), stride, 0)
      : make_geom(x.size(0), x.size(1), x.size(2), x.size(3), w.size(0),
                  w.size(2), w.size(3), stride, pad);
  const int M = geo.Co, N = geo.B * geo.OH * geo.OW, K = geo.Ci * geo.KH * geo.KW;
  const int split_k = slk_effective_split(K, slk_pick_split_k(M, N, K, 1));
  auto plan = plan_split(split_k, {geo.B, geo.Co, geo.OH, geo.OW}, x.options());

  ConvFwdStore st{plan.buf.data_ptr<float>(),
                  bias.has_value() ? bias->data_ptr<float>() : nullptr,
                  geo.Co, geo.OH * geo.OW, geo.d_ohow,
                  !plan.slab && split_k > 1,
                  plan.slab ? plan.out.numel() : 0};
  dispatch_geom(geo, [&](auto ic) {
    if (padded) {
      using GT = typename PickGather<ConvFwdGatherP, decltype(ic)::value>::type;
      GT g{wc.data_ptr<float>(), xp.data_ptr<float>(), geo};
      slk_launch_gemm(g, st, M, N, K, 1, split_k, stream);
    } else {
      using GT = typename PickGather<ConvFwdGather, decltype(ic)::value>::type;
      GT g{wc.data_ptr<float>(), xp.data_ptr<float>(), geo};
      slk_launch_gemm(g, st, M, N, K, 1, split_k, stream);
    }
  });
  if (plan.slab) slab_reduce(plan.buf, split_k, plan.out, stream);
  return plan.out;
}

at::Tensor conv2d_bwd_data(const at::Tensor& gy, const at::Tensor& w, int stride,
                           int pad, int H, int W) {
  TORCH_CHECK(gy.is_cuda() && gy.dim() == 4 && gy.scalar_type() == at::kFloat);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const int KH = w.size(2), KW = w.size(3);
  const int Ci = w.size(1), Co = w.size(0);
  const int B = gy.size(0);
  // gx = winograd-conv of gy with rotated/transposed weights at pad' = 2-p
  if (stride == 1 && KH == 3 && KW == 3 && pad <= 2) {
    const int Tw = B * (H / 2) * (W / 2);
    bool fused = H % 2 == 0 && W % 2 == 0 && wino_fused_ok(Co, Ci, Tw, H, W);
    // backward-data ONLY: the ci-split fused kernel also wins on the
    // small-T high-channel tails (measured, 40-iter A/B under SLK_WINO=3:
    // 256ch 8x8 44.6 vs 49.3 us, 256->512 4x4 31.6 vs 38.1, 512ch 4x4 45.3
    // vs 49.9; the 2x2 layers lose 62 vs 35 and stay out).  Forward at the
    // same shapes measured WORSE fused and keeps the >=256-block rule.
    if (!fused && H % 2 == 0 && W % 2 == 0 && H >= 4 && Ci >= 64
        && Ci % 32 == 0 && Co % 8 == 0 && Tw % 32 == 0
        && (long)(Tw / 32) * (Ci / 32) >= 32 && wino_env_on()) {
      fused = true;  // Ci >= 64: measured down to 64ch gx (24.4 vs 37.0 us)
    }
    if (fused) {
      return conv2d_wino_fused(gy, w, c10::nullopt, 2 - pad, /*flip=*/true);
    }
    if (wino_wins(Co, Ci, gy.size(2), 3, 3, 1, H, W)) {
      return conv2d_wino(gy, w, c10::nullopt, 2 - pad, /*flip=*/true);
    }
  }

  if (conv_pad_mode() && stride == 1 && KH == KW && pad <= KH - 1) {
    // gx = valid-conv(pad(gy, K-1-p), flipT(w)): bounds-free forward gather.
    // Derivation: y[oh] sums x[oh - p + kh] => gx[ih] = sum_kh gy[ih + p - kh]
    // = sum_kh' gy_pad[ih + kh'] with kh' = KH-1-kh and pad q = KH-1-p.
    auto wt = flipT_w(w);
    const int q = KH - 1 - pad;
    auto gyp = pad_nchw(gy, q);
    ConvGeom geo = make_geom(B, Co, gyp.size(2), gyp.size(3), Ci, KH, KW, 1, 0);
    TORCH_CHECK(geo.OH == H && geo.OW == W, "bwd-data geometry mismatch");
    const int M = Ci, N = B * H * W, K = Co * KH * KW;
    const int split_k = slk_effective_split(K, slk_pick_split_k(M, N, K, 1));
    auto plan = plan_split(split_k, {B, Ci, H, W}, gy.options());
    ConvFwdStore st{plan.buf.data_ptr<float>(), nullptr, Ci, H * W, geo.d_ohow,
                    !plan.slab && split_k > 1, plan.slab ? plan.out.numel() : 0};
    dispatch_geom(geo, [&](auto ic) {
      using GT = typename PickGather<ConvFwdGatherP, decltype(ic)::value>::type;
      GT g{wt.data_ptr<float>(), gyp.data_ptr<float>(), geo};
      slk_launch_gemm(g, st, M, N, K, 1, split_k, stream);
    });
    if (plan.slab) slab_reduce(plan.buf, split_k, plan.out, stream);
    return plan.out;
  }

  auto gyc = gy.contiguous();
  auto wc = w.contiguous();
  ConvGeom geo = make_geom(B, Ci, H, W, Co, KH, KW, stride, pad);
  TORCH_CHECK(geo.OH == gy.size(2) && geo.OW == gy.size(3),
              "bwd-data geometry mismatch");
  const int M = geo.Ci, N = geo.B * H * W, K = geo.Co * KH * KW;
  const int split_k = slk_effective_split(K, slk_pick_split_k(M, N, K, 1));
  auto plan = plan_split(split_k, {B, Ci, H, W}, gy.options());
  ConvBwdDataStore st{plan.buf.data_ptr<float>(), geo.Ci, H * W, geo.d_hw,
                      !plan.slab && split_k > 1,
                      plan.slab ? plan.out.numel() : 0};
  dispatch_geom(geo, [&](auto ic) {
    using GT = typename PickGather<ConvBwdDataGather, decltype(ic)::value>::type;
    GT g{wc.data_ptr<float>(), gyc.data_ptr<float>(), geo};
    slk_launch_gemm(g, st, M, N, K, 1, split_k, stream);
  });
  if (plan.slab) slab_reduce(plan.buf, split_k, plan.out, stream);
  return plan.out;
}

at::Tensor conv2d_bwd_weight(const at::Tensor& gy, const at::Tensor& x, int KH,
                             int KW, int stride, int pad, bool x_is_padded) {
  TORCH_CHECK(gy.is_cuda() && x.is_cuda() && gy.scalar_type() == at::kFloat);
  // Winograd weight-gradient.  FUSED twin first (in-kernel transforms,
  // tile-axis reduction with per-slice slabs): measured faster than every
  // alternative on ALL eligible shapes — 512ch 2x2: 13.2 us vs 29.1 routed,
  // 512ch 4x4: 36.2 vs 48.2, 64->128: 33.5 vs 45.9 (profiles/SUMMARY.md).
  // The transform+frequency-GEMM pipeline (conv2d_wino_bwdw) remains for
  // Ci/Co not multiples of 32.
  if (!x_is_padded && !conv_pad_mode() && stride == 1 && KH == 3 && KW == 3
      && pad <= 2 && gy.size(2) % 2 == 0 && gy.size(3) % 2 == 0) {
    static int wv = [] {
      const char* e = std::getenv("SLK_WINO");
      return e ? atoi(e) : 1;
    }();
    if (wv != 0 && x.size(1) % 32 == 0 && gy.size(1) % 32 == 0) {
      return conv2d_wino_bwdw_fused(gy, x, pad);
    }
    if (wino_wins_bwdw(x.size(1), gy.size(1), x.size(2), gy.size(2),
                       gy.size(3))) {
      return conv2d_wino_bwdw(gy, x, pad);
    }
  }
  const bool padded = x_is_padded || conv_pad_mode();
  auto gyc = gy.contiguous();
  auto stream = c10::hip::getCurrentHIPStream().stream();

  at::Tensor xp = padded ? (x_is_padded ? x.contiguous() : pad_nchw(x, pad))
                         : x.contiguous();
  ConvGeom geo = padded
      ? make_geom(xp.size(0), xp.size(1), xp.size(2), xp.size(3), gy.size(1),
                  KH, KW, stride, 0)
      : make_geom(x.size(0), x.size(1), x.size(2), x.size(3), gy.size(1),
                  KH, KW, stride, pad);
  TORCH_CHECK(geo.OH == gy.size(2) && geo.OW == gy.size(3),
              "bwd-weight geometry mismatch");
  const int M = geo.Co, N = geo.Ci * KH * KW, K = geo.B * geo.OH * geo.OW;
  const int split_k = slk_effective_split(K, slk_pick_split_k(M, N, K, 1));
  auto plan = plan_split(split_k, {geo.Co, geo.Ci, KH, KW}, gy.options());
  // bwd-weight always accumulates over K even at split 1 unless slab? No:
  // at split 1 a single block owns each output tile -> direct store is fine.
  AtomicStore st{plan.buf.data_ptr<float>(), N, !plan.slab && split_k > 1,
                 plan.slab ? plan.out.numel() : 0};
  const bool fast = (geo.OH * geo.OW) % SLK_BK == 0;
  dispatch_geom(geo, [&](auto ic) {
    if (padded) {
      using GT = typename PickGather<BwdWP, decltype(ic)::value>::type;
      GT g{gyc.data_ptr<float>(), xp.data_ptr<float>(), geo, fast};
      slk_launch_gemm(g, st, M, N, K, 1, split_k, stream);
    } else {
      using GT = typename PickGather<BwdWD, decltype(ic)::value>::type;
      GT g{gyc.data_ptr<float>(), xp.data_ptr<float>(), geo, fast};
      slk_launch_gemm(g, st, M, N, K, 1, split_k, stream);
    }
  });
  if (plan.slab) slab_reduce(plan.buf, split_k, plan.out, stream);
  return plan.out;
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
  long chunks = ((long)B * HW) / 4096;
  if (chunks < 1) chunks = 1;
  if (chunks > 16) chunks = 16;
  auto slab = at::empty({chunks, C}, gy.options());
  auto stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(conv_bias_grad_kernel, dim3(C, (uint32_t)chunks), dim3(256),
                     0, stream, gyc.data_ptr<float>(), slab.data_ptr<float>(), B, C,
                     HW);
  hipLaunchKernelGGL(conv_bias_finalize_kernel, dim3(ceil_div(C, 256)), dim3(256),
                     0, stream, slab.data_ptr<float>(), (int)chunks,
                     gb.data_ptr<float>(), C);
  return gb;
}

}  // namespace slk
