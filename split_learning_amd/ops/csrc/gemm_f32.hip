// Strided/batched fp32 MFMA GEMM + Linear forward + column-sum.
// Serves Linear fwd/bwd (reference nn.Linear sites: src/model/VGG16_CIFAR10.py:107-117),
// attention QK^T / PV batched matmuls (src/model/BERT_AGNEWS.py:66-74), and
// LoRA adapters.  Transposes are handled by stride swaps — no data movement.
#include "tile_gemm.h"
#include "torch_util.h"

namespace slk {

struct StridedGather {
  const float* A;
  const float* B;
  long sAb, sAm, sAk;
  long sBb, sBk, sBn;

  // Contexts hold 32-bit OFFSETS against the functor's uniform (SGPR) base
  // pointers rather than per-context 64-bit pointers: the big-tile kernel
  // keeps 8 A-contexts live and the pointer form cost 16 VGPR of its
  // register budget (the 128x128 kernel sat at 3 waves/SIMD; see
  // tile_gemm.h).  Host guards numel < 2^31 (matmul_f32).
  struct KCtx {};
  struct ACtx { int off; bool valid; };
  struct BCtx { int off; bool valid; };

  __device__ KCtx prepK(int) const { return {}; }
  __device__ ACtx prepA(int b, int m, bool valid, int) const {
    return {(int)((long)b * sAb + (long)m * sAm), valid};
  }
  __device__ float loadA(const ACtx& c, const KCtx&, int k, bool kv) const {
    const float v = A[c.off + (long)k * sAk];
    return (c.valid & kv) ? v : 0.f;
  }
  __device__ BCtx prepB(int b, int n, bool valid, int) const {
    return {(int)((long)b * sBb + (long)n * sBn), valid};
  }
  __device__ float loadB(const BCtx& c, const KCtx&, int k, bool kv) const {
    const float v = B[c.off + (long)k * sBk];
    return (c.valid & kv) ? v : 0.f;
  }
};

struct StridedStore {
  float* C;
  long sCb;
  int N;
  const float* bias;  // per-column bias (nullable)
  bool accumulate;    // atomic accumulate into C (beta=1; one add per element)
  long slab_stride;   // > 0: split ks stores into its own slab (no atomics)
  __device__ void store(int b, int m, int n, float v, int ks) const {
    float* p = C + (long)ks * slab_stride + (long)b * sCb + (long)m * N + n;
    if (bias != nullptr && ks == 0) v += bias[n];
    if (accumulate) {
      atomicAdd(p, v);
    } else {
      *p = v;
    }
  }
};

// split-K partial sums are added by slab_reduce (conv2d.hip) in fixed slab
// order, the same way every run (atomic accumulation is order-dependent for
// three or more splits, and training amplifies that rounding noise)

// split_k > 1: every split writes its own slab, reduced into c afterwards —
// or, with keep_slabs, handed back unreduced as [splits * numel(c)] for a
// consumer that sums them itself (c is then left untouched)
static void launch_strided(const at::Tensor& a2, const at::Tensor& b2, at::Tensor& c,
                           bool ta, bool tb, const c10::optional<at::Tensor>& bias,
                           bool accumulate, int split_k,
                           at::Tensor* keep_slabs = nullptr) {
  const bool batched = a2.dim() == 3;
  const int nb = batched ? a2.size(0) : 1;
  const int M = ta ? a2.size(-1) : a2.size(-2);
  const int K = ta ? a2.size(-2) : a2.size(-1);
  const int N = tb ? b2.size(-2) : b2.size(-1);

  StridedGather g;
  g.A = a2.data_ptr<float>();
  g.B = b2.data_ptr<float>();
  g.sAb = batched ? a2.stride(0) : 0;
  g.sAm = ta ? a2.stride(-1) : a2.stride(-2);
  g.sAk = ta ? a2.stride(-2) : a2.stride(-1);
  g.sBb = (b2.dim() == 3) ? b2.stride(0) : 0;
  g.sBk = tb ? b2.stride(-1) : b2.stride(-2);
  g.sBn = tb ? b2.stride(-2) : b2.stride(-1);

  auto stream = c10::hip::getCurrentHIPStream().stream();
  // the launcher BK-aligns the split: size the slab by the effective count
  split_k = slk_effective_split(K, split_k);
  TORCH_CHECK(!(accumulate && split_k > 1), "split-K cannot accumulate into C");
  const long numel = (long)nb * M * N;
  at::Tensor slab;
  if (split_k > 1) slab = at::empty({(long)split_k * numel}, c.options());

  StridedStore st;
  st.C = split_k > 1 ? slab.data_ptr<float>() : c.data_ptr<float>();
  st.sCb = batched ? (long)M * N : 0;
  st.N = N;
  st.bias = bias.has_value() ? bias->data_ptr<float>() : nullptr;
  st.accumulate = accumulate;
  st.slab_stride = split_k > 1 ? numel : 0;

  slk_launch_gemm(g, st, M, N, K, nb, split_k, stream, slk_use_big(M, N));
  if (split_k > 1 && keep_slabs != nullptr) {
    *keep_slabs = slab;
  } else if (split_k > 1) {
    slab_reduce(slab.data_ptr<float>(), split_k, c.data_ptr<float>(), numel,
                stream);
  }
}

at::Tensor matmul_f32(const at::Tensor& a, const at::Tensor& b, bool ta, bool tb,
                      c10::optional<at::Tensor> out, bool accumulate) {
  TORCH_CHECK(a.is_cuda() && b.is_cuda(), "matmul_f32: GPU tensors required");
  TORCH_CHECK(a.scalar_type() == at::kFloat && b.scalar_type() == at::kFloat,
              "matmul_f32 is fp32-only");
  TORCH_CHECK(a.dim() == b.dim() && (a.dim() == 2 || a.dim() == 3),
              "matmul_f32: 2-D or 3-D tensors, same rank");
  TORCH_CHECK(a.numel() < (1ll << 31) && b.numel() < (1ll << 31),
              "matmul_f32: int32 gather offsets (tensor too large)");
  const int M = ta ? a.size(-1) : a.size(-2);
  const int Ka = ta ? a.size(-2) : a.size(-1);
  const int Kb = tb ? b.size(-1) : b.size(-2);
  const int N = tb ? b.size(-2) : b.size(-1);
  TORCH_CHECK(Ka == Kb, "matmul_f32: inner dims mismatch ", Ka, " vs ", Kb);
  if (a.dim() == 3) TORCH_CHECK(a.size(0) == b.size(0), "batch mismatch");

  at::Tensor c;
  if (out.has_value()) {
    c = *out;
  } else {
    c = a.dim() == 3 ? at::empty({a.size(0), M, N}, a.options())
                     : at::empty({M, N}, a.options());
  }
  int split_k = 1;
  if (!accumulate && !out.has_value()) {
    const int bm = slk_use_big(M, N) ? SLK_BM2 : SLK_BM;
    const int bn = slk_use_big(M, N) ? SLK_BN2 : SLK_BN;
    split_k = slk_pick_split_k(M, N, Ka, a.dim() == 3 ? a.size(0) : 1, bm, bn);
  }
  launch_strided(a, b, c, ta, tb, c10::nullopt, accumulate, split_k);
  return c;
}

// slabs matmul_f32 splits a fresh [nb, M, K] @ [nb, K, N] into (1: no split)
int matmul_f32_slab_count(int nb, int M, int N, int K) {
  const bool big = slk_use_big(M, N);
  return slk_effective_split(
      K, slk_pick_split_k(M, N, K, nb, big ? SLK_BM2 : SLK_BM,
                          big ? SLK_BN2 : SLK_BN));
}

// Batched a @ b (3-D, no transposes) with matmul_f32's split-K choice, the
// slabs left unreduced: returns [splits, nb, M, N], of which the caller adds
// slab 0, 1, ... in order as slab_reduce would.  The Winograd
// output transform takes its M this way (wino.hip).
at::Tensor matmul_f32_slabs(const at::Tensor& a, const at::Tensor& b) {
  TORCH_CHECK(a.is_cuda() && b.is_cuda() && a.dim() == 3 && b.dim() == 3 &&
              a.scalar_type() == at::kFloat && b.scalar_type() == at::kFloat,
              "matmul_f32_slabs: 3-D fp32 GPU tensors");
  TORCH_CHECK(a.numel() < (1ll << 31) && b.numel() < (1ll << 31),
              "matmul_f32_slabs: int32 gather offsets (tensor too large)");
  TORCH_CHECK(a.size(0) == b.size(0) && a.size(2) == b.size(1),
              "matmul_f32_slabs: shape mismatch");
  const int nb = a.size(0), M = a.size(1), K = a.size(2), N = b.size(2);
  // the effective count: launch_strided maps it onto itself
  const int split_k = matmul_f32_slab_count(nb, M, N, K);
  at::Tensor c, slabs;
  if (split_k == 1) c = at::empty({1, nb, M, N}, a.options());
  else c = at::empty({0}, a.options());   // options carrier only
  launch_strided(a, b, c, false, false, c10::nullopt, false, split_k, &slabs);
  if (!slabs.defined()) return c;
  return slabs.view({-1, nb, M, N});
}

at::Tensor linear_fwd(const at::Tensor& x, const at::Tensor& w,
                      c10::optional<at::Tensor> bias) {
  // y[M,N] = x[M,K] @ w[N,K]^T + b; split-K when the tile grid underfills the
  // chip (batch-32 rows = 1 M-tile: the 4096->10 classifier is ONE tile).
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat, "linear_fwd: fp32 GPU");
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kFloat,
              "linear_fwd: weight must be a fp32 GPU tensor (got device ",
              w.device(), ")");
  TORCH_CHECK(!bias.has_value() || bias->is_cuda(), "linear_fwd: bias device");
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && x.size(1) == w.size(1));
  const int M = x.size(0), N = w.size(0), K = x.size(1);
  const bool big = slk_use_big(M, N);
  int split_k = slk_pick_split_k(M, N, K, 1, big ? SLK_BM2 : SLK_BM,
                                 big ? SLK_BN2 : SLK_BN);
  auto y = at::empty({M, N}, x.options());
  launch_strided(x, w, y, /*ta=*/false, /*tb=*/true, bias, /*acc=*/false, split_k);
  return y;
}

// column sum of a [M,N] matrix -> [N] (Linear bias gradient)
__global__ void colsum_kernel(const float* __restrict__ x, float* __restrict__ out,
                              int M, int N) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float acc = 0.f;
  for (int m = 0; m < M; ++m) acc += x[(long)m * N + n];
  out[n] = acc;
}

at::Tensor colsum_f32(const at::Tensor& x) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.scalar_type() == at::kFloat);
  auto xc = x.contiguous();
  auto out = at::empty({x.size(1)}, x.options());
  int N = x.size(1);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(colsum_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, stream,
                     xc.data_ptr<float>(), out.data_ptr<float>(), x.size(0), N);
  return out;
}

}  // namespace slk
