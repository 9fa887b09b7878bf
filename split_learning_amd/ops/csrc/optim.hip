// Fused optimizer updates (SGD+momentum, AdamW), exact torch.optim semantics
// (reference optimizer sites: src/train/VGG16.py:62 SGD(lr, momentum);
// src/train/BERT.py:69 / KWT.py:62 AdamW(lr, weight_decay)).
// The C++ wrapper loops tensors and launches one elementwise kernel per tensor;
// per-microbatch step capture into a hipGraph absorbs the launch overhead.
#include <torch/extension.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include "common.h"

namespace slk {

// zero_after: clears the gradient after applying it, replacing the per-tensor
// zero_grad fill kernels (autograd then accumulates the next microbatch's
// gradients into already-zeroed buffers).
__global__ void sgd_kernel(float* __restrict__ p, float* __restrict__ g,
                           float* __restrict__ buf, long n, float lr, float momentum,
                           float weight_decay, bool first, bool zero_after) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float grad = g[i];
    if (zero_after) g[i] = 0.f;
    if (weight_decay != 0.f) grad += weight_decay * p[i];
    float b;
    if (momentum != 0.f) {
      b = first ? grad : momentum * buf[i] + grad;  // torch dampening=0
      buf[i] = b;
    } else {
      b = grad;
    }
    p[i] -= lr * b;
  }
}

// AdamW's derived coefficients, formed on the host in double: in float,
// 1.f - 0.999f is 1.3e-5 (relative) away from 1 - 0.999, and exp_avg_sq
// carried that factor.
struct AdamCoef {
  float omb1, omb2;  // 1 - beta
  float bc1, bc2;    // 1 - beta^step
};

static inline AdamCoef adam_coef(double beta1, double beta2, int64_t step) {
  return {(float)(1.0 - beta1), (float)(1.0 - beta2),
          (float)(1.0 - std::pow(beta1, (double)step)),
          (float)(1.0 - std::pow(beta2, (double)step))};
}

__global__ void adamw_kernel(float* __restrict__ p, float* __restrict__ g,
                             float* __restrict__ m, float* __restrict__ v, long n,
                             float lr, float beta1, float beta2, float eps,
                             float weight_decay, AdamCoef k,
                             bool zero_after) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    // decoupled weight decay (AdamW): p *= (1 - lr*wd)
    float pv = p[i] * (1.f - lr * weight_decay);
    const float grad = g[i];
    if (zero_after) g[i] = 0.f;
    const float mi = beta1 * m[i] + k.omb1 * grad;
    const float vi = beta2 * v[i] + k.omb2 * grad * grad;
    m[i] = mi;
    v[i] = vi;
    const float mhat = mi / k.bc1;
    const float vhat = vi / k.bc2;
    p[i] = pv - lr * mhat / (sqrtf(vhat) + eps);
  }
}

static inline int opt_grid(long n) {
  return (int)std::min<long>((n + 255) / 256, 2048);
}

// ---- fully fused multi-tensor path: ONE launch per optimizer step ----
// desc layout (int64, device): [prefix(n+1) | numel(n) | p(n) | g(n) | b1(n) | b2(n)]
// prefix[t] = first chunk index of tensor t; CHUNK elements per block.
constexpr long SLK_OPT_CHUNK = 16384;

__device__ __forceinline__ int find_tensor(const long* prefix, int n, long chunk) {
  int lo = 0, hi = n;  // prefix[t] <= chunk < prefix[t+1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= chunk) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- gradient-norm clipping (torch.nn.utils.clip_grad_norm_, norm_type 2) ----
// Two small launches in front of the fused step: per-chunk sums of squares in
// double (the product of two floats is exact there, and 1e25-sized gradients
// do not overflow as torch's fp32 sum does), then one block that turns them
// into out[0] = total norm, out[1] = clip coefficient.  The fused step reads
// out[1] and scales each gradient as it loads it; no scaling pass exists.
// No atomics and a fixed reduction order: the same gradients give the same bits.

__global__ void grad_sumsq_fused_kernel(const long* __restrict__ desc, int n,
                                        double* __restrict__ partial) {
  __shared__ double red[4];
  const long* prefix = desc;
  const long* numels = desc + (n + 1);
  const long* gp = numels + 2 * n;
  const int t = find_tensor(prefix, n, blockIdx.x);
  const long base = ((long)blockIdx.x - prefix[t]) * SLK_OPT_CHUNK;
  const long end = min(base + SLK_OPT_CHUNK, numels[t]);
  const float* g = (const float*)gp[t];
  double s = 0.0;
  // same float4 body + scalar tail (and alignment) as sgd_fused_kernel
  const long end4 = base + ((end - base) & ~3L);
  for (long i = base + (long)threadIdx.x * 4; i < end4; i += (long)blockDim.x * 4) {
    const float4 gv = *(const float4*)(g + i);
    s += (double)gv.x * (double)gv.x;
    s += (double)gv.y * (double)gv.y;
    s += (double)gv.z * (double)gv.z;
    s += (double)gv.w * (double)gv.w;
  }
  for (long i = end4 + threadIdx.x; i < end; i += blockDim.x)
    s += (double)g[i] * (double)g[i];
  // shuffle tree inside each 64-lane wave, then the four wave sums through LDS
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void grad_clip_coef_kernel(const double* __restrict__ partial,
                                      long chunks, double max_norm,
                                      float* __restrict__ out) {
  __shared__ double red[256];
  double s = 0.0;
  for (long i = threadIdx.x; i < chunks; i += blockDim.x) s += partial[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double norm = sqrt(red[0]);
    const double coef = max_norm / (norm + 1e-6);
    out[0] = (float)norm;
    // not fmin: a NaN norm must stay a NaN coefficient (torch.clamp keeps it)
    out[1] = (float)(coef > 1.0 ? 1.0 : coef);
  }
}

// The clipped gradient, rounded to float before anything else uses it (as
// torch's in-place g.mul_(coef) is): kept out of fma contraction with the
// weight-decay / moment arithmetic that follows.
__device__ __forceinline__ float scale_grad(float g, float coef) {
#pragma clang fp contract(off)
  return g * coef;
}

__global__ void sgd_fused_kernel(const long* __restrict__ desc, int n, float lr,
                                 float momentum, float weight_decay, bool first,
                                 bool zero_after,
                                 const float* __restrict__ grad_scale) {
  const long* prefix = desc;
  const long* numels = desc + (n + 1);
  const long* pp = numels + n;
  const long* gp = pp + n;
  const long* bp = gp + n;
  const int t = find_tensor(prefix, n, blockIdx.x);
  const long base = ((long)blockIdx.x - prefix[t]) * SLK_OPT_CHUNK;
  const long ne = numels[t];
  const long end = min(base + SLK_OPT_CHUNK, ne);
  float* p = (float*)pp[t];
  float* g = (float*)gp[t];
  float* buf = (float*)bp[t];
  const bool clip = grad_scale != nullptr;
  const float coef = clip ? grad_scale[1] : 1.f;
  auto upd = [&](float pv, float gv, float bv, float& po, float& bo) {
    if (clip) gv = scale_grad(gv, coef);
    if (weight_decay != 0.f) gv += weight_decay * pv;
    float b = (momentum != 0.f) ? (first ? gv : momentum * bv + gv) : gv;
    bo = b;
    po = pv - lr * b;
  };
  // float4 main body (chunk bases are 16384-element aligned; torch GPU
  // allocations are >=256B aligned) + scalar tail
  const long end4 = base + ((end - base) & ~3L);
  for (long i = base + (long)threadIdx.x * 4; i < end4; i += (long)blockDim.x * 4) {
    float4 pv = *(float4*)(p + i);
    float4 gv = *(float4*)(g + i);
    float4 bv = momentum != 0.f ? *(float4*)(buf + i) : float4{0, 0, 0, 0};
    float4 po, bo;
    upd(pv.x, gv.x, bv.x, po.x, bo.x);
    upd(pv.y, gv.y, bv.y, po.y, bo.y);
    upd(pv.z, gv.z, bv.z, po.z, bo.z);
    upd(pv.w, gv.w, bv.w, po.w, bo.w);
    *(float4*)(p + i) = po;
    if (momentum != 0.f) *(float4*)(buf + i) = bo;
    if (zero_after) *(float4*)(g + i) = float4{0, 0, 0, 0};
  }
  for (long i = end4 + threadIdx.x; i < end; i += blockDim.x) {
    float po, bo;
    upd(p[i], g[i], momentum != 0.f ? buf[i] : 0.f, po, bo);
    p[i] = po;
    if (momentum != 0.f) buf[i] = bo;
    if (zero_after) g[i] = 0.f;
  }
}

__global__ void adamw_fused_kernel(const long* __restrict__ desc, int n, float lr,
                                   float beta1, float beta2, float eps,
                                   float weight_decay, AdamCoef k,
                                   bool zero_after,
                                   const float* __restrict__ grad_scale) {
  // (scalar loop: AdamW tensors in this zoo are small; the SGD path above is
  // the hot one and is vectorized)
  const long* prefix = desc;
  const long* numels = desc + (n + 1);
  const long* pp = numels + n;
  const long* gp = pp + n;
  const long* mp = gp + n;
  const long* vp = mp + n;
  const int t = find_tensor(prefix, n, blockIdx.x);
  const long base = ((long)blockIdx.x - prefix[t]) * SLK_OPT_CHUNK;
  const long end = min(base + SLK_OPT_CHUNK, numels[t]);
  float* p = (float*)pp[t];
  float* g = (float*)gp[t];
  float* m = (float*)mp[t];
  float* v = (float*)vp[t];
  const bool clip = grad_scale != nullptr;
  const float coef = clip ? grad_scale[1] : 1.f;
  for (long i = base + threadIdx.x; i < end; i += blockDim.x) {
    float pv = p[i] * (1.f - lr * weight_decay);
    float grad = g[i];
    if (clip) grad = scale_grad(grad, coef);
    if (zero_after) g[i] = 0.f;
    const float mi = beta1 * m[i] + k.omb1 * grad;
    const float vi = beta2 * v[i] + k.omb2 * grad * grad;
    m[i] = mi;
    v[i] = vi;
    p[i] = pv - lr * (mi / k.bc1) / (sqrtf(vi / k.bc2) + eps);
  }
}

at::Tensor make_opt_desc(std::vector<at::Tensor> params,
                         std::vector<at::Tensor> grads,
                         std::vector<at::Tensor> s1,
                         std::vector<at::Tensor> s2) {
  const int n = (int)params.size();
  std::vector<long> host((n + 1) + n * 5);
  long* prefix = host.data();
  long* numels = prefix + (n + 1);
  long* pp = numels + n;
  long* gp = pp + n;
  long* b1 = gp + n;
  long* b2 = b1 + n;
  long chunks = 0;
  for (int i = 0; i < n; ++i) {
    prefix[i] = chunks;
    const long ne = params[i].numel();
    numels[i] = ne;
    chunks += (ne + SLK_OPT_CHUNK - 1) / SLK_OPT_CHUNK;
    pp[i] = (long)params[i].data_ptr<float>();
    gp[i] = (long)grads[i].data_ptr<float>();
    b1[i] = (long)s1[i].data_ptr<float>();
    b2[i] = s2.empty() ? 0 : (long)s2[i].data_ptr<float>();
  }
  prefix[n] = chunks;
  auto t = at::from_blob(host.data(), {(long)host.size()}, at::kLong).clone();
  return t.to(params[0].device());
}

int64_t opt_desc_chunks(const at::Tensor& desc, int64_t n) {
  return desc[ n ].item<int64_t>();
}

// grad_scale = the [norm, coef] pair grad_norm_fused wrote, or nothing
static const float* grad_scale_ptr(const c10::optional<at::Tensor>& gs,
                                   const at::Tensor& desc) {
  if (!gs.has_value()) return nullptr;
  TORCH_CHECK(gs->scalar_type() == at::kFloat && gs->is_contiguous() &&
                  gs->numel() >= 2 && gs->device() == desc.device(),
              "grad_scale: contiguous float32 [2] on the descriptor's device");
  return gs->data_ptr<float>();
}

void grad_norm_fused(const at::Tensor& desc, int64_t n, int64_t chunks,
                     double max_norm, const at::Tensor& partial,
                     const at::Tensor& out) {
  TORCH_CHECK(chunks > 0 && n > 0, "grad_norm_fused: empty descriptor");
  TORCH_CHECK(partial.scalar_type() == at::kDouble && partial.is_contiguous() &&
                  partial.numel() >= chunks && partial.device() == desc.device(),
              "grad_norm_fused: partial is contiguous float64 [chunks]");
  TORCH_CHECK(out.scalar_type() == at::kFloat && out.is_contiguous() &&
                  out.numel() >= 2 && out.device() == desc.device(),
              "grad_norm_fused: out is contiguous float32 [2]");
  auto stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(grad_sumsq_fused_kernel, dim3((uint32_t)chunks), dim3(256), 0,
                     stream, desc.data_ptr<int64_t>(), (int)n,
                     partial.data_ptr<double>());
  hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(256), 0, stream,
                     partial.data_ptr<double>(), (long)chunks, max_norm,
                     out.data_ptr<float>());
}

void sgd_step_fused(const at::Tensor& desc, int64_t n, int64_t chunks, double lr,
                    double momentum, double weight_decay, bool first,
                    bool zero_after, c10::optional<at::Tensor> grad_scale) {
  auto stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(sgd_fused_kernel, dim3((uint32_t)chunks), dim3(256), 0, stream,
                     desc.data_ptr<int64_t>(), (int)n, (float)lr, (float)momentum,
                     (float)weight_decay, first, zero_after,
                     grad_scale_ptr(grad_scale, desc));
}

void adamw_step_fused(const at::Tensor& desc, int64_t n, int64_t chunks,
                      int64_t step, double lr, double beta1, double beta2,
                      double eps, double weight_decay, bool zero_after,
                      c10::optional<at::Tensor> grad_scale) {
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const AdamCoef k = adam_coef(beta1, beta2, step);
  hipLaunchKernelGGL(adamw_fused_kernel, dim3((uint32_t)chunks), dim3(256), 0,
                     stream, desc.data_ptr<int64_t>(), (int)n, (float)lr,
                     (float)beta1, (float)beta2, (float)eps, (float)weight_decay,
                     k, zero_after, grad_scale_ptr(grad_scale, desc));
}

void sgd_step(std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
              std::vector<at::Tensor> bufs, double lr, double momentum,
              double weight_decay, bool first, bool zero_after) {
  auto stream = c10::hip::getCurrentHIPStream().stream();
  for (size_t i = 0; i < params.size(); ++i) {
    const long n = params[i].numel();
    hipLaunchKernelGGL(sgd_kernel, dim3(opt_grid(n)), dim3(256), 0, stream,
                       params[i].data_ptr<float>(), grads[i].data_ptr<float>(),
                       bufs[i].data_ptr<float>(), n, (float)lr, (float)momentum,
                       (float)weight_decay, first, zero_after);
  }
}

void adamw_step(std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
                std::vector<at::Tensor> ms, std::vector<at::Tensor> vs, int64_t step,
                double lr, double beta1, double beta2, double eps,
                double weight_decay, bool zero_after) {
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const AdamCoef k = adam_coef(beta1, beta2, step);
  for (size_t i = 0; i < params.size(); ++i) {
    const long n = params[i].numel();
    hipLaunchKernelGGL(adamw_kernel, dim3(opt_grid(n)), dim3(256), 0, stream,
                       params[i].data_ptr<float>(), grads[i].data_ptr<float>(),
                       ms[i].data_ptr<float>(), vs[i].data_ptr<float>(), n, (float)lr,
                       (float)beta1, (float)beta2, (float)eps, (float)weight_decay,
                       k, zero_after);
  }
}

}  // namespace slk
