// Row softmax (attention) and fused cross-entropy (log-softmax + NLL, mean
// reduction) with on-GPU NaN detection — feature parity with the reference's
// per-batch NaN check (src/train/VGG16.py:169-171).
#include <torch/extension.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include "common.h"

namespace slk {

// one wave per row; D looped in chunks of 64
__global__ void softmax_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                   long R, int D) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int waves = blockDim.x >> 6;
  for (long row = (long)blockIdx.x * waves + wid; row < R;
       row += (long)gridDim.x * waves) {
    const float* xr = x + row * D;
    float* yr = y + row * D;
    float m = -INFINITY;
    for (int d = lane; d < D; d += 64) m = fmaxf(m, xr[d]);
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    float s = 0.f;
    for (int d = lane; d < D; d += 64) {
      const float e = expf(xr[d] - m);
      yr[d] = e;
      s += e;
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    const float inv = 1.f / s;
    for (int d = lane; d < D; d += 64) yr[d] *= inv;
  }
}

__global__ void softmax_bwd_kernel(const float* __restrict__ gy,
                                   const float* __restrict__ y,
                                   float* __restrict__ gx, long R, int D) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int waves = blockDim.x >> 6;
  for (long row = (long)blockIdx.x * waves + wid; row < R;
       row += (long)gridDim.x * waves) {
    const float* gr = gy + row * D;
    const float* yr = y + row * D;
    // gy - dot cancels: a near-one-hot row leaves ~1e-4 of its operands, so
    // dot and the difference stay in double (D/64 terms per lane) and gx is
    // the rounded result of the saved fp32 y, not of a rounded dot
    double dot = 0.0;
    for (int d = lane; d < D; d += 64) dot += (double)gr[d] * (double)yr[d];
    for (int off = 32; off > 0; off >>= 1) dot += __shfl_xor(dot, off, 64);
    float* oxr = gx + row * D;
    for (int d = lane; d < D; d += 64)
      oxr[d] = (float)((double)yr[d] * ((double)gr[d] - dot));
  }
}

at::Tensor softmax_fwd(const at::Tensor& x) {
  const long R = x.size(0);
  const int D = x.size(1);
  auto y = at::empty_like(x);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const int waves = 4;
  int grid = (int)std::min<long>((R + waves - 1) / waves, 4096);
  hipLaunchKernelGGL(softmax_fwd_kernel, dim3(grid), dim3(64 * waves), 0, stream,
                     x.data_ptr<float>(), y.data_ptr<float>(), R, D);
  return y;
}

at::Tensor softmax_bwd(const at::Tensor& gy, const at::Tensor& y) {
  const long R = gy.size(0);
  const int D = gy.size(1);
  auto gx = at::empty_like(gy);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const int waves = 4;
  int grid = (int)std::min<long>((R + waves - 1) / waves, 4096);
  hipLaunchKernelGGL(softmax_bwd_kernel, dim3(grid), dim3(64 * waves), 0, stream,
                     gy.data_ptr<float>(), y.data_ptr<float>(), gx.data_ptr<float>(),
                     R, D);
  return gx;
}

// fused CE forward: probs[b] = softmax(logits[b]); loss = mean(-log p[label]).
// One wave per row, each wave summing its rows in order.  A single-block
// launch (small B) adds the waves' sums in fixed order and stores the loss,
// so it is the same every run; multi-block launches atomicAdd into a zeroed
// DOUBLE scalar (hundreds of float adds into a sum of size `loss` each
// rounded to its ulp: 7 ulp off at B = 300) that the host casts to float.
__global__ void ce_fwd_kernel(const float* __restrict__ logits,
                              const int64_t* __restrict__ labels,
                              float* __restrict__ probs, float* __restrict__ loss,
                              double* __restrict__ loss_acc, int B, int C) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int waves = blockDim.x >> 6;
  __shared__ float wave_sum[16];
  float acc = 0.f;
  for (int row = blockIdx.x * waves + wid; row < B; row += gridDim.x * waves) {
    const float* xr = logits + (long)row * C;
    float* pr = probs + (long)row * C;
    if (C <= 64) {
      // a lane per class: logit and exp stay in registers, probs is written
      // once (e * inv, the value the store-reload-multiply below leaves), and
      // the label is fetched before the reductions; its logit comes from the
      // lane that holds it
      const bool in = lane < C;
      const int64_t lbl = labels[row];
      const float xv = in ? xr[lane] : 0.f;
      float m = in ? fmaxf(-INFINITY, xv) : -INFINITY;
      for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
      const float e = expf(xv - m);
      float s = 0.f;
      if (in) s += e;
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      const float inv = 1.f / s;
      if (in) pr[lane] = e * inv;
      // a label outside [0, C) is the caller's error here as in the loop form
      // (there an out-of-bounds read, here another lane's value)
      const float xl = __shfl(xv, (int)lbl, 64);
      if (lane == 0) {
        const float lse = m + logf(s);
        acc += (lse - xl) / (float)B;
      }
      continue;
    }
    float m = -INFINITY;
    for (int d = lane; d < C; d += 64) m = fmaxf(m, xr[d]);
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    float s = 0.f;
    for (int d = lane; d < C; d += 64) {
      const float e = expf(xr[d] - m);
      pr[d] = e;
      s += e;
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    const float inv = 1.f / s;
    for (int d = lane; d < C; d += 64) pr[d] *= inv;
    if (lane == 0) {
      const int64_t lbl = labels[row];
      const float lse = m + logf(s);
      acc += (lse - xr[lbl]) / (float)B;
    }
  }
  if (gridDim.x > 1) {
    if (lane == 0 && acc != 0.f) atomicAdd(loss_acc, (double)acc);
    return;
  }
  if (lane == 0) wave_sum[wid] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int k = 0; k < waves; ++k) s += wave_sum[k];
    *loss = s;
  }
}

__global__ void ce_bwd_kernel(const float* __restrict__ probs,
                              const int64_t* __restrict__ labels,
                              const float* __restrict__ gloss,
                              float* __restrict__ glogits, int B, int C) {
  const long total = (long)B * C;
  const float g = *gloss / (float)B;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int row = (int)(i / C);
    const int col = (int)(i - (long)row * C);
    const float onehot = (labels[row] == col) ? 1.f : 0.f;
    glogits[i] = (probs[i] - onehot) * g;
  }
}

std::vector<at::Tensor> ce_fwd(const at::Tensor& logits, const at::Tensor& labels) {
  const int B = logits.size(0), C = logits.size(1);
  auto probs = at::empty_like(logits);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const int waves = 4;
  int grid = std::max(1, std::min((B + waves - 1) / waves, 1024));
  if (B <= 256) grid = 1;  // fixed-order in-block sum (see ce_fwd_kernel)
  if (grid == 1) {
    auto loss = at::zeros({}, logits.options());
    hipLaunchKernelGGL(ce_fwd_kernel, dim3(1), dim3(64 * waves), 0, stream,
                       logits.data_ptr<float>(), labels.data_ptr<int64_t>(),
                       probs.data_ptr<float>(), loss.data_ptr<float>(), nullptr,
                       B, C);
    return {loss, probs};
  }
  // B > 256 only: the double scalar costs one cast launch that the one-block
  // path (every batch size the zoo trains or benchmarks with) does not pay
  auto acc = at::zeros({}, logits.options().dtype(at::kDouble));
  hipLaunchKernelGGL(ce_fwd_kernel, dim3(grid), dim3(64 * waves), 0, stream,
                     logits.data_ptr<float>(), labels.data_ptr<int64_t>(),
                     probs.data_ptr<float>(), nullptr, acc.data_ptr<double>(), B,
                     C);
  return {acc.to(at::kFloat), probs};
}

at::Tensor ce_bwd(const at::Tensor& probs, const at::Tensor& labels,
                  const at::Tensor& gloss) {
  const int B = probs.size(0), C = probs.size(1);
  auto glogits = at::empty_like(probs);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const long total = (long)B * C;
  int grid = (int)std::min<long>((total + 255) / 256, 2048);
  hipLaunchKernelGGL(ce_bwd_kernel, dim3(grid), dim3(256), 0, stream,
                     probs.data_ptr<float>(), labels.data_ptr<int64_t>(),
                     gloss.data_ptr<float>(), glogits.data_ptr<float>(), B, C);
  return glogits;
}

}  // namespace slk
