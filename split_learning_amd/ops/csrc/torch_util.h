// Host helpers shared by the torch-facing .hip files (common.h stays free of
// torch headers).
#pragma once

#include <torch/extension.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include "common.h"

namespace slk {

// empty + single fill-KERNEL launch instead of at::zeros (no aten dispatch;
// and never hipMemsetAsync — see slk_zero_async in common.h).
static inline at::Tensor zeroed(at::IntArrayRef sizes, const at::TensorOptions& opt) {
  auto t = at::empty(sizes, opt);
  slk_zero_async(t.data_ptr<float>(), t.numel(),
                 c10::hip::getCurrentHIPStream().stream());
  return t;
}

// chunk count for per-channel reductions over (B, HW) that write chunk slabs
// and finalize in fixed order (BatchNorm statistics, conv bias gradient)
static inline int reduce_chunks(long per_channel) {
  long c = per_channel / 4096;
  if (c < 1) c = 1;
  if (c > 16) c = 16;
  return (int)c;
}

// out[i] = sum_s slab[s*numel + i], s in fixed order (conv2d.hip)
void slab_reduce(const float* slab, int splits, float* out, long numel,
                 hipStream_t stream);
// the same for two slab sets in one launch; a set with numel 0 has no job
void slab_reduce_pair(const float* slab_a, int splits_a, float* out_a,
                      long numel_a, const float* slab_b, int splits_b,
                      float* out_b, long numel_b, hipStream_t stream);

}  // namespace slk
