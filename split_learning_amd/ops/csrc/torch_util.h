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

// The one way to fill a FastDiv (common.h): divisor d (0 stands for an empty
// dimension and divides as 1) and the largest dividend the op's kernels will
// pass to div(); max_n < 0 means none (a divider the launch does not use).
// Refuses, before anything is launched, a pair whose quotients are not exact.
static inline FastDiv fast_div(long d, long max_n, const char* op) {
  if (d == 0) d = 1;
  if (max_n < 0) max_n = 0;
  TORCH_CHECK(d > 0 && FastDiv::covers((unsigned long long)d,
                                       (unsigned long long)max_n),
              op, ": index ", max_n, " divided by ", d,
              " is outside FastDiv's exact range (needs index * divisor < 2^40"
              " and index < 2^31); use a smaller batch or image");
  FastDiv f;
  f.d = (unsigned)d;
  f.m = (0x10000000000ull / f.d) + 1;
  return f;
}

// chunk count for per-channel reductions over (B, HW) that write chunk slabs
// and finalize in fixed order (BatchNorm statistics, conv bias gradient)
static inline int reduce_chunks(long per_channel) {
  long c = per_channel / 4096;
  if (c < 1) c = 1;
  if (c > 16) c = 16;
  return (int)c;
}

// key_bias is [BH/heads, S] additive fp32 (BERT feeds -10000 at pads, MHA
// -inf); one row per sample, shared by that sample's heads.  (attention.hip,
// attention_tiled.hip)
static inline at::Tensor check_key_bias(const at::Tensor& kb, long BH, long S,
                                        int64_t heads, const char* who) {
  TORCH_CHECK(heads >= 1 && BH % heads == 0, who, ": BH=", BH,
              " is not a multiple of heads=", heads);
  TORCH_CHECK(kb.is_cuda() && kb.scalar_type() == at::kFloat && kb.dim() == 2 &&
                  kb.size(0) == BH / heads && kb.size(1) == S,
              who, ": key_bias must be a float32 cuda tensor [BH/heads=",
              BH / heads, ", S=", S, "]");
  return kb.contiguous();
}

// out[i] = sum_s slab[s*numel + i], s in fixed order (conv2d.hip)
void slab_reduce(const float* slab, int splits, float* out, long numel,
                 hipStream_t stream);
// the same for two slab sets in one launch; a set with numel 0 has no job
void slab_reduce_pair(const float* slab_a, int splits_a, float* out_a,
                      long numel_a, const float* slab_b, int splits_b,
                      float* out_b, long numel_b, hipStream_t stream);

}  // namespace slk
