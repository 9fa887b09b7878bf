// Common helpers for the split_learning_amd CDNA4 (gfx950) kernels.
// All kernels here are written directly in HIP for MI355X — wave64, MFMA
// matrix cores, LDS — no CUDA compatibility paths.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#define SLK_WAVE 64

using f32x2 = __attribute__((ext_vector_type(2))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;

#define HIP_CHECK(expr)                                                          \
  do {                                                                           \
    hipError_t _e = (expr);                                                      \
    if (_e != hipSuccess) {                                                      \
      TORCH_CHECK(false, "HIP error: ", hipGetErrorString(_e), " at ", __FILE__, \
                  ":", __LINE__);                                                \
    }                                                                            \
  } while (0)

static inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }

// Zero-fill as a KERNEL node, never hipMemsetAsync: captured memset nodes were
// observed to intermittently misorder against dependent kernel nodes on
// hipGraph replay (per-process at graphExec instantiation; root-caused by
// bisection — see profiles/SUMMARY.md "graph divergence").  Kernel nodes
// order correctly; cost is the same single launch.
static __global__ void slk_zero_kernel(float* __restrict__ p, long n) {
  // float4 main body + scalar tail (torch allocations are 16B-aligned)
  const long n4 = n >> 2;
  f32x4* __restrict__ p4 = reinterpret_cast<f32x4*>(p);
  const long stride = (long)gridDim.x * blockDim.x;
  const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long i = i0; i < n4; i += stride) p4[i] = f32x4{};
  for (long i = (n4 << 2) + i0; i < n; i += stride) p[i] = 0.f;
}

static inline void slk_zero_async(float* p, long n, hipStream_t stream) {
  const int grid = (int)std::min<long>((n / 4 + 255) / 256 + 1, 4096);
  hipLaunchKernelGGL(slk_zero_kernel, dim3(grid), dim3(256), 0, stream, p, n);
}

// splitmix64 — counter-based RNG hash for dropout (deterministic per
// (seed, offset, index); quality is ample for Bernoulli masks).
__device__ __forceinline__ uint64_t slk_mix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__device__ __forceinline__ float slk_uniform(uint64_t seed, uint64_t offset,
                                             uint64_t idx) {
  uint64_t h = slk_mix64(seed ^ slk_mix64(offset * 0xD1342543DE82EF95ull + idx));
  // top 24 bits -> [0, 1)
  return (float)(h >> 40) * (1.0f / 16777216.0f);
}

// 32-bit mask hash (lowbias32) for dropout draws INSIDE compute kernels:
// ~6 VALU vs ~25 for the 64-bit path (two splitmix64 = four 64-bit
// multiplies) — the difference made the fused attention kernel VALU-bound
// at BERT scale.  Fold (seed, offset) into one 32-bit stream id host/SALU-
// side via slk_mix64 first.
__device__ __forceinline__ float slk_uniform32(uint32_t stream, uint32_t idx) {
  uint32_t x = idx * 0x9E3779B9u + stream;
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return (float)(x >> 8) * (1.0f / 16777216.0f);
}

// ReLU and the max-pool selection rule, one definition each for every kernel
// that applies them (standalone and fused forms must agree bit for bit).
// Both keep a NaN, as torch does: fmaxf(NaN, 0) is 0 and NaN > best is false,
// either of which turns a diverged activation into a healthy-looking zero
// before the loss's NaN check can see it.
__device__ __forceinline__ float slk_relu(float v) {
  return v <= 0.f ? 0.f : v;
}

// does v replace the running maximum best?  (torch: val > max || isnan(val))
__device__ __forceinline__ bool slk_pool_takes(float v, float best) {
  return v > best || v != v;
}

// Fast integer division by a runtime constant (one 64-bit mul + shift).
// Valid for dividend < 2^24 and divisor < 2^16 (all tensor-index math here):
// m = floor(2^40/d)+1; q = (n*m) >> 40 == n/d exactly when n*d < 2^40.
struct FastDiv {
  unsigned d;
  unsigned long long m;
  void init(unsigned d_) {
    d = d_ == 0 ? 1 : d_;
    m = (0x10000000000ull / d) + 1;
  }
  __device__ __forceinline__ unsigned div(unsigned n) const {
    return (unsigned)(((unsigned long long)n * m) >> 40);
  }
  __device__ __forceinline__ unsigned mod(unsigned n, unsigned q) const {
    return n - q * d;
  }
};

// A loop i = first, first + step, ... < hi whose iterations each load and then
// use, run U iterations at a time: the loads of U consecutive iterations are
// issued before the first use, so a wave has U (times the loads per
// iteration) memory requests in flight where the plain loop has one and waits
// a full round trip per iteration.  use() runs in ascending i on the same
// thread as in the plain loop, so whatever it accumulates keeps its order and
// its bits.  What is left after the last full batch runs as one batch each of
// U/2, U/4, ... 1 iterations where that many remain: nothing past hi is
// loaded or used, and no load sits under a predicate of its own (the compiler
// pulls the first use into such a block, and with it the wait).
template <int U, class T, class I, class Load, class Use>
__device__ __forceinline__ void slk_batched(I first, I hi, I step, Load load,
                                            Use use) {
  static_assert(U >= 1 && (U & (U - 1)) == 0, "U: a power of two");
  I i = first;
  // hi - (U - 1) * step cannot overflow where i + (U - 1) * step could
  for (; i < hi - (U - 1) * step; i += U * step) {
    T v[U];
    #pragma unroll
    for (int u = 0; u < U; ++u) v[u] = load(i + u * step);
    #pragma unroll
    for (int u = 0; u < U; ++u) use(i + u * step, v[u]);
  }
  if constexpr (U > 1) slk_batched<U / 2, T>(i, hi, step, load, use);
}

// batch depths (loads in flight per wave and stream) of the reduction loops;
// ops/build.py passes SLK_BN_U / SLK_SLAB_U from the environment for sweeps
// with tools/reduce_bench.py (profiles/SUMMARY.md round 8)
#ifndef SLK_BN_U
#define SLK_BN_U 8      // BatchNorm sums and the one-launch kernels' phase 2
#endif
#ifndef SLK_SLAB_U
#define SLK_SLAB_U 8    // split-K slab sums
#endif

// out[i] = 0.f + slab[i] + slab[numel + i] + ... in slab order, the split-K
// finalize of every slab producer (conv2d.hip, wino.hip, gemm_f32.hip).
// V is float, or f32x4 where numel % 4 == 0 and both bases are 16-byte
// aligned (numel then counts vectors); a vector add is four scalar adds, so
// an element's sum does not depend on V or on the thread that forms it.
// (block, nblocks): the launch's blocks that work on this slab set
template <class V>
__device__ __forceinline__ void slab_reduce_body(const V* __restrict__ slab,
                                                 int splits,
                                                 V* __restrict__ out,
                                                 long numel, int block,
                                                 int nblocks) {
  const long stride = (long)nblocks * blockDim.x;
  for (long i = (long)block * blockDim.x + threadIdx.x; i < numel;
       i += stride) {
    V s = V(0.f);
    slk_batched<SLK_SLAB_U, V>(
        0, splits, 1, [&](int k) { return slab[(long)k * numel + i]; },
        [&](int, const V& v) { s += v; });
    out[i] = s;
  }
}

static inline bool slab_is_vec4(const void* slab, const void* out, long numel) {
  return numel % 4 == 0 && (((uintptr_t)slab | (uintptr_t)out) & 15) == 0;
}

// blocks of 256 threads for one slab set: a thread per float4 or per float
static inline int slab_reduce_grid(const void* slab, const void* out,
                                   long numel) {
  const long n = slab_is_vec4(slab, out, numel) ? numel / 4 : numel;
  return (int)std::min<long>((n + 255) / 256, 4096);
}

// block-level reduction into lane 0 of wave 0 (sums `val` over blockDim.x
// threads; blockDim.x must be a multiple of 64 and <= 1024)
template <typename T>
__device__ __forceinline__ T slk_block_sum(T val, T* lds_scratch /* >= 16 */) {
  // wave reduce
  for (int off = 32; off > 0; off >>= 1) val += __shfl_down(val, off, 64);
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int nwaves = blockDim.x >> 6;
  if (lane == 0) lds_scratch[wid] = val;
  __syncthreads();
  T out = (T)0;
  if (wid == 0) {
    out = (lane < nwaves) ? lds_scratch[lane] : (T)0;
    for (int off = 8; off > 0; off >>= 1) out += __shfl_down(out, off, 64);
  }
  return out;  // valid in thread 0 only
}
