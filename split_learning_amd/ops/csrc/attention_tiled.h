// What the tiled attention kernels of both operand types share
// (attention_tiled.hip: fp32 operands, attention_tiled_bf16.hip: bf16
// operands): the argument block, the two operand layouts' addressing, the
// causal block order, the dropout stream and the template dispatch.  The
// layouts, the causal walk and the dropout element index are described in
// attention_tiled.hip's header.
#pragma once

#include <type_traits>

#include "torch_util.h"

namespace slk {

constexpr int AT_TILE = 64;   // rows per block tile and keys per walked tile

// sum / max over the four 16-lane groups that share a row
__device__ __forceinline__ float at_group_sum(float x) {
  x += __shfl_xor(x, 16, 64);
  return x + __shfl_xor(x, 32, 64);
}
__device__ __forceinline__ float at_group_max(float x) {
  x = fmaxf(x, __shfl_xor(x, 16, 64));
  return fmaxf(x, __shfl_xor(x, 32, 64));
}

__device__ __forceinline__ uint32_t at_rng_stream(uint64_t seed, uint64_t offset) {
  return (uint32_t)(slk_mix64(seed ^ slk_mix64(offset)) >> 32);  // = attn_fwd_kernel
}

// One operand's strides in floats (head-strided layout only).
struct AtStride {
  long batch;
  int row;
};

// One block's [S][HD] slice of an operand: its first element and the distance
// between rows.  Contiguous [BH,S,HD]: the distance is the constant HD and
// folds into the address arithmetic as before.  Head-strided: b and h are
// block-uniform, so the slice base is scalar arithmetic done once per operand.
template <class T>
struct AtSlice {
  T* p;
  int ld;
};

template <int HD, bool HEADS, class T>
__device__ __forceinline__ AtSlice<T> at_slice(T* p, const AtStride& st, int bh,
                                               int heads, int S) {
  if constexpr (HEADS)
    return {p + (long)(bh / heads) * st.batch + (bh % heads) * HD, st.row};
  else
    return {p + (long)bh * S * HD, HD};
}

struct AtArgs {
  const float* q;
  const float* k;
  const float* v;
  const float* key_bias;   // [BH/heads, S] or null
  float* out;              // fwd: written; bwd: read
  float* lse;              // [BH,S] fwd: written; bwd: read
  const float* gout;       // bwd
  float* delta;            // [BH,S] dq kernel writes, dkv kernel reads
  float* gq;
  float* gk;
  float* gv;
  const long* offset_in;   // dropout counter (fwd: live; bwd: the saved copy)
  long* offset_out;        // fwd: the offset it read
  uint64_t seed;
  int S, heads;
  float scale, p, inv_keep;
  // head-strided instantiations only (the contiguous ones never read them)
  AtStride sq, sk, sv, so, sgo, sgq, sgk, sgv;
};

// the walked tile's additive row: bias (or 0) at keys < S, -inf past S
template <bool BIAS>
__device__ __forceinline__ float at_key_bias(const float* __restrict__ kbr,
                                             int key, int S) {
  if (key >= S) return -INFINITY;
  return BIAS ? kbr[key] : 0.f;
}

// Which (tile, bh) a block takes; the grid is (tiles, BH) in both modes.
// Non-causal: the block indices as they are.  Causal: a forward / dq block of
// query tile qt walks qt + 1 key tiles and a dkv block of key tile kt walks
// tiles - kt query tiles, so the blocks are taken in launch order level by
// level: all bh of the heaviest tile first (heavy_last: that is the last
// tile, else tile 0), then all bh of the next.  Neighbours in launch order
// then carry equal work, whatever rule spreads them over the chip, and the
// light blocks fill the tail.  (Tile-fastest orders put every bh's heavy
// tile on the same launch-order residue: profiles/SUMMARY.md.)
struct AtBlock {
  int tile, bh;
};
template <bool CAUSAL>
__device__ __forceinline__ AtBlock at_block(bool heavy_last) {
  if (!CAUSAL) return {(int)blockIdx.x, (int)blockIdx.y};
  const unsigned long id = (unsigned long)blockIdx.y * gridDim.x + blockIdx.x;
  const int level = (int)(id / gridDim.y);
  return {heavy_last ? (int)gridDim.x - 1 - level : level, (int)(id % gridDim.y)};
}

// Causal mode, diagonal tile (query tile == key tile): tile-local key `key`
// is hidden from tile-local query row `row` when it lies in the row's future.
__device__ __forceinline__ bool at_hidden(bool diagonal, int row, int key) {
  return diagonal && key > row;
}

// host: the checked problem (attention_tiled.hip: at_check_dims)
struct AtProblem {
  long BH;
  int S, hd;
  bool drop, bias, causal;
  at::Tensor kb, off;
};

#define SLK_AT_DISPATCH(KERNEL, HEADS, pr, grid, stream, args)                 \
  do {                                                                         \
    auto go = [&](auto hd_c, auto drop_c, auto bias_c, auto causal_c) {        \
      hipLaunchKernelGGL(                                                      \
          (KERNEL<decltype(hd_c)::value, decltype(drop_c)::value,              \
                  decltype(bias_c)::value, HEADS,                              \
                  decltype(causal_c)::value>),                                 \
          grid, dim3(256), 0, stream, args);                                   \
    };                                                                         \
    auto go_c = [&](auto hd_c, auto drop_c, auto bias_c) {                     \
      if ((pr).causal) go(hd_c, drop_c, bias_c, std::true_type{});             \
      else go(hd_c, drop_c, bias_c, std::false_type{});                        \
    };                                                                         \
    auto go_b = [&](auto hd_c, auto drop_c) {                                  \
      if ((pr).bias) go_c(hd_c, drop_c, std::true_type{});                     \
      else go_c(hd_c, drop_c, std::false_type{});                              \
    };                                                                         \
    auto go_d = [&](auto hd_c) {                                               \
      if ((pr).drop) go_b(hd_c, std::true_type{});                             \
      else go_b(hd_c, std::false_type{});                                      \
    };                                                                         \
    if ((pr).hd == 32) go_d(std::integral_constant<int, 32>{});                \
    else go_d(std::integral_constant<int, 64>{});                              \
  } while (0)

// attention_tiled_bf16.hip: the bf16-operand kernels behind the same host
// functions (their trailing `bf16` argument), one launch each on `stream`
void at_bf16_fwd(bool heads_layout, const AtProblem& pr, dim3 grid,
                 hipStream_t stream, const AtArgs& a);
void at_bf16_bwd_dq(bool heads_layout, const AtProblem& pr, dim3 grid,
                    hipStream_t stream, const AtArgs& a);
void at_bf16_bwd_dkv(bool heads_layout, const AtProblem& pr, dim3 grid,
                     hipStream_t stream, const AtArgs& a);

}  // namespace slk
