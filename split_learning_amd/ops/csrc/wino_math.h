// The F(2x2, 3x3) Winograd transforms, one definition each for every kernel of
// wino.hip that applies them.  The standalone transform kernels and the fused
// kernels must agree bit for bit (the pair kernel with the two standalone
// fused kernels, the in-kernel weight transform with wino_wt_in_kernel's, the
// fused epilogues with wino_out_kernel / wino_gw_kernel), so both forms of
// each transform call the SAME expression here: a fused body with
// compile-time indices, a thread-per-row kernel with run-time ones.  Keep
// every association and operand order as written; fp contraction has to see
// identical expressions on both sides.
//
//   y  = A^T [ (G g G^T) .* (B^T d B) ] A          forward / bwd-data
//   gw = G^T [ (A gy A^T) (x) (B^T d B) ] G        bwd-weight
//   B^T = [[1,0,-1,0],[0,1,1,0],[0,-1,1,0],[0,1,0,-1]]
//   G   = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]]
//   A   = [[1,0],[1,1],[1,-1],[0,-1]]
//
// Device-only: include from .hip sources.
#pragma once

#include "common.h"

namespace slk {

// tile t = (b, th, tw) of a [B][tH][tW] tile grid; d_thw divides by tH*tW,
// d_tw by tW.  The tile's 2x2 output pixels start at (2 th, 2 tw), its 4x4
// input patch at (2 th - pad, 2 tw - pad).
struct WinoTile { unsigned b, th, tw; };

__device__ __forceinline__ WinoTile wino_tile(unsigned t, const FastDiv& d_thw,
                                              const FastDiv& d_tw) {
  WinoTile r;
  r.b = d_thw.div(t);
  const unsigned rem = d_thw.mod(t, r.b);
  r.th = d_tw.div(rem);
  r.tw = d_tw.mod(rem, r.th);
  return r;
}

// the 4x4 patch of plane xp [H][W] whose corner is (ih0, iw0), zero outside
// the plane (the conv's padding) and all zero when !tv (a tile past the end of
// a bwd-weight slice's range)
__device__ __forceinline__ void wino_load_patch(float (&d)[4][4],
                                                const float* __restrict__ xp,
                                                int ih0, int iw0, int H, int W,
                                                bool tv = true) {
  #pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int ih = ih0 + a;
    const bool hv = tv && (unsigned)ih < (unsigned)H;
    #pragma unroll
    for (int bb = 0; bb < 4; ++bb) {
      const int iw = iw0 + bb;
      const bool v = hv && (unsigned)iw < (unsigned)W;
      d[a][bb] = v ? xp[(long)ih * W + iw] : 0.f;
    }
  }
}

// input transform B^T d B in two halves, so a caller takes one frequency row
// at a time (the fused kernels stage a row with one ds_write_b128).
// u = B^T d: rows [d0-d2, d1+d2, d2-d1, d1-d3]
__device__ __forceinline__ void wino_Bt_d(float (&u)[4][4],
                                          const float (&d)[4][4]) {
  #pragma unroll
  for (int bb = 0; bb < 4; ++bb) {
    u[0][bb] = d[0][bb] - d[2][bb];
    u[1][bb] = d[1][bb] + d[2][bb];
    u[2][bb] = d[2][bb] - d[1][bb];
    u[3][bb] = d[1][bb] - d[3][bb];
  }
}

// frequency row a of (B^T d) B from u = B^T d
__device__ __forceinline__ f32x4 wino_BtdB_row(const float (&u)[4][4], int a) {
  return f32x4{u[a][0] - u[a][2], u[a][1] + u[a][2], u[a][2] - u[a][1],
               u[a][1] - u[a][3]};
}

// row a of G applied to three taps (a column of g for G g, a row of G g for
// (G g) G^T)
__device__ __forceinline__ float wino_G_row(int a, float g0, float g1,
                                            float g2) {
  return a == 0 ? g0
       : a == 1 ? 0.5f * (g0 + g1 + g2)
       : a == 2 ? 0.5f * (g0 - g1 + g2)
       : g2;
}

// frequency row a of the weight transform G g G^T: t = row a of G g
__device__ __forceinline__ f32x4 wino_GgGt_row(const float (&t)[3]) {
  return f32x4{wino_G_row(0, t[0], t[1], t[2]), wino_G_row(1, t[0], t[1], t[2]),
               wino_G_row(2, t[0], t[1], t[2]), wino_G_row(3, t[0], t[1], t[2])};
}

// row a of A applied to a pair: [g0], [g0+g1], [g0-g1], [-g1]
__device__ __forceinline__ float wino_A_row(int a, float g0, float g1) {
  return a == 0 ? g0 : a == 1 ? g0 + g1 : a == 2 ? g0 - g1 : -g1;
}

// frequency row a of dM = A gy A^T for the 2x2 tile gy = [[g00, g01], [g10,
// g11]]: row a of A gy is (c0, c1), then the same across the columns
__device__ __forceinline__ f32x4 wino_AgAt_row(int a, float g00, float g01,
                                               float g10, float g11) {
  const float c0 = wino_A_row(a, g00, g10);
  const float c1 = wino_A_row(a, g01, g11);
  return f32x4{wino_A_row(0, c0, c1), wino_A_row(1, c0, c1),
               wino_A_row(2, c0, c1), wino_A_row(3, c0, c1)};
}

// row o of A^T applied to four values: [m0+m1+m2], [m1-m2-m3]
__device__ __forceinline__ float wino_At_row(int o, float m0, float m1,
                                             float m2, float m3) {
  return o == 0 ? m0 + m1 + m2 : m1 - m2 - m3;
}

// output pixel (oi, oj) of the tile, A^T m A + bv: row oi of A^T m, then the
// same across the columns; the bias goes on last
__device__ __forceinline__ float wino_AtmA(const float (&m)[4][4], int oi,
                                           int oj, float bv) {
  float u[4];
  #pragma unroll
  for (int bb = 0; bb < 4; ++bb)
    u[bb] = wino_At_row(oi, m[0][bb], m[1][bb], m[2][bb], m[3][bb]);
  return wino_At_row(oj, u[0], u[1], u[2], u[3]) + bv;
}

// column of G^T applied to four values: the three taps
// [u0 + .5(u1+u2)], [.5(u1-u2)], [.5(u1+u2) + u3]
__device__ __forceinline__ void wino_Gt_col(float& t0, float& t1, float& t2,
                                            float u0, float u1, float u2,
                                            float u3) {
  t0 = u0 + 0.5f * (u1 + u2);
  t1 = 0.5f * (u1 - u2);
  t2 = 0.5f * (u1 + u2) + u3;
}

// weight gradient gw = G^T u G (3x3) of one (co, ci) pair's 16 frequencies
__device__ __forceinline__ void wino_GtuG(float (&gw)[3][3],
                                          const float (&u)[4][4]) {
  // t = G^T u (3x4)
  float t[3][4];
  #pragma unroll
  for (int b = 0; b < 4; ++b)
    wino_Gt_col(t[0][b], t[1][b], t[2][b], u[0][b], u[1][b], u[2][b], u[3][b]);
  #pragma unroll
  for (int r = 0; r < 3; ++r)
    wino_Gt_col(gw[r][0], gw[r][1], gw[r][2], t[r][0], t[r][1], t[r][2],
                t[r][3]);
}

}  // namespace slk
