// Which kernel a conv call runs: the whole decision, as pure functions of the
// conv shape and the SLK_WINO level.  Host-only and header-free on purpose, so
// the table compiles and can be checked without a GPU or torch.
//
// SLK_WINO level: 0 = direct kernels only, 1 = measured routing (default),
// 2 = force the unfused Winograd forms wherever they are legal (sweeps),
// 3 = additionally force the fused forward/bwd-data kernel wherever legal.
#pragma once

namespace slk {

enum class ConvRoute {
  Direct,         // implicit-GEMM gather kernel (conv2d.hip)
  Wino,           // transform + 16 frequency GEMMs + transform (wino.hip)
  WinoFused,      // wino_fused_kernel: transforms in-kernel
  WinoBwdW,       // bwd-weight transform + frequency-GEMM pipeline
  WinoBwdWFused,  // wino_bwdw_fused_kernel
};

inline const char* conv_route_name(ConvRoute r) {
  switch (r) {
    case ConvRoute::Direct: return "direct";
    case ConvRoute::Wino: return "wino";
    case ConvRoute::WinoFused: return "wino_fused";
    case ConvRoute::WinoBwdW: return "wino_bwdw";
    case ConvRoute::WinoBwdWFused: return "wino_bwdw_fused";
  }
  return "?";
}

// the FORWARD conv's shape: x [B, Ci, H, W], w [Co, Ci, KH, KW]; all three
// directions of one layer are routed from the same nine numbers
struct ConvShape {
  int B, Ci, H, W, Co, KH, KW, stride, pad;
  int OH() const { return (H + 2 * pad - KH) / stride + 1; }
  int OW() const { return (W + 2 * pad - KW) / stride + 1; }
  bool is_3x3_s1() const { return KH == 3 && KW == 3 && stride == 1; }
};

// fused-Winograd eligibility for a 3x3 s1 conv Cin -> Cout with T 2x2 output
// tiles: shape constraints + grid fill.  The fused kernel's base grid is
// (T/32) x (Cout/32); for FORWARD the measured win/lose line falls at >= 256
// base blocks (1 per CU) — below it the ci-split can fill the grid but the
// forward still measured WORSE fused (8x8 tails: 52.4 vs 49.9 us), so forward
// keeps the 256 rule.  Backward-data has an extension below.
inline bool wino_fused_ok(int level, int Cin, int Cout, int T, int OH, int OW) {
  if (level == 0) return false;
  if ((OH | OW) & 1) return false;
  if (Cout % 32 != 0 || T % 32 != 0 || Cin % 8 != 0) return false;
  if (level >= 3) return true;  // force: ci-split fills the grid (sweeps)
  return (long)(T / 32) * (Cout / 32) >= 256;
}

// unfused F(2x2,3x3) beats the direct implicit-GEMM kernel on the MEASURED win
// set only — square channel counts at either end of the stack (64ch/32x32 and
// >=256ch tails); the 128ch middle loses to V/M HBM inflation
// (tools/wino_check.py table in profiles/SUMMARY.md).  H is the height of the
// tensor being convolved (x forward, gy backward-data).
inline bool wino_wins(int level, int Ci, int Co, int H, int OH, int OW) {
  if (level == 0) return false;
  if ((OH | OW) & 1) return false;
  if (level >= 2) return true;  // force (sweeps)
  return Ci == Co && (Ci >= 256 || H >= 32);
}

inline bool wino_wins_bwdw(int level, int Ci, int Co, int H, int OH, int OW) {
  if (level == 0) return false;
  if ((OH | OW) & 1) return false;
  if (level >= 2) return true;
  // measured win set (tools/wino_check.py under SLK_WINO=0): square channel
  // counts win everywhere EXCEPT the 4x4 layers, where T = B*4 makes the
  // frequency GEMMs too small (512ch 4x4: 62 vs 48 us direct); the stem
  // (3ch 32x32) also wins mildly (44.9 vs 49.3 us) — its direct form is a
  // 9-n-tile tall-K pathology
  return (Ci == Co && H != 4) || (Ci <= 4 && H >= 32);
}

inline ConvRoute route_fwd(const ConvShape& s, int level) {
  if (s.is_3x3_s1()) {
    const int OH = s.OH(), OW = s.OW();
    const int T = s.B * (OH / 2) * (OW / 2);
    if (wino_fused_ok(level, s.Ci, s.Co, T, OH, OW)) return ConvRoute::WinoFused;
    if (wino_wins(level, s.Ci, s.Co, s.H, OH, OW)) return ConvRoute::Wino;
  }
  return ConvRoute::Direct;
}

// gx = winograd-conv of gy (Co channels, OH x OW) with the rotated/transposed
// weights at pad' = 2 - pad, producing Ci channels at H x W
inline ConvRoute route_bwd_data(const ConvShape& s, int level) {
  if (s.is_3x3_s1() && s.pad <= 2) {
    const int T = s.B * (s.H / 2) * (s.W / 2);
    if (s.H % 2 == 0 && s.W % 2 == 0) {
      if (wino_fused_ok(level, s.Co, s.Ci, T, s.H, s.W)) return ConvRoute::WinoFused;
      // backward-data ONLY: the ci-split fused kernel also wins on the
      // small-T high-channel tails (measured, 40-iter A/B under SLK_WINO=3:
      // 256ch 8x8 44.6 vs 49.3 us, 256->512 4x4 31.6 vs 38.1, 512ch 4x4 45.3
      // vs 49.9; the 2x2 layers lose 62 vs 35 and stay out).  Forward at the
      // same shapes measured WORSE fused and keeps the >=256-block rule.
      // Ci >= 64: measured down to 64ch gx (24.4 vs 37.0 us).
      if (level != 0 && s.H >= 4 && s.Ci >= 64 && s.Ci % 32 == 0 &&
          s.Co % 8 == 0 && T % 32 == 0 && (long)(T / 32) * (s.Ci / 32) >= 32) {
        return ConvRoute::WinoFused;
      }
    }
    if (wino_wins(level, s.Co, s.Ci, s.OH(), s.H, s.W)) return ConvRoute::Wino;
  }
  return ConvRoute::Direct;
}

// Winograd weight-gradient.  FUSED twin first (in-kernel transforms,
// tile-axis reduction with per-slice slabs): measured faster than every
// alternative on ALL eligible shapes — 512ch 2x2: 13.2 us vs 29.1 routed,
// 512ch 4x4: 36.2 vs 48.2, 64->128: 33.5 vs 45.9 (profiles/SUMMARY.md).  The
// transform+frequency-GEMM pipeline remains for Ci/Co not multiples of 32.
inline ConvRoute route_bwd_weight(const ConvShape& s, int level) {
  const int OH = s.OH(), OW = s.OW();
  if (s.is_3x3_s1() && s.pad <= 2 && OH % 2 == 0 && OW % 2 == 0) {
    if (level != 0 && s.Ci % 32 == 0 && s.Co % 32 == 0) {
      return ConvRoute::WinoBwdWFused;
    }
    if (wino_wins_bwdw(level, s.Ci, s.Co, s.H, OH, OW)) return ConvRoute::WinoBwdW;
  }
  return ConvRoute::Direct;
}

}  // namespace slk
