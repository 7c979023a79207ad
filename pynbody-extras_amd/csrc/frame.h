// frame.h — the frame a pass reads particles in (include/pbx.h,
// pbx_profile_set_frame / pbx_property_moments_frame): an optional shift, an
// optional periodic wrap (positions only) and an optional rotation of one
// 3-vector array, in this order.  The constants are kernel arguments
// (wave-uniform: scalar registers), the arithmetic is float64 without FMA
// contraction in the order pbx.h states, and a step whose flag is off is
// skipped — never run with zeros or the identity, which would turn an
// infinite coordinate into NaN (0 * inf).
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/pbx.h"
#include "pbx_common.h"

namespace pbx {

// one array's half of a frame (positions: c, R; velocities: vc, R)
struct FrameHalf {
  int shift, rot;
  double c[3];
  double R[9];  // row-major
  bool any() const { return shift || rot; }
};

// the periodic wrap of the positions, between the shift and the rotation
struct FrameWrap {
  int on;
  double L, lo[3];
};

// What a kernel takes.  WRAP is a template parameter of the kernels beside
// FRAME: the wrap-less (and the frame-less) instantiations take FrameK<false>,
// the two halves and nothing else — the argument block they had before the
// wrap existed — and only the instantiations launched for a frame with a wrap
// carry its constants.
template <bool WRAP>
struct FrameK;
template <>
struct FrameK<false> {
  FrameHalf pos, vel;
};
template <>
struct FrameK<true> {
  FrameHalf pos, vel;
  FrameWrap wrap;
};

// both halves and the wrap as pbx.h packs them: frame[15] = {c[3], vc[3],
// R[9]}, and frame[19] = {..., L, lo[3]} with PBX_FRAME_WRAP (host side)
struct Frame {
  FrameHalf pos, vel;
  FrameWrap wrap;
  bool pos_any() const { return pos.any() || wrap.on; }
  bool any() const { return pos_any() || vel.any(); }
  template <bool WRAP>
  FrameK<WRAP> k() const {
    if constexpr (WRAP) return FrameK<true>{pos, vel, wrap};
    else return FrameK<false>{pos, vel};
  }
};

constexpr int FRAME_FLAGS = PBX_FRAME_POS | PBX_FRAME_VEL | PBX_FRAME_ROT | PBX_FRAME_WRAP;

// flags / frame as an entry point receives them: unknown bits and a bad wrap
// are a PBX_ERR_VALUE; frame[15..18] is read only with PBX_FRAME_WRAP
inline Frame frame_of(int flags, const double *f) {
  if (flags & ~FRAME_FLAGS)
    fail(PBX_ERR_VALUE, "flags must be a mask of PBX_FRAME_* bits (got 0x%x)", flags);
  Frame fr{};
  if (!f) return fr;
  if (flags & PBX_FRAME_WRAP) {
    const double L = f[15];
    if (!(L > 0.0) || L == __builtin_inf())
      fail(PBX_ERR_VALUE, "PBX_FRAME_WRAP: the box size must be finite and positive (got %g)", L);
    for (int k = 0; k < 3; ++k)
      if (f[16 + k] != 0.0 && f[16 + k] != -0.5 * L)
        fail(PBX_ERR_VALUE, "PBX_FRAME_WRAP: lo[%d] must be 0.0 or -0.5 * L (got %g, L = %g)", k,
             f[16 + k], L);
    fr.wrap.on = 1;
    fr.wrap.L = L;
    for (int k = 0; k < 3; ++k) fr.wrap.lo[k] = f[16 + k];
  }
  fr.pos.shift = (flags & PBX_FRAME_POS) != 0;
  fr.vel.shift = (flags & PBX_FRAME_VEL) != 0;
  fr.pos.rot = fr.vel.rot = (flags & PBX_FRAME_ROT) != 0;
  for (int k = 0; k < 3; ++k) {
    fr.pos.c[k] = f[k];
    fr.vel.c[k] = f[3 + k];
  }
  for (int k = 0; k < 9; ++k) fr.pos.R[k] = fr.vel.R[k] = f[6 + k];
  return fr;
}

__device__ __forceinline__ void frame_shift(const FrameHalf &h, double &x, double &y, double &z) {
#pragma clang fp contract(off)
  if (h.shift) {
    x = x - h.c[0];
    y = y - h.c[1];
    z = z - h.c[2];
  }
}

__device__ __forceinline__ void frame_rotate(const FrameHalf &h, double &x, double &y, double &z) {
#pragma clang fp contract(off)
  if (h.rot) {
    const double a = x, b = y, c = z;
    x = (h.R[0] * a + h.R[1] * b) + h.R[2] * c;
    y = (h.R[3] * a + h.R[4] * b) + h.R[5] * c;
    z = (h.R[6] * a + h.R[7] * b) + h.R[8] * c;
  }
}

// the periodic wrap into [lo, lo + L): IEEE division, floor, and "+ 0.0" so
// that a -0.0 from floor counts as +0.0 (then -0.0 - 0.0 * L stays -0.0, as
// the reference's integer k gives)
__device__ __forceinline__ void frame_wrap(const FrameWrap &w, double &x, double &y, double &z) {
#pragma clang fp contract(off)
  if (w.on) {
    x = x - (__builtin_floor((x - w.lo[0]) / w.L) + 0.0) * w.L;
    y = y - (__builtin_floor((y - w.lo[1]) / w.L) + 0.0) * w.L;
    z = z - (__builtin_floor((z - w.lo[2]) / w.L) + 0.0) * w.L;
  }
}

// a wrap-less half (every velocity; positions without a wrap): shift, rotation
__device__ __forceinline__ void frame_apply(const FrameHalf &h, double &x, double &y, double &z) {
  frame_shift(h, x, y, z);
  frame_rotate(h, x, y, z);
}

// positions with a wrap: shift, wrap, rotation
__device__ __forceinline__ void frame_apply(const FrameHalf &h, const FrameWrap &w, double &x,
                                            double &y, double &z) {
  frame_shift(h, x, y, z);
  frame_wrap(w, x, y, z);
  frame_rotate(h, x, y, z);
}

template <bool WRAP>
__device__ __forceinline__ void frame_apply_pos(const FrameK<WRAP> &f, double &x, double &y,
                                                double &z) {
  if constexpr (WRAP) frame_apply(f.pos, f.wrap, x, y, z);
  else frame_apply(f.pos, x, y, z);
}

}  // namespace pbx
