// frame.h — the affine frame a pass reads particles in (include/pbx.h,
// pbx_profile_set_frame / pbx_property_moments_frame): an optional shift and
// an optional rotation of one 3-vector array.  The constants are kernel
// arguments (wave-uniform: scalar registers), the arithmetic is float64
// without FMA contraction in the order pbx.h states, and a step whose flag is
// off is skipped — never run with zeros or the identity, which would turn an
// infinite coordinate into NaN (0 * inf).
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/pbx.h"

namespace pbx {

// one array's half of a frame (positions: c, R; velocities: vc, R)
struct FrameHalf {
  int shift, rot;
  double c[3];
  double R[9];  // row-major
};

// both halves as pbx.h packs them: frame[15] = {c[3], vc[3], R[9]}
struct Frame {
  FrameHalf pos, vel;
  bool any() const { return pos.shift || pos.rot || vel.shift || vel.rot; }
};

inline Frame frame_of(int flags, const double *f) {
  Frame fr{};
  if (!f) return fr;
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

__device__ __forceinline__ void frame_apply(const FrameHalf &h, double &x, double &y, double &z) {
#pragma clang fp contract(off)
  if (h.shift) {
    x = x - h.c[0];
    y = y - h.c[1];
    z = z - h.c[2];
  }
  if (h.rot) {
    const double a = x, b = y, c = z;
    x = (h.R[0] * a + h.R[1] * b) + h.R[2] * c;
    y = (h.R[3] * a + h.R[4] * b) + h.R[5] * c;
    z = (h.R[6] * a + h.R[7] * b) + h.R[8] * c;
  }
}

}  // namespace pbx
