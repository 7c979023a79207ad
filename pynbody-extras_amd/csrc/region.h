// region.h — the region a pass keeps particles in (include/pbx.h,
// pbx_profile_set_region / pbx_property_moments_region): a conjunction of at
// most PBX_REGION_MAX clauses, each one primitive (sphere, disc, cuboid, band
// of x / y / z / r / rxy), optionally negated.  The kinds, the negate flags
// and the constants are wave-uniform (scalar loads and scalar branches): a
// kernel argument of the property pass, and for the selection kernels — whose
// SelectParams travels inside several other argument structs — the handle's
// device copy behind a pointer in SelectParams.  The arithmetic is float64
// without FMA contraction in the order pbx.h states, on the coordinates the
// pass holds (the frame's, when one is set).  Every comparison is strict; a
// negated clause is the logical NOT of the clause's boolean (a NaN coordinate
// fails a plain clause and passes a negated one, as ~mask does in numpy).
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/pbx.h"
#include "pbx_common.h"

namespace pbx {

struct Region {
  int n;  // clauses; 0 = no region
  unsigned char kind[PBX_REGION_MAX];
  unsigned char neg[PBX_REGION_MAX];
  double prm[PBX_REGION_MAX][6];  // per kind, as pbx.h lists them
  bool any() const { return n != 0; }
};

// the four arguments of pbx_profile_set_region as a Region (checked)
inline Region region_of(int nclauses, const int *kinds, const int *negate, const double *params) {
  Region g{};
  if (nclauses < 0 || nclauses > PBX_REGION_MAX)
    fail(PBX_ERR_VALUE, "a region holds at most %d clauses (got %d)", PBX_REGION_MAX, nclauses);
  if (nclauses == 0) return g;
  if (!kinds || !params) fail(PBX_ERR_VALUE, "region clauses without kinds or params");
  for (int c = 0; c < nclauses; ++c) {
    const int k = kinds[c];
    if (k < PBX_REGION_SPHERE || k > PBX_REGION_BAND)
      fail(PBX_ERR_VALUE, "clause %d: unknown region kind %d", c, k);
    const double *q = params + 6 * c;
    if (k == PBX_REGION_BAND) {
      const double f = q[0];
      if (!(f == PBX_BAND_X || f == PBX_BAND_Y || f == PBX_BAND_Z || f == PBX_BAND_R ||
            f == PBX_BAND_RXY))
        fail(PBX_ERR_VALUE, "clause %d: unknown band field code %g", c, f);
    }
    g.kind[c] = (unsigned char)k;
    g.neg[c] = (negate && negate[c]) ? 1 : 0;
    for (int j = 0; j < 6; ++j) g.prm[c][j] = q[j];
  }
  g.n = nclauses;
  return g;
}

// every clause of g holds for (x, y, z) (only the kernels instantiated for a
// region call this)
__device__ __forceinline__ bool region_keep(const Region &g, double x, double y, double z) {
#pragma clang fp contract(off)
  bool keep = true;
  // (not unrolled: a clause's constants are scalar loads at a run-time offset
  // inside the loop; unrolled, all 8 x 6 would be held in scalar registers)
#pragma clang loop unroll(disable)
  for (int c = 0; c < g.n; ++c) {
    const double *q = g.prm[c];
    bool in;
    switch (g.kind[c]) {  // (uniform)
      case PBX_REGION_SPHERE: {
        const double dx = x - q[0], dy = y - q[1], dz = z - q[2];
        in = ((dx * dx + dy * dy) + dz * dz) < q[3];
        break;
      }
      case PBX_REGION_DISC: {
        const double dx = x - q[0], dy = y - q[1], dz = z - q[2];
        in = ((dx * dx + dy * dy) < q[3]) & (__builtin_fabs(dz) < q[4]);
        break;
      }
      case PBX_REGION_CUBOID:
        in = (x > q[0]) & (x < q[3]) & (y > q[1]) & (y < q[4]) & (z > q[2]) & (z < q[5]);
        break;
      default: {  // PBX_REGION_BAND: {field, lo, hi, has_lo, has_hi}
        const int fc = (int)q[0];
        double f;
        if (fc == PBX_BAND_X) f = x;
        else if (fc == PBX_BAND_Y) f = y;
        else if (fc == PBX_BAND_Z) f = z;
        else if (fc == PBX_BAND_R) f = __builtin_sqrt((x * x + y * y) + z * z);
        else f = __builtin_sqrt(x * x + y * y);
        in = ((q[3] == 0.0) | (f > q[1])) & ((q[4] == 0.0) | (f < q[2]));
        break;
      }
    }
    keep &= (in != (g.neg[c] != 0));
  }
  return keep;
}

}  // namespace pbx
