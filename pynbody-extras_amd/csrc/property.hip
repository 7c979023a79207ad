// property.hip — scalar properties of a particle selection on gfx950.
//
// Replaces the numpy passes of pynbodyext.properties (properties/generic.py:
// 39-198: centre of mass, bulk velocity, angular momentum, kappa_rot, pattern
// speed; properties/base.py:106-119: ParamSum) and the shrinking-sphere
// centre behind CenPos("ssc"): one streaming read of the particles with the
// Sphere / family predicate of the profile selection applied in the same
// pass, a count and up to 18 float64 sums out.
//
// Determinism: the particle -> thread mapping depends only on (span, grid)
// and the grid only on span; a thread adds its particles in index order in
// registers; a wave combines its lanes with a fixed __shfl_xor butterfly; a
// block adds its waves in wave order through LDS and writes one row of
// partials; property_reduce adds the rows in a fixed order (the
// reduce_slab_part / reduce_slab_final convention of profile.hip: PROP_RG
// interleaved partials, then the partials in order).  No floating-point
// atomics.  Every accumulator is independent of the others, so the group
// mask never changes a sum's bits.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "frame.h"
#include "pbx_common.h"
#include "region.h"

namespace pbx {
namespace prop {

constexpr int MAX_FAM = 16;
constexpr int NS = PBX_PROP_NSUMS;
constexpr int PROP_TPB = 256;                // threads per block
constexpr int PROP_NW = PROP_TPB / 64;       // waves per block
constexpr int PROP_ITEMS = 4;                // particles per thread and sweep, all loads in flight
// at most 4 blocks per CU of the 256-CU part; a constant, not the device's
// CU count, so that a span maps to the same grid (and the same bits) on
// every device.  One sweep of the full grid covers
// PROP_MAX_BLOCKS * PROP_TPB * PROP_ITEMS = 1,048,576 particles.
constexpr int PROP_MAX_BLOCKS = 1024;
constexpr int PROP_RG = 32;                  // interleaved partials of property_reduce
constexpr int PROP_NOUT = NS + 1;            // the sums and the count
constexpr int MAX_SHRINK_ITER = 10000;       // pbx_property_shrink_center gives up after this many

constexpr uint32_t POS_GROUPS = PBX_PROP_COM | PBX_PROP_ANGMOM | PBX_PROP_KAPPA |
                                PBX_PROP_KAPPA_MEAN | PBX_PROP_PATTERN;
constexpr uint32_t VEL_GROUPS = PBX_PROP_COV | PBX_PROP_ANGMOM | PBX_PROP_KAPPA |
                                PBX_PROP_KAPPA_MEAN | PBX_PROP_PATTERN;
constexpr uint32_t ALL_GROUPS = 127u;

// The predicate of one pass.  The contract is select_xyz / in_family of
// profile.hip (pbx_profile_select): a particle is kept when it lies in one of
// the family ranges (or none are given) and (use_sphere == 0 or
// ((dx*dx + dy*dy) + dz*dz) < r2max, strict, no FMA contraction).  Particles
// are indexed relative to `base` (the first particle of the families' span):
// the arrays a kernel receives start there.
struct PropParams {
  int use_sphere;
  int nfam;
  int64_t base, span;
  double cx, cy, cz, r2max;
  int64_t fam_lo[MAX_FAM];
  int64_t fam_hi[MAX_FAM];
};

__device__ __forceinline__ bool prop_in_family(int64_t i, const PropParams &p) {
  if (p.nfam == 0) return true;
  bool in = false;
  for (int f = 0; f < p.nfam; ++f) in |= (i >= p.fam_lo[f]) & (i < p.fam_hi[f]);
  return in;
}

__device__ __forceinline__ bool prop_in_sphere(double x, double y, double z, const PropParams &p) {
#pragma clang fp contract(off)
  const double dx = x - p.cx, dy = y - p.cy, dz = z - p.cz;
  return ((dx * dx + dy * dy) + dz * dz) < p.r2max;
}

// One pass over the particles [base, base + span).  POS / VEL: the pass
// reads positions / velocities at all (a sphere or a position group; a
// velocity group).  FRAME: what was read is taken to the frame `fr` before
// the sphere test and the terms (frame.h); without it fr is not looked at and
// the pass is the frame-less one.  REGION (POS only): the clauses of rg are
// ANDed into the predicate on the same coordinates (region.h); without it rg
// is not looked at and the pass is the region-less one.  part: one row of NS
// sums per block; cnt: its count.
template <bool POS, bool VEL, bool FRAME, bool REGION = false>
__global__ void __launch_bounds__(PROP_TPB)
    property_moments(const double *__restrict__ pos, const double *__restrict__ vel,
                     const double *__restrict__ mass, PropParams p, Frame fr, Region rg,
                     uint32_t groups, double *__restrict__ part, long long *__restrict__ cnt) {
#pragma clang fp contract(off)
  __shared__ double ws[PROP_NW][NS];
  __shared__ long long wc[PROP_NW];
  double acc[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) acc[k] = 0.0;
  long long c = 0;
  const int64_t stride = (int64_t)gridDim.x * PROP_TPB;
  for (int64_t j0 = (int64_t)blockIdx.x * PROP_TPB + threadIdx.x; j0 < p.span;
       j0 += stride * PROP_ITEMS) {
    double x[PROP_ITEMS], y[PROP_ITEMS], z[PROP_ITEMS];
    double vx[PROP_ITEMS], vy[PROP_ITEMS], vz[PROP_ITEMS], m[PROP_ITEMS];
    bool keep[PROP_ITEMS];
    // every load of the sweep in flight at once (a particle outside the span
    // or the families reads particle 0 of the span: no branch, no extra line)
#pragma unroll
    for (int k = 0; k < PROP_ITEMS; ++k) {
      const int64_t j = j0 + k * stride;
      keep[k] = (j < p.span) && prop_in_family(p.base + j, p);
      const int64_t jj = keep[k] ? j : 0;
      if constexpr (POS) {
        const double *q = pos + 3 * jj;
        x[k] = q[0];
        y[k] = q[1];
        z[k] = q[2];
      }
      if constexpr (VEL) {
        const double *q = vel + 3 * jj;
        vx[k] = q[0];
        vy[k] = q[1];
        vz[k] = q[2];
      }
    }
    if constexpr (FRAME) {
#pragma unroll
      for (int k = 0; k < PROP_ITEMS; ++k) {
        if constexpr (POS) frame_apply(fr.pos, x[k], y[k], z[k]);
        if constexpr (VEL) frame_apply(fr.vel, vx[k], vy[k], vz[k]);
      }
    }
    if (p.use_sphere) {
#pragma unroll
      for (int k = 0; k < PROP_ITEMS; ++k) keep[k] = keep[k] && prop_in_sphere(x[k], y[k], z[k], p);
    }
    if constexpr (REGION && POS) {
#pragma unroll
      for (int k = 0; k < PROP_ITEMS; ++k) keep[k] = keep[k] & region_keep(rg, x[k], y[k], z[k]);
    }
    // the masses of the kept particles only
#pragma unroll
    for (int k = 0; k < PROP_ITEMS; ++k) {
      m[k] = 1.0;
      if (mass && keep[k]) m[k] = mass[j0 + k * stride];
    }
#pragma unroll
    for (int k = 0; k < PROP_ITEMS; ++k) {
      if (!keep[k]) continue;  // (predicated: an unkept particle's NaN never meets a sum)
      const double mm = m[k];
      c += 1;
      if (groups & PBX_PROP_MASS) acc[0] = acc[0] + mm;
      if (POS && (groups & PBX_PROP_COM)) {
        acc[1] = acc[1] + x[k] * mm;
        acc[2] = acc[2] + y[k] * mm;
        acc[3] = acc[3] + z[k] * mm;
      }
      if (VEL && (groups & PBX_PROP_COV)) {
        acc[4] = acc[4] + vx[k] * mm;
        acc[5] = acc[5] + vy[k] * mm;
        acc[6] = acc[6] + vz[k] * mm;
      }
      if (POS && VEL) {
        if (groups & PBX_PROP_ANGMOM) {
          acc[7] = acc[7] + mm * (y[k] * vz[k] - z[k] * vy[k]);
          acc[8] = acc[8] + mm * (z[k] * vx[k] - x[k] * vz[k]);
          acc[9] = acc[9] + mm * (x[k] * vy[k] - y[k] * vx[k]);
        }
        if (groups & (PBX_PROP_KAPPA | PBX_PROP_KAPPA_MEAN)) {
          // 0/0 on the z axis and ke == 0 give numpy's NaN / inf
          const double vc = (x[k] * vy[k] - y[k] * vx[k]) / __builtin_sqrt(x[k] * x[k] + y[k] * y[k]);
          const double ke = 0.5 * ((vx[k] * vx[k] + vy[k] * vy[k]) + vz[k] * vz[k]);
          if (groups & PBX_PROP_KAPPA) {
            acc[10] = acc[10] + (0.5 * mm) * (vc * vc);
            acc[11] = acc[11] + mm * ke;
          }
          if (groups & PBX_PROP_KAPPA_MEAN) acc[12] = acc[12] + (0.5 * (vc * vc)) / ke;
        }
        if (groups & PBX_PROP_PATTERN) {
          acc[13] = acc[13] + (mm * x[k]) * x[k];
          acc[14] = acc[14] + (mm * y[k]) * y[k];
          acc[15] = acc[15] + (mm * x[k]) * y[k];
          acc[16] = acc[16] + mm * (x[k] * vy[k] + y[k] * vx[k]);
          acc[17] = acc[17] + mm * (x[k] * vx[k] - y[k] * vy[k]);
        }
      }
    }
  }
  // lanes of a wave: the xor butterfly (both partners add the same two
  // values, so every lane ends with the same bits)
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    double v = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    acc[k] = v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c = c + __shfl_xor(c, o, 64);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NS; ++k) ws[w][k] = acc[k];
    wc[w] = c;
  }
  __syncthreads();
  // waves of the block, in wave order
  if (threadIdx.x < NS) {
    double s = ws[0][threadIdx.x];
    for (int ww = 1; ww < PROP_NW; ++ww) s = s + ws[ww][threadIdx.x];
    part[(int64_t)blockIdx.x * NS + threadIdx.x] = s;
  } else if (threadIdx.x == NS) {
    long long s = 0;
    for (int ww = 0; ww < PROP_NW; ++ww) s += wc[ww];
    cnt[blockIdx.x] = s;
  }
}

// The rows of one pass in a fixed order: partial g = rows g, g + PROP_RG,
// ... in turn, then the partials in g order.  out: NS doubles, then the
// count as an int64.  One block of PROP_RG * PROP_NOUT threads.
__global__ void __launch_bounds__(PROP_RG *PROP_NOUT)
    property_reduce(const double *__restrict__ part, const long long *__restrict__ cnt, int rows,
                    double *__restrict__ out) {
  __shared__ double gs[PROP_RG][NS];
  __shared__ long long gc[PROP_RG];
  const int g = threadIdx.x / PROP_NOUT, col = threadIdx.x % PROP_NOUT;
  if (col < NS) {
    double s = 0.0;
    for (int r = g; r < rows; r += PROP_RG) s = s + part[(int64_t)r * NS + col];
    gs[g][col] = s;
  } else {
    long long s = 0;
    for (int r = g; r < rows; r += PROP_RG) s += cnt[r];
    gc[g] = s;
  }
  __syncthreads();
  if (g != 0) return;
  if (col < NS) {
    double s = 0.0;
    for (int k = 0; k < PROP_RG; ++k) s = s + gs[k][col];
    out[col] = s;
  } else {
    long long s = 0;
    for (int k = 0; k < PROP_RG; ++k) s += gc[k];
    ((long long *)out)[NS] = s;
  }
}

// ------------------------------------------------------------------- host
// blocks of a pass over `span` particles (a function of span alone)
static int grid_of(int64_t span) {
  const int64_t per = (int64_t)PROP_TPB * PROP_ITEMS;
  return (int)std::min<int64_t>((span + per - 1) / per, PROP_MAX_BLOCKS);
}

struct Span {
  int64_t lo, hi;
};

// the span [lo, hi) of n particles that holds every family member (no families: all)
static Span family_span(int64_t n, const int64_t *fam, int nfam) {
  if (nfam <= 0) return {0, n};
  int64_t lo = n, hi = 0;
  for (int f = 0; f < nfam; ++f) {
    const int64_t a = std::max<int64_t>(0, fam[2 * f]), b = std::min<int64_t>(n, fam[2 * f + 1]);
    if (b > a) {
      lo = std::min(lo, a);
      hi = std::max(hi, b);
    }
  }
  if (hi <= lo) lo = hi = 0;
  return {lo, hi};
}

static void check_common(int64_t n, const int64_t *fam, int nfam) {
  if (n < 0) fail(PBX_ERR_VALUE, "negative length");
  if (nfam < 0 || nfam > MAX_FAM) fail(PBX_ERR_VALUE, "at most %d family ranges", MAX_FAM);
  if (nfam > 0 && !fam) fail(PBX_ERR_VALUE, "family ranges are NULL");
}

// The particles of a pass on the device, starting at the span's first
// particle: the caller's device arrays, or host arrays staged through the
// pinned ring (only the span crosses PCIe).
struct Staged {
  PropParams p{};
  const double *pos = nullptr, *vel = nullptr, *mass = nullptr;
  Frame fr{};  // (all flags off: the frame-less kernels)
  Region rg{};  // (no clauses: the region-less kernels)
};

static const double *stage(Device &d, hipStream_t st, const double *a, int width, int64_t lo,
                           int64_t span, int on_device, int slot) {
  if (!a) return nullptr;
  const double *src = a + (size_t)width * (size_t)lo;
  if (on_device || span == 0) return src;
  const size_t bytes = sizeof(double) * (size_t)width * (size_t)span;
  double *dst = (double *)d.slot(slot).ensure(bytes);
  h2d_staged(d, dst, src, bytes, st);
  return dst;
}

static Staged stage_particles(Device &d, hipStream_t st, const double *pos, const double *vel,
                              const double *mass, int64_t n, int on_device, const int64_t *fam,
                              int nfam) {
  Staged s;
  const Span sp = family_span(n, fam, nfam);
  s.p.nfam = nfam;
  s.p.base = sp.lo;
  s.p.span = sp.hi - sp.lo;
  for (int f = 0; f < nfam; ++f) {
    s.p.fam_lo[f] = fam[2 * f];
    s.p.fam_hi[f] = fam[2 * f + 1];
  }
  s.pos = stage(d, st, pos, 3, sp.lo, s.p.span, on_device, kSlotPropPos);
  s.vel = stage(d, st, vel, 3, sp.lo, s.p.span, on_device, kSlotPropVel);
  s.mass = stage(d, st, mass, 1, sp.lo, s.p.span, on_device, kSlotPropMass);
  return s;
}

// one pass + its reduction + the read-back (one stream sync)
static void run_pass(Device &d, hipStream_t st, const Staged &s, uint32_t groups, int64_t *n_kept,
                     double *sums) {
  *n_kept = 0;
  for (int k = 0; k < NS; ++k) sums[k] = 0.0;
  if (s.p.span <= 0) return;
  const int grid = grid_of(s.p.span);
  // [rows of sums][counts][the result]
  double *part = (double *)d.slot(kSlotPropPart)
                     .ensure(sizeof(double) * ((size_t)PROP_MAX_BLOCKS * (NS + 1) + PROP_NOUT));
  long long *cnt = (long long *)(part + (size_t)PROP_MAX_BLOCKS * NS);
  double *out = part + (size_t)PROP_MAX_BLOCKS * (NS + 1);
  const bool use_pos = s.p.use_sphere || s.rg.any() || (groups & POS_GROUPS);
  const bool use_vel = (groups & VEL_GROUPS) != 0;
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(PROP_TPB), 0, st, s.pos, s.vel, s.mass, s.p, s.fr,
                       s.rg, groups, part, cnt);
  };
  // (a frame half whose array the pass does not read changes nothing)
  const bool framed = (use_pos && (s.fr.pos.shift || s.fr.pos.rot)) ||
                      (use_vel && (s.fr.vel.shift || s.fr.vel.rot));
  if (s.rg.any()) {  // (a region reads positions)
    if (framed) {
      if (use_vel) launch(property_moments<true, true, true, true>);
      else launch(property_moments<true, false, true, true>);
    } else if (use_vel) launch(property_moments<true, true, false, true>);
    else launch(property_moments<true, false, false, true>);
  } else if (framed) {
    if (use_pos && use_vel) launch(property_moments<true, true, true>);
    else if (use_pos) launch(property_moments<true, false, true>);
    else launch(property_moments<false, true, true>);
  } else if (use_pos && use_vel) launch(property_moments<true, true, false>);
  else if (use_pos) launch(property_moments<true, false, false>);
  else if (use_vel) launch(property_moments<false, true, false>);
  else launch(property_moments<false, false, false>);
  PBX_HIP(hipGetLastError());
  hipLaunchKernelGGL(property_reduce, dim3(1), dim3(PROP_RG * PROP_NOUT), 0, st, part, cnt, grid,
                     out);
  PBX_HIP(hipGetLastError());
  double h[PROP_NOUT];
  PBX_HIP(hipMemcpyAsync(h, out, sizeof(h), hipMemcpyDeviceToHost, st));
  PBX_HIP(hipStreamSynchronize(st));
  std::memcpy(sums, h, sizeof(double) * NS);
  std::memcpy(n_kept, &h[NS], sizeof(int64_t));
}

}  // namespace prop
}  // namespace pbx

using namespace pbx;
using namespace pbx::prop;

extern "C" {

int pbx_property_moments_region(const double *pos, const double *vel, const double *mass,
                                int64_t n, int on_device, int use_sphere, const double *sphere,
                                const int64_t *fam, int nfam, uint32_t groups, int flags,
                                const double *frame, int nclauses, const int *kinds,
                                const int *negate, const double *params, int64_t *n_kept,
                                double *h_sums) {
  return guard([&] {
    const Region rg = region_of(nclauses, kinds, negate, params);
    if (flags & ~(PBX_FRAME_POS | PBX_FRAME_VEL | PBX_FRAME_ROT))
      fail(PBX_ERR_VALUE, "flags must be a mask of PBX_FRAME_* bits (got 0x%x)", flags);
    if (!n_kept || !h_sums) fail(PBX_ERR_VALUE, "null output");
    check_common(n, fam, nfam);
    if (groups == 0 || (groups & ~ALL_GROUPS))
      fail(PBX_ERR_VALUE, "groups must be a non-empty mask of PBX_PROP_* bits (got 0x%x)", groups);
    if ((groups & VEL_GROUPS) && !vel)
      fail(PBX_ERR_VALUE, "the requested groups read velocities: vel is NULL");
    if (use_sphere && !sphere) fail(PBX_ERR_VALUE, "use_sphere without a sphere");
    if ((use_sphere || rg.any() || (groups & POS_GROUPS)) && !pos)
      fail(PBX_ERR_VALUE, "a sphere, a region or the requested groups read positions: pos is NULL");
    Device &d = current_device();
    std::lock_guard<std::mutex> lk(d.mu);
    hipStream_t st = d.stream;
    ScopedTimer tm("pbx.property.moments");
    const bool use_pos = use_sphere || rg.any() || (groups & POS_GROUPS);
    const bool use_vel = (groups & VEL_GROUPS) != 0;
    Staged s = stage_particles(d, st, use_pos ? pos : nullptr, use_vel ? vel : nullptr, mass, n,
                               on_device, fam, nfam);
    if (use_sphere) {
      s.p.use_sphere = 1;
      s.p.cx = sphere[0];
      s.p.cy = sphere[1];
      s.p.cz = sphere[2];
      s.p.r2max = sphere[3];
    }
    s.fr = frame_of(flags, frame);
    s.rg = rg;
    run_pass(d, st, s, groups, n_kept, h_sums);
  });
}

int pbx_property_moments_frame(const double *pos, const double *vel, const double *mass, int64_t n,
                               int on_device, int use_sphere, const double *sphere,
                               const int64_t *fam, int nfam, uint32_t groups, int flags,
                               const double *frame, int64_t *n_kept, double *h_sums) {
  return pbx_property_moments_region(pos, vel, mass, n, on_device, use_sphere, sphere, fam, nfam,
                                     groups, flags, frame, 0, nullptr, nullptr, nullptr, n_kept,
                                     h_sums);
}

int pbx_property_moments(const double *pos, const double *vel, const double *mass, int64_t n,
                         int on_device, int use_sphere, const double *sphere, const int64_t *fam,
                         int nfam, uint32_t groups, int64_t *n_kept, double *h_sums) {
  return pbx_property_moments_frame(pos, vel, mass, n, on_device, use_sphere, sphere, fam, nfam,
                                    groups, 0, nullptr, n_kept, h_sums);
}

int pbx_property_shrink_center(const double *pos, const double *mass, int64_t n, int on_device,
                               const int64_t *fam, int nfam, double r0, double shrink_factor,
                               int64_t min_particles, double *h_cen, int64_t *iterations,
                               int64_t *n_last) {
  return guard([&] {
    if (!h_cen || !iterations || !n_last) fail(PBX_ERR_VALUE, "null output");
    check_common(n, fam, nfam);
    if (!(r0 > 0.0)) fail(PBX_ERR_VALUE, "r0 must be positive (got %g)", r0);
    if (!(shrink_factor > 0.0 && shrink_factor < 1.0))
      fail(PBX_ERR_VALUE, "shrink_factor must lie in (0, 1) (got %g)", shrink_factor);
    if (min_particles < 1)
      fail(PBX_ERR_VALUE, "min_particles must be >= 1 (got %lld)", (long long)min_particles);
    if (!pos) fail(PBX_ERR_VALUE, "pos is NULL");
    Device &d = current_device();
    std::lock_guard<std::mutex> lk(d.mu);
    hipStream_t st = d.stream;
    ScopedTimer tm("pbx.property.shrink_center");
    // staged once; every iteration re-reads them from HBM
    Staged s = stage_particles(d, st, pos, nullptr, mass, n, on_device, fam, nfam);
    const uint32_t groups = PBX_PROP_MASS | PBX_PROP_COM;
    int64_t c = 0, it = 0;
    double sums[NS];
    run_pass(d, st, s, groups, &c, sums);
    double com[3] = {sums[1] / sums[0], sums[2] / sums[0], sums[3] / sums[0]};
    int64_t last = c;
    double r = r0;
    s.p.use_sphere = 1;
    for (;;) {
      // (r reaches 0 and the sphere empties eventually; a factor close to 1
      // could take 10^9 passes to get there)
      if (it >= MAX_SHRINK_ITER)
        fail(PBX_ERR_RUNTIME, "shrinking sphere: more than %d iterations", MAX_SHRINK_ITER);
      s.p.cx = com[0];
      s.p.cy = com[1];
      s.p.cz = com[2];
      s.p.r2max = r * r;
      run_pass(d, st, s, groups, &c, sums);
      if (c <= min_particles) break;  // (a NaN centre keeps nothing: ends here)
      for (int k = 0; k < 3; ++k) com[k] = sums[1 + k] / sums[0];
      last = c;
      r *= shrink_factor;
      ++it;
    }
    for (int k = 0; k < 3; ++k) h_cen[k] = com[k];
    *iterations = it;
    *n_last = last;
  });
}

}  // extern "C"
