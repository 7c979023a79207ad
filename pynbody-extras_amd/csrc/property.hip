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
// is not looked at and the pass is the region-less one.  WRAP (FRAME and POS
// only): the frame holds a periodic wrap; without it the kernel takes
// FrameK<false>, the argument block it had before the wrap existed.  part: one
// row of NS sums per block; cnt: its count.
template <bool POS, bool VEL, bool FRAME, bool REGION = false, bool WRAP = false>
__global__ void __launch_bounds__(PROP_TPB)
    property_moments(const double *__restrict__ pos, const double *__restrict__ vel,
                     const double *__restrict__ mass, PropParams p, FrameK<WRAP> fr, Region rg,
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
        if constexpr (POS) frame_apply_pos(fr, x[k], y[k], z[k]);
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

// --------------------------------------------------------- enclosed sums
// pbx_property_enclosed: Σ m and the count of the kept particles with
// r < t[j] for up to ENC_MAX thresholds, and the extrema of x, y, z, r, in
// one read of pos / mass (32 bytes per particle whatever the number of
// thresholds: they are kernel arguments, their accumulators registers).  No
// sqrt is taken on the device: the host turns a threshold t into the exact
// bound on the squared radius (enc_square_bound).  The grid, the particle -> thread mapping, the order in which a thread adds and
// the three reduction steps are those of property_moments / property_reduce,
// so a threshold's sum has the bits of that pass's mass sum over the same n
// particles with the masses outside the threshold replaced by 0.0.
constexpr int ENC_MAX = PBX_ENCLOSED_MAX;    // thresholds of one pass
constexpr int ENC_NEXT = PBX_ENCLOSED_NEXT;  // min x, max x, min y, max y, min z, max z, max r
constexpr int ENC_NCNT = ENC_MAX + 1;        // the thresholds' counts, then the kept count
constexpr int ENC_RCOLS = 32;                // columns of enclosed_reduce (>= ENC_NCNT)
constexpr int ENC_NOUT = ENC_MAX + ENC_NEXT + ENC_NCNT;  // 8-byte words of a result
static_assert(ENC_NCNT <= ENC_RCOLS && ENC_NEXT <= ENC_RCOLS, "enclosed_reduce columns");
static_assert(64 + ENC_NCNT <= 128 && 128 + ENC_NEXT <= PROP_TPB, "writer threads of a block");

template <int NTC>
struct EncThresholds {
  double t[NTC];  // (unused slots NaN: nothing is below them)
};

// the rows of partials of one pass (a row per block) and its result
struct EncPart {
  double *sum;     // [PROP_MAX_BLOCKS][ENC_MAX]
  double *ext;     // [PROP_MAX_BLOCKS][ENC_NEXT]
  long long *cnt;  // [PROP_MAX_BLOCKS][ENC_NCNT]
};

// numpy's min / max of two values: a NaN wins (and stays)
__device__ __forceinline__ double enc_min(double a, double v) { return (v < a || v != v) ? v : a; }
__device__ __forceinline__ double enc_max(double a, double v) { return (v > a || v != v) ? v : a; }
__device__ __forceinline__ double enc_fold(int col, double a, double v) {
  return (col < 6 && !(col & 1)) ? enc_min(a, v) : enc_max(a, v);
}
__device__ __forceinline__ double enc_identity(int col) {
  return (col < 6 && !(col & 1)) ? __builtin_inf() : -__builtin_inf();
}

// NTC: the thresholds the instantiation holds (nt rounded up to 2^L - 1).
// FRAME / REGION / WRAP as in property_moments.  want_ext (uniform): the
// extrema.
template <int NTC, bool FRAME, bool REGION, bool WRAP = false>
__global__ void __launch_bounds__(PROP_TPB)
    property_enclosed(const double *__restrict__ pos, const double *__restrict__ mass, PropParams p,
                      FrameK<WRAP> fr, Region rg, EncThresholds<NTC> th, int want_ext,
                      EncPart out) {
#pragma clang fp contract(off)
  __shared__ double ws[PROP_NW][NTC];
  __shared__ long long wc[PROP_NW][NTC + 1];
  __shared__ double we[PROP_NW][ENC_NEXT];
  double acc[NTC];
  unsigned cn[NTC];  // (a thread sees span / (grid * PROP_TPB) particles: 32 bits hold it)
#pragma unroll
  for (int j = 0; j < NTC; ++j) {
    acc[j] = 0.0;
    cn[j] = 0;
  }
  unsigned c = 0;
  double ex[ENC_NEXT];
#pragma unroll
  for (int e = 0; e < ENC_NEXT; ++e) ex[e] = enc_identity(e);
  const int64_t stride = (int64_t)gridDim.x * PROP_TPB;
  for (int64_t j0 = (int64_t)blockIdx.x * PROP_TPB + threadIdx.x; j0 < p.span;
       j0 += stride * PROP_ITEMS) {
    double x[PROP_ITEMS], y[PROP_ITEMS], z[PROP_ITEMS], m[PROP_ITEMS];
    bool keep[PROP_ITEMS];
    // (as property_moments: every load of the sweep in flight, an unkept
    // particle reads particle 0 of the span)
#pragma unroll
    for (int k = 0; k < PROP_ITEMS; ++k) {
      const int64_t j = j0 + k * stride;
      keep[k] = (j < p.span) && prop_in_family(p.base + j, p);
      const double *q = pos + 3 * (keep[k] ? j : 0);
      x[k] = q[0];
      y[k] = q[1];
      z[k] = q[2];
    }
    if constexpr (FRAME) {
#pragma unroll
      for (int k = 0; k < PROP_ITEMS; ++k) frame_apply_pos(fr, x[k], y[k], z[k]);
    }
    if (p.use_sphere) {
#pragma unroll
      for (int k = 0; k < PROP_ITEMS; ++k) keep[k] = keep[k] && prop_in_sphere(x[k], y[k], z[k], p);
    }
    if constexpr (REGION) {
#pragma unroll
      for (int k = 0; k < PROP_ITEMS; ++k) keep[k] = keep[k] & region_keep(rg, x[k], y[k], z[k]);
    }
#pragma unroll
    for (int k = 0; k < PROP_ITEMS; ++k) {
      m[k] = 1.0;
      if (mass && keep[k]) m[k] = mass[j0 + k * stride];
    }
    // The squared radius only: th.t[j] is the smallest double whose correctly
    // rounded sqrt reaches the caller's threshold (enc_square_bound), so
    // r2 < th.t[j] is sqrt(r2) < threshold exactly, and max r is the sqrt of
    // max r2 (the host takes it).  Everything below is predicated, not
    // branched.
    double r2[PROP_ITEMS];
#pragma unroll
    for (int k = 0; k < PROP_ITEMS; ++k) {
      r2[k] = (x[k] * x[k] + y[k] * y[k]) + z[k] * z[k];
      c += keep[k];
    }
    // (threshold by threshold: an accumulator still adds its particles in
    // index order, and a threshold is live for four compares only)
#pragma unroll
    for (int j = 0; j < NTC; ++j) {
      const double tj = th.t[j];
#pragma unroll
      for (int k = 0; k < PROP_ITEMS; ++k) {
        const bool in = keep[k] & (r2[k] < tj);  // (a NaN on either side: false)
        acc[j] = acc[j] + (in ? m[k] : 0.0);
        cn[j] += in;
      }
    }
    if (want_ext) {
#pragma unroll
      for (int k = 0; k < PROP_ITEMS; ++k) {
        const bool kp = keep[k];
        ex[0] = kp ? enc_min(ex[0], x[k]) : ex[0];
        ex[1] = kp ? enc_max(ex[1], x[k]) : ex[1];
        ex[2] = kp ? enc_min(ex[2], y[k]) : ex[2];
        ex[3] = kp ? enc_max(ex[3], y[k]) : ex[3];
        ex[4] = kp ? enc_min(ex[4], z[k]) : ex[4];
        ex[5] = kp ? enc_max(ex[5], z[k]) : ex[5];
        ex[6] = kp ? enc_max(ex[6], r2[k]) : ex[6];
      }
    }
  }
  // lanes of a wave: the xor butterfly of property_moments
  // (a wave's counts still fit 32 bits)
#pragma unroll
  for (int j = 0; j < NTC; ++j) {
    double v = acc[j];
    unsigned u = cn[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      v = v + __shfl_xor(v, o, 64);
      u = u + __shfl_xor(u, o, 64);
    }
    acc[j] = v;
    cn[j] = u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c = c + __shfl_xor(c, o, 64);
  if (want_ext) {
#pragma unroll
    for (int e = 0; e < ENC_NEXT; ++e) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) ex[e] = enc_fold(e, ex[e], __shfl_xor(ex[e], o, 64));
    }
  }
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < NTC; ++j) ws[w][j] = acc[j];
#pragma unroll
    for (int j = 0; j < NTC; ++j) wc[w][j] = cn[j];
    wc[w][NTC] = c;
#pragma unroll
    for (int e = 0; e < ENC_NEXT; ++e) we[w][e] = ex[e];
  }
  __syncthreads();
  // waves of the block, in wave order: sums by the first wave's threads,
  // counts by the second's, extrema by the third's
  const int t = threadIdx.x;
  if (t < NTC) {
    double s = ws[0][t];
    for (int ww = 1; ww < PROP_NW; ++ww) s = s + ws[ww][t];
    out.sum[(int64_t)blockIdx.x * ENC_MAX + t] = s;
  } else if (t >= 64 && t < 64 + NTC + 1) {
    const int j = t - 64;
    long long s = 0;
    for (int ww = 0; ww < PROP_NW; ++ww) s += wc[ww][j];
    // (the kept count sits in the last column whatever NTC is)
    out.cnt[(int64_t)blockIdx.x * ENC_NCNT + (j == NTC ? ENC_MAX : j)] = s;
  } else if (want_ext && t >= 128 && t < 128 + ENC_NEXT) {
    const int e = t - 128;
    double s = we[0][e];
    for (int ww = 1; ww < PROP_NW; ++ww) s = enc_fold(e, s, we[ww][e]);
    out.ext[(int64_t)blockIdx.x * ENC_NEXT + e] = s;
  }
}

// The rows of an enclosed pass in the order of property_reduce: partial g =
// rows g, g + PROP_RG, ... in turn, then the partials in g order.  res:
// ENC_MAX sums, ENC_NEXT extrema, ENC_NCNT counts (columns >= nt untouched).
// Blocks of PROP_RG * ENC_RCOLS threads: block 0 folds the sums, block 1 the
// counts, block 2 (launched only when they are wanted) the extrema.  A thread
// has all of its at most ENC_RPT rows in flight before it folds them in row
// order: one load latency, not one per row.
constexpr int ENC_RPT = PROP_MAX_BLOCKS / PROP_RG;  // rows of one partial

template <class T, class Fold>
__device__ __forceinline__ T enc_fold_rows(const T *__restrict__ col0, int stride, int g, int rows,
                                           T init, Fold fold) {
  T v[ENC_RPT];
#pragma unroll
  for (int i = 0; i < ENC_RPT; ++i) {
    const int r = g + i * PROP_RG;
    v[i] = col0[(int64_t)(r < rows ? r : 0) * stride];
  }
  T s = init;
#pragma unroll
  for (int i = 0; i < ENC_RPT; ++i)
    if (g + i * PROP_RG < rows) s = fold(s, v[i]);
  return s;
}

__global__ void __launch_bounds__(PROP_RG *ENC_RCOLS)
    enclosed_reduce(EncPart part, int rows, int nt, double *__restrict__ res) {
  __shared__ double gd[PROP_RG][ENC_RCOLS];
  __shared__ long long gc[PROP_RG][ENC_RCOLS];
  const int g = threadIdx.x / ENC_RCOLS, col = threadIdx.x % ENC_RCOLS;
  const auto add = [](double a, double b) { return a + b; };
  if (blockIdx.x == 0) {  // the sums
    if (col < nt) gd[g][col] = enc_fold_rows(part.sum + col, ENC_MAX, g, rows, 0.0, add);
    __syncthreads();
    if (g != 0 || col >= nt) return;
    double s = 0.0;
    for (int k = 0; k < PROP_RG; ++k) s = s + gd[k][col];
    res[col] = s;
  } else if (blockIdx.x == 1) {  // the thresholds' counts and the kept count
    const bool has = col < nt || col == ENC_MAX;
    if (has)
      gc[g][col] = enc_fold_rows(part.cnt + col, ENC_NCNT, g, rows, 0ll,
                                 [](long long a, long long b) { return a + b; });
    __syncthreads();
    if (g != 0 || !has) return;
    long long s = 0;
    for (int k = 0; k < PROP_RG; ++k) s += gc[k][col];
    ((long long *)res)[ENC_MAX + ENC_NEXT + col] = s;
  } else {  // the extrema
    const bool has = col < ENC_NEXT;
    const auto fold = [col](double a, double b) { return enc_fold(col, a, b); };
    if (has) gd[g][col] = enc_fold_rows(part.ext + col, ENC_NEXT, g, rows, enc_identity(col), fold);
    __syncthreads();
    if (g != 0 || !has) return;
    double s = enc_identity(col);
    for (int k = 0; k < PROP_RG; ++k) s = enc_fold(col, s, gd[k][col]);
    res[ENC_MAX + col] = s;
  }
}

// ----------------------------------------------------------- wrap extents
// pbx_property_wrap_extents: what WrapBox("minirange") asks of the particles
// before it can choose a convention per axis.  One read of pos[0:n] (24 bytes
// per particle), no predicate; per axis both candidate wraps of frame.h
// (lo = -0.5 * L and lo = 0.0) and their min / max with numpy's NaN rule.
// Column 4 * axis + {0 min wc, 1 max wc, 2 min wu, 3 max wu}.  The grid, the
// particle -> thread mapping and the three fold steps are those of
// property_enclosed's extrema; a min / max does not depend on the order, so
// the result depends on the particles alone.
constexpr int WEXT_N = 12;
constexpr int WEXT_RCOLS = 16;  // columns of wrap_extents_reduce (>= WEXT_N)
static_assert(WEXT_N <= WEXT_RCOLS && WEXT_N <= PROP_TPB, "wrap extents columns");

__device__ __forceinline__ double wext_fold(int col, double a, double v) {
  return (col & 1) ? enc_max(a, v) : enc_min(a, v);
}
__device__ __forceinline__ double wext_identity(int col) {
  return (col & 1) ? -__builtin_inf() : __builtin_inf();
}

__global__ void __launch_bounds__(PROP_TPB)
    property_wrap_extents(const double *__restrict__ pos, int64_t n, FrameHalf sh, double L,
                          double lo_c, double *__restrict__ part) {  // (sh: its shift only)
#pragma clang fp contract(off)
  __shared__ double we[PROP_NW][WEXT_N];
  double ex[WEXT_N];
#pragma unroll
  for (int e = 0; e < WEXT_N; ++e) ex[e] = wext_identity(e);
  const int64_t stride = (int64_t)gridDim.x * PROP_TPB;
  for (int64_t j0 = (int64_t)blockIdx.x * PROP_TPB + threadIdx.x; j0 < n;
       j0 += stride * PROP_ITEMS) {
    double v[PROP_ITEMS][3];
    bool in[PROP_ITEMS];
    // (as property_enclosed: every load of the sweep in flight, a slot past
    // the end reads particle 0 and is folded into nothing)
#pragma unroll
    for (int k = 0; k < PROP_ITEMS; ++k) {
      const int64_t j = j0 + k * stride;
      in[k] = j < n;
      const double *q = pos + 3 * (in[k] ? j : 0);
      v[k][0] = q[0];
      v[k][1] = q[1];
      v[k][2] = q[2];
    }
#pragma unroll
    for (int k = 0; k < PROP_ITEMS; ++k) {
      if (sh.shift) {  // (uniform)
        v[k][0] = v[k][0] - sh.c[0];
        v[k][1] = v[k][1] - sh.c[1];
        v[k][2] = v[k][2] - sh.c[2];
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        // the wrap step of frame_apply with either lower bound
        const double x = v[k][a];
        const double wc = x - (__builtin_floor((x - lo_c) / L) + 0.0) * L;
        const double wu = x - (__builtin_floor((x - 0.0) / L) + 0.0) * L;
        ex[4 * a + 0] = in[k] ? enc_min(ex[4 * a + 0], wc) : ex[4 * a + 0];
        ex[4 * a + 1] = in[k] ? enc_max(ex[4 * a + 1], wc) : ex[4 * a + 1];
        ex[4 * a + 2] = in[k] ? enc_min(ex[4 * a + 2], wu) : ex[4 * a + 2];
        ex[4 * a + 3] = in[k] ? enc_max(ex[4 * a + 3], wu) : ex[4 * a + 3];
      }
    }
  }
#pragma unroll
  for (int e = 0; e < WEXT_N; ++e) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ex[e] = wext_fold(e, ex[e], __shfl_xor(ex[e], o, 64));
  }
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
#pragma unroll
    for (int e = 0; e < WEXT_N; ++e) we[w][e] = ex[e];
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < WEXT_N) {
    double s = we[0][t];
    for (int ww = 1; ww < PROP_NW; ++ww) s = wext_fold(t, s, we[ww][t]);
    part[(int64_t)blockIdx.x * WEXT_N + t] = s;
  }
}

// the rows of a wrap-extents pass in the order of enclosed_reduce; one block
// of PROP_RG * WEXT_RCOLS threads, res: WEXT_N doubles
__global__ void __launch_bounds__(PROP_RG *WEXT_RCOLS)
    wrap_extents_reduce(const double *__restrict__ part, int rows, double *__restrict__ res) {
  __shared__ double gd[PROP_RG][WEXT_RCOLS];
  const int g = threadIdx.x / WEXT_RCOLS, col = threadIdx.x % WEXT_RCOLS;
  const bool has = col < WEXT_N;
  const auto fold = [col](double a, double b) { return wext_fold(col, a, b); };
  if (has) gd[g][col] = enc_fold_rows(part + col, WEXT_N, g, rows, wext_identity(col), fold);
  __syncthreads();
  if (g != 0 || !has) return;
  double s = wext_identity(col);
  for (int k = 0; k < PROP_RG; ++k) s = wext_fold(col, s, gd[k][col]);
  res[col] = s;
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
    hipLaunchKernelGGL(kern, dim3(grid), dim3(PROP_TPB), 0, st, s.pos, s.vel, s.mass, s.p,
                       s.fr.k<false>(), s.rg, groups, part, cnt);
  };
  auto launch_wrap = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(PROP_TPB), 0, st, s.pos, s.vel, s.mass, s.p,
                       s.fr.k<true>(), s.rg, groups, part, cnt);
  };
  // (a frame half whose array the pass does not read changes nothing)
  const bool framed = (use_pos && s.fr.pos_any()) || (use_vel && s.fr.vel.any());
  if (use_pos && s.fr.wrap.on) {  // (the instantiations that carry the wrap's constants)
    if (s.rg.any()) {
      if (use_vel) launch_wrap(property_moments<true, true, true, true, true>);
      else launch_wrap(property_moments<true, false, true, true, true>);
    } else if (use_vel) launch_wrap(property_moments<true, true, true, false, true>);
    else launch_wrap(property_moments<true, false, true, false, true>);
  } else if (s.rg.any()) {  // (a region reads positions)
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

// what one enclosed pass returns (entries >= nt are not meaningful)
struct Enclosed {
  int64_t kept = 0;
  double msum[ENC_MAX];
  int64_t count[ENC_MAX];
  double ext[ENC_NEXT];
};

// The smallest double s >= +0 with sqrt(s) >= t (NaN for a NaN t; +0 for
// t <= 0: nothing is below it).  The correctly rounded sqrt is monotonic, so
// the s with sqrt(s) >= t are exactly those from this one up, and
// sqrt(r2) < t  <=>  r2 < enc_square_bound(t): the kernel takes no sqrt and
// decides every particle as the definition in pbx.h does.  Bisection over
// the bit patterns of the non-negative doubles, which order as their values.
static double enc_square_bound(double t) {
  if (t != t) return t;
  auto at = [](uint64_t b) {
    double v;
    std::memcpy(&v, &b, sizeof(v));
    return v;
  };
  uint64_t lo = 0, hi = 0x7ff0000000000000ull;  // +0 .. +inf
  if (std::sqrt(at(lo)) >= t) return 0.0;
  while (hi - lo > 1) {  // sqrt(at(lo)) < t <= sqrt(at(hi))
    const uint64_t mid = lo + (hi - lo) / 2;
    if (std::sqrt(at(mid)) >= t) hi = mid;
    else lo = mid;
  }
  return at(hi);
}

template <int NTC>
static void launch_enclosed(hipStream_t st, int grid, const Staged &s, int nt, const double *t,
                            int want_ext, const EncPart &part) {
  EncThresholds<NTC> th;
  for (int j = 0; j < NTC; ++j) th.t[j] = j < nt ? enc_square_bound(t[j]) : __builtin_nan("");
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(PROP_TPB), 0, st, s.pos, s.mass, s.p,
                       s.fr.k<false>(), s.rg, th, want_ext, part);
  };
  auto launch_wrap = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(PROP_TPB), 0, st, s.pos, s.mass, s.p,
                       s.fr.k<true>(), s.rg, th, want_ext, part);
  };
  const bool framed = s.fr.pos_any();
  if (s.fr.wrap.on) {
    if (s.rg.any()) launch_wrap(property_enclosed<NTC, true, true, true>);
    else launch_wrap(property_enclosed<NTC, true, false, true>);
  } else if (s.rg.any()) {
    if (framed) launch(property_enclosed<NTC, true, true>);
    else launch(property_enclosed<NTC, false, true>);
  } else if (framed) launch(property_enclosed<NTC, true, false>);
  else launch(property_enclosed<NTC, false, false>);
}

// one enclosed pass + its reduction + the read-back (one stream sync)
static void run_enclosed(Device &d, hipStream_t st, const Staged &s, int nt, const double *t,
                         bool want_ext, Enclosed &e) {
  e.kept = 0;
  for (int j = 0; j < ENC_MAX; ++j) {
    e.msum[j] = 0.0;
    e.count[j] = 0;
  }
  for (int k = 0; k < ENC_NEXT; ++k) e.ext[k] = __builtin_nan("");
  if (s.p.span <= 0) return;
  const int grid = grid_of(s.p.span);
  // [rows of sums][rows of extrema][rows of counts][the result]
  const size_t rows = PROP_MAX_BLOCKS;
  double *base = (double *)d.slot(kSlotPropPart)
                     .ensure(sizeof(double) * (rows * (ENC_MAX + ENC_NEXT + ENC_NCNT) + ENC_NOUT));
  EncPart part;
  part.sum = base;
  part.ext = part.sum + rows * ENC_MAX;
  part.cnt = (long long *)(part.ext + rows * ENC_NEXT);
  double *res = (double *)(part.cnt + rows * ENC_NCNT);
  // the instantiation that holds nt thresholds: 2^L - 1 of them
  if (nt <= 1) launch_enclosed<1>(st, grid, s, nt, t, want_ext, part);
  else if (nt <= 3) launch_enclosed<3>(st, grid, s, nt, t, want_ext, part);
  else if (nt <= 7) launch_enclosed<7>(st, grid, s, nt, t, want_ext, part);
  else if (nt <= 15) launch_enclosed<15>(st, grid, s, nt, t, want_ext, part);
  else launch_enclosed<ENC_MAX>(st, grid, s, nt, t, want_ext, part);
  PBX_HIP(hipGetLastError());
  // (blocks: the sums, the counts and, when wanted, the extrema)
  hipLaunchKernelGGL(enclosed_reduce, dim3(want_ext ? 3 : 2), dim3(PROP_RG * ENC_RCOLS), 0, st,
                     part, grid, nt, res);
  PBX_HIP(hipGetLastError());
  double h[ENC_NOUT];
  PBX_HIP(hipMemcpyAsync(h, res, sizeof(h), hipMemcpyDeviceToHost, st));
  PBX_HIP(hipStreamSynchronize(st));
  const int64_t *hc = (const int64_t *)(h + ENC_MAX + ENC_NEXT);
  e.kept = hc[ENC_MAX];
  for (int j = 0; j < nt; ++j) {
    e.msum[j] = h[j];
    e.count[j] = hc[j];
  }
  if (want_ext && e.kept > 0) {
    for (int k = 0; k < ENC_NEXT; ++k) e.ext[k] = h[ENC_MAX + k];
    e.ext[6] = std::sqrt(e.ext[6]);  // (max r = sqrt(max r2): sqrt is monotonic; a NaN stays)
  }
}

// the arguments the two enclosed entry points share, checked and staged
static Staged stage_scope(Device &d, hipStream_t st, const double *pos, const double *mass,
                          int64_t n, int on_device, int use_sphere, const double *sphere,
                          const int64_t *fam, int nfam, int flags, const double *frame,
                          const Region &rg) {
  Staged s = stage_particles(d, st, pos, nullptr, mass, n, on_device, fam, nfam);
  if (use_sphere) {
    s.p.use_sphere = 1;
    s.p.cx = sphere[0];
    s.p.cy = sphere[1];
    s.p.cz = sphere[2];
    s.p.r2max = sphere[3];
  }
  s.fr = frame_of(flags, frame);
  s.rg = rg;
  return s;
}

static void check_scope(const double *pos, int64_t n, int use_sphere, const double *sphere,
                        const int64_t *fam, int nfam, int flags, const double *frame) {
  (void)frame_of(flags, frame);  // (the flags and the wrap, before anything is staged)
  check_common(n, fam, nfam);
  if (use_sphere && !sphere) fail(PBX_ERR_VALUE, "use_sphere without a sphere");
  if (!pos) fail(PBX_ERR_VALUE, "pos is NULL");
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
    const Frame fr = frame_of(flags, frame);  // (checks the flags and the wrap)
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
    s.fr = fr;
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

int pbx_property_enclosed(const double *pos, const double *mass, int64_t n, int on_device,
                          int use_sphere, const double *sphere, const int64_t *fam, int nfam,
                          int flags, const double *frame, int nclauses, const int *kinds,
                          const int *negate, const double *params, int nt, const double *h_t,
                          int64_t *n_kept, double *h_msum, int64_t *h_count, double *h_ext) {
  return guard([&] {
    const Region rg = region_of(nclauses, kinds, negate, params);
    if (!n_kept) fail(PBX_ERR_VALUE, "null output");
    if (nt < 0 || nt > ENC_MAX)
      fail(PBX_ERR_VALUE, "nt must lie in [0, %d] (got %d)", ENC_MAX, nt);
    if (nt > 0 && (!h_t || !h_msum || !h_count))
      fail(PBX_ERR_VALUE, "thresholds without h_t, h_msum or h_count");
    check_scope(pos, n, use_sphere, sphere, fam, nfam, flags, frame);
    Device &d = current_device();
    std::lock_guard<std::mutex> lk(d.mu);
    hipStream_t st = d.stream;
    ScopedTimer tm("pbx.property.enclosed");
    const Staged s = stage_scope(d, st, pos, mass, n, on_device, use_sphere, sphere, fam, nfam,
                                 flags, frame, rg);
    Enclosed e;
    run_enclosed(d, st, s, nt, h_t, h_ext != nullptr, e);
    *n_kept = e.kept;
    for (int j = 0; j < nt; ++j) {
      h_msum[j] = e.msum[j];
      h_count[j] = e.count[j];
    }
    if (h_ext)
      for (int k = 0; k < ENC_NEXT; ++k) h_ext[k] = e.ext[k];
  });
}

int pbx_property_wrap_extents(const double *pos, int64_t n, int on_device, int flags,
                              const double *frame, double L, double *h_ext) {
  return guard([&] {
    if (!h_ext) fail(PBX_ERR_VALUE, "null output");
    if (n < 0) fail(PBX_ERR_VALUE, "negative length");
    const Frame fr = frame_of(flags, frame);
    if (fr.pos.rot || fr.wrap.on)
      fail(PBX_ERR_VALUE,
           "wrap extents are taken before a wrap and a rotation: flags may hold PBX_FRAME_POS and "
           "PBX_FRAME_VEL only (got 0x%x)", flags);
    if (!(L > 0.0) || L == __builtin_inf())
      fail(PBX_ERR_VALUE, "the box size must be finite and positive (got %g)", L);
    for (int e = 0; e < WEXT_N; ++e) h_ext[e] = (e & 1) ? -__builtin_inf() : __builtin_inf();
    if (n == 0) return;
    if (!pos) fail(PBX_ERR_VALUE, "pos is NULL");
    Device &d = current_device();
    std::lock_guard<std::mutex> lk(d.mu);
    hipStream_t st = d.stream;
    ScopedTimer tm("pbx.property.wrap_extents");
    const double *dpos = stage(d, st, pos, 3, 0, n, on_device, kSlotPropPos);
    const int grid = grid_of(n);
    // [rows of extrema][the result]
    double *part = (double *)d.slot(kSlotPropPart)
                       .ensure(sizeof(double) * ((size_t)PROP_MAX_BLOCKS * WEXT_N + WEXT_N));
    double *res = part + (size_t)PROP_MAX_BLOCKS * WEXT_N;
    hipLaunchKernelGGL(property_wrap_extents, dim3(grid), dim3(PROP_TPB), 0, st, dpos, n, fr.pos, L,
                       -0.5 * L, part);
    PBX_HIP(hipGetLastError());
    hipLaunchKernelGGL(wrap_extents_reduce, dim3(1), dim3(PROP_RG * WEXT_RCOLS), 0, st, part, grid,
                       res);
    PBX_HIP(hipGetLastError());
    PBX_HIP(hipMemcpyAsync(h_ext, res, sizeof(double) * WEXT_N, hipMemcpyDeviceToHost, st));
    PBX_HIP(hipStreamSynchronize(st));
  });
}

int pbx_property_virial_radius(const double *pos, const double *mass, int64_t n, int on_device,
                               int use_sphere, const double *sphere, const int64_t *fam, int nfam,
                               int flags, const double *frame, int nclauses, const int *kinds,
                               const int *negate, const double *params, double target_rho,
                               double eta, int niter_max, int has_rmax, double r_max, int levels,
                               double *h_radius, int64_t *iterations, int64_t *passes,
                               int64_t *n_kept, int *status) {
  return guard([&] {
    const Region rg = region_of(nclauses, kinds, negate, params);
    if (!h_radius || !iterations || !passes || !n_kept || !status)
      fail(PBX_ERR_VALUE, "null output");
    if (!(target_rho > 0.0)) fail(PBX_ERR_VALUE, "target_rho must be positive (got %g)", target_rho);
    if (!(eta >= 0.0)) fail(PBX_ERR_VALUE, "eta must not be negative (got %g)", eta);
    if (niter_max < 1) fail(PBX_ERR_VALUE, "niter_max must be >= 1 (got %d)", niter_max);
    if (levels < 0 || levels > PBX_ENCLOSED_LEVELS)
      fail(PBX_ERR_VALUE, "levels must lie in [0, %d] (got %d)", PBX_ENCLOSED_LEVELS, levels);
    check_scope(pos, n, use_sphere, sphere, fam, nfam, flags, frame);
    Device &d = current_device();
    std::lock_guard<std::mutex> lk(d.mu);
    hipStream_t st = d.stream;
    ScopedTimer tm("pbx.property.virial_radius");
    // staged once; every pass re-reads them from HBM
    const Staged s = stage_scope(d, st, pos, mass, n, on_device, use_sphere, sphere, fam, nfam,
                                 flags, frame, rg);
    const int L = levels ? levels : PBX_VIRIAL_LEVELS;
    Enclosed e;
    int64_t np = 0;
    *h_radius = __builtin_nan("");
    *status = PBX_VIRIAL_NOT_CONVERGED;
    *iterations = niter_max;
    *n_kept = 0;
    if (!has_rmax) {
      run_enclosed(d, st, s, 0, nullptr, true, e);
      ++np;
      r_max = e.ext[1] - e.ext[0];
      *n_kept = e.kept;
      if (e.kept == 0) {  // (r_max is NaN: every mid and every z is, nothing converges)
        *passes = np;
        return;
      }
    }
    const double pi = 3.141592653589793;
    double left = 0.0, right = r_max;
    int i = 0;
    while (i < niter_max) {
      if ((right - left) < 0) {
        *h_radius = (right + left) / 2;
        *status = PBX_VIRIAL_CONVERGED;
        *iterations = i;
        break;
      }
      // the midpoints of the next lv iterations in heap order: node k holds
      // the bounds its branch would; child 2k + 1 follows left = mid, child
      // 2k + 2 follows right = mid
      const int lv = std::min(L, niter_max - i);
      const int nt = (1 << lv) - 1;
      double lo[ENC_MAX], hi[ENC_MAX], t[ENC_MAX];
      lo[0] = left;
      hi[0] = right;
      for (int k = 0; k < nt; ++k) {
        t[k] = (lo[k] + hi[k]) / 2;
        if (2 * k + 2 < nt) {
          lo[2 * k + 1] = t[k];
          hi[2 * k + 1] = hi[k];
          lo[2 * k + 2] = lo[k];
          hi[2 * k + 2] = t[k];
        }
      }
      run_enclosed(d, st, s, nt, t, false, e);
      ++np;
      *n_kept = e.kept;
      // walk the decisions of those iterations
      bool done = false;
      for (int k = 0, lvl = 0; lvl < lv; ++lvl, ++i) {
        if ((right - left) < 0) {
          *h_radius = (right + left) / 2;
          *iterations = i;
          done = true;
          break;
        }
        const double mid = t[k];
        const double z = target_rho - e.msum[k] / (4 * pi * std::pow(mid, 3.0) / 3);
        if (std::fabs(z) < eta) {
          *h_radius = mid;
          *iterations = i + 1;
          done = true;
          break;
        } else if (z < 0) {
          left = mid;
          k = 2 * k + 1;
        } else {
          right = mid;
          k = 2 * k + 2;
        }
      }
      if (done) {
        *status = PBX_VIRIAL_CONVERGED;
        break;
      }
    }
    *passes = np;
  });
}

}  // extern "C"
