/*
 * pbx.h — C ABI of libpbx.so, the MI355X-native (gfx950, HIP) engine behind
 * the pynbodyext gravity and radial-profile hot path.
 *
 * Every entry point takes plain pointers and sizes (no framework types) and
 * returns an int status:
 *     PBX_OK          0  success
 *     PBX_ERR_VALUE   1  bad argument          -> Python ValueError
 *     PBX_ERR_RUNTIME 2  HIP / RCCL failure     -> Python RuntimeError
 *     PBX_ERR_NODEV   3  no usable gfx950 GPU   -> Python RuntimeError
 * and the message of the last failure on the calling thread is returned by
 * pbx_last_error().  Nothing here falls back to a CPU path: a missing GPU is
 * an error.
 *
 * The functions below replace the reference's PyO3 boundary module
 * `pynbodyext._rust` (crates/pynbodyext-rust/src/lib.rs:10-27) and the numpy
 * seams of pynbodyext.profiles (profiles/bins.py:346-395,
 * profiles/proarray.py:272-334).  Each block cites the reference interface
 * it replaces.  Host ("h_") pointers are pageable host memory owned by the
 * caller; device ("d_") pointers are HBM allocations (pbx_malloc) and are
 * only used by the device-resident API (bench, multi-GPU).
 */
#ifndef PBX_H
#define PBX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBX_OK 0
#define PBX_ERR_VALUE 1
#define PBX_ERR_RUNTIME 2
#define PBX_ERR_NODEV 3

/* Softening kernel codes: the reference's Option<u8> kernel argument
 * (crates/pynbodyext-rust/src/gravity.rs:67-82).  PBX_KERNEL_NONE is the
 * Newtonian path taken when kernel is None (direct.rs:115-368). */
#define PBX_KERNEL_NONE (-1)
#define PBX_KERNEL_PLUMMER 0
#define PBX_KERNEL_SPLINE 1

/* want bitmask for the fused direct-sum entry */
#define PBX_WANT_POT 1
#define PBX_WANT_ACC 2

/* element types of pbx_profile_select_typed */
#define PBX_F64 0
#define PBX_F32 1

/* ------------------------------------------------------------------ */
/* runtime                                                             */
/* ------------------------------------------------------------------ */
const char *pbx_last_error(void);
int pbx_version(void);                   /* returns e.g. 100 for 0.1.0 */
int pbx_device_count(int *count);
int pbx_set_device(int device);          /* per calling thread */
int pbx_get_device(int *device);
/* Direct-sum precision (process-wide).  precise=1: every 1/sqrt is
 * v_rsq_f64 + one Newton step (~1e-16 relative, the reference's IEEE
 * 1.0/sqrt to rounding).  precise=0 (default; env PBX_PRECISE=1 flips it):
 * the all-particles Newtonian symmetric kernel (n >= 8192) uses v_rsq_f64
 * unrefined, ~5e-8 relative per pair, results within ~1e-7 of the reference
 * (contract 1e-5; direct.rs:165-180 / :296-308 replaced).  No equivalent in
 * the PyO3 module (gravity.rs:448-709). */
int pbx_set_precise(int on);
int pbx_get_precise(int *on);
int pbx_device_synchronize(void);
int pbx_device_name(char *buf, int buflen);

int pbx_malloc(void **d_ptr, size_t bytes);
int pbx_free(void *d_ptr);
int pbx_memcpy_htod(void *d_dst, const void *h_src, size_t bytes);
/* Host -> device copy rates of `bytes` (best of 3 after a warm-up, GB/s):
 * from pinned host memory (one DMA) and from pageable memory through the
 * library's pinned chunks (what a profile call on host arrays uses).  No
 * reference counterpart: the bench's bound for the user-facing profile. */
int pbx_measure_h2d(int64_t bytes, double *pinned_gbs, double *staged_gbs);
/* The current device's cache of engine buffers (profile / octree handles
 * take freed blocks instead of hipMalloc): out[0] cached bytes, out[1]
 * cached blocks, out[2] allocations served from the cache, out[3]
 * allocations that called hipMalloc.  pbx_device_pool_trim frees every
 * cached block (memory back to the device for other users).  No reference
 * counterpart (runtime). */
int pbx_device_pool_stats(int64_t *out);
int pbx_device_pool_trim(void);
int pbx_memcpy_dtoh(void *h_dst, const void *d_src, size_t bytes);
int pbx_memcpy_dtod(void *d_dst, const void *d_src, size_t bytes);
int pbx_memset(void *d_ptr, int value, size_t bytes);

/* Library-owned stream of the current device (all pbx kernels run on it)
 * and HIP events on that stream, so callers can time kernels live. */
int pbx_stream(void **stream);
int pbx_event_create(void **event);
int pbx_event_destroy(void *event);
int pbx_event_record(void *event);
int pbx_event_elapsed_ms(void *start, void *stop, float *ms);
int pbx_stream_synchronize(void);

/* ------------------------------------------------------------------ */
/* gravity: direct summation, host-array boundary                      */
/* ------------------------------------------------------------------ */
/* Replace the four PyO3 pyfunctions of crates/pynbodyext-rust/src/gravity.rs:
 *   direct_accelerations_py            (:448-512)
 *   direct_accelerations_at_points_py  (:514-583)
 *   direct_potentials_py               (:585-644)
 *   direct_potentials_at_points_py     (:646-709)
 * which call crates/gravity/src/direct.rs:115-658.
 * h_pos: n x 3 doubles, C order.  h_masses / h_softenings: n doubles or NULL
 * (NULL masses = unit masses, direct.rs:121-128).  kernel: PBX_KERNEL_*;
 * softenings with PBX_KERNEL_NONE is a PBX_ERR_VALUE with the reference's
 * message (gravity.rs:480-484).  Outputs are caller-allocated:
 * h_acc n x 3, h_pot n. */
int pbx_direct_accelerations(const double *h_pos, int64_t n,
                             const double *h_masses, const double *h_softenings,
                             int kernel, double *h_acc);
int pbx_direct_potentials(const double *h_pos, int64_t n,
                          const double *h_masses, const double *h_softenings,
                          int kernel, double *h_pot);
int pbx_direct_accelerations_at_points(const double *h_pos, int64_t n,
                                       const double *h_targets, int64_t m,
                                       const double *h_masses,
                                       const double *h_softenings, int kernel,
                                       double *h_acc);
int pbx_direct_potentials_at_points(const double *h_pos, int64_t n,
                                    const double *h_targets, int64_t m,
                                    const double *h_masses,
                                    const double *h_softenings, int kernel,
                                    double *h_pot);

/* ------------------------------------------------------------------ */
/* gravity: direct summation, device-resident API (bench / multi-GPU)  */
/* ------------------------------------------------------------------ */
/* Pack device arrays pos (n x 3) and mass (n, or NULL = unit masses) into
 * the 32-byte source records {x, y, z, m} the direct-sum kernel streams. */
int pbx_pack_sources(const double *d_pos, const double *d_mass, int64_t n,
                     double *d_records);
/* Fused direct sum over device-resident records.
 *   d_src      : n_src x 4 records {x,y,z,m}
 *   d_src_h    : n_src softenings or NULL (only read when kernel >= 0)
 *   d_tgt      : n_tgt x 3 target positions
 *   d_tgt_h    : n_tgt target softenings or NULL (all-particles softened
 *                form h = max(h_i, h_j), direct.rs:402,426)
 *   self_offset: >= 0 -> target t is source (self_offset + t) and that pair
 *                is skipped (all-particles form); -1 -> at-points form, no skip
 *   want       : PBX_WANT_POT | PBX_WANT_ACC
 *   d_pot      : n_tgt doubles, d_acc: n_tgt x 3 doubles (either may be NULL
 *                when not wanted) */
int pbx_direct_dev(const double *d_src, const double *d_src_h, int64_t n_src,
                   const double *d_tgt, const double *d_tgt_h, int64_t n_tgt,
                   int64_t self_offset, int kernel, int want, double *d_pot,
                   double *d_acc);

/* All-particles Newtonian direct sum with each unordered pair evaluated
 * once (Newton's third law; pbx_direct_dev and the host entry points use it
 * by themselves for n >= 8192), split into work units so that ranks can
 * share one solve: every rank runs its units into a per-particle
 * accumulator d_acc4 (npad x 4 doubles, zeroed by the caller), the ranks sum
 * the accumulators (pbx_comm_allreduce_f64), and each rank converts its own
 * particles [lo, hi) into potentials / accelerations.  h_weights (optional,
 * n_units) = relative cost of each unit, for balancing. */
int pbx_direct_sym_plan(int64_t n, int64_t *npad, int64_t *n_units, int64_t *h_weights);
int pbx_direct_sym_accumulate(const double *d_src, int64_t n, int64_t u0, int64_t u1, int want,
                              double *d_acc4);
int pbx_direct_sym_finish(const double *d_acc4, int64_t lo, int64_t hi, int want, double *d_pot,
                          double *d_acc);
/* When all n particles carry the same mass (compared bitwise on the device,
 * per accumulate call) the pair loop runs without the mass and multiplies
 * by it once per flushed partial sum.  Counters of the calling thread's
 * device: pair-kernel launches of the uniform-mass and of the general
 * instantiation (either pointer may be NULL). */
int pbx_direct_sym_path_stats(int64_t *uniform_launches, int64_t *general_launches);

/* ------------------------------------------------------------------ */
/* gravity: Barnes-Hut octree                                         */
/* ------------------------------------------------------------------ */
/* Replaces the PyO3 class `Octree` (crates/pynbodyext-rust/src/gravity.rs:
 * 114-445) over crates/gravity/src/tree.rs + multipole.rs.  The tree lives
 * in HBM behind an opaque handle; it reproduces the reference octree node
 * for node (root box, octants, split rule, payload order), so the opening
 * decisions of every target equal the reference's.
 * pos/masses/softenings/points/outputs are host arrays when on_device == 0,
 * device arrays when on_device == 1.  kernel: PBX_KERNEL_PLUMMER or
 * PBX_KERNEL_SPLINE (the PyO3 layer maps None to Plummer, gravity.rs:77-82).
 * want: PBX_WANT_POT | PBX_WANT_ACC. */
typedef struct pbx_octree pbx_octree;
/* Octree::new (gravity.rs:123-226): structure; mass payload iff masses */
int pbx_octree_create(const double *pos, int64_t n, const double *masses,
                      const double *softenings, int64_t leaf_capacity,
                      int multipole_order, int kernel, int on_device,
                      pbx_octree **out);
int pbx_octree_destroy(pbx_octree *tree);
/* Octree::new semantics on new particles (same leaf_capacity / order /
 * kernel), reusing the handle's HBM buffers (a time step of a simulation,
 * the next snapshot); mass payload iff masses */
int pbx_octree_rebuild(pbx_octree *tree, const double *pos, int64_t n, const double *masses,
                       const double *softenings, int on_device);
/* build_mass(masses=None) (gravity.rs:228-239): NULL keeps current masses */
int pbx_octree_build_mass(pbx_octree *tree, const double *masses, int on_device);
/* set_softenings (gravity.rs:241-258; h_max is not rebuilt, tree.rs:777) */
int pbx_octree_set_softenings(pbx_octree *tree, const double *softenings, int on_device);
/* set_kernel (gravity.rs:260-265) */
int pbx_octree_set_kernel(pbx_octree *tree, int kernel);
/* compute_potentials / compute_accelerations (gravity.rs:267-346,
 * tree.rs:1415-1496): every particle, self pair skipped, outputs in the
 * caller's particle order (pot n, acc n x 3) */
int pbx_octree_compute(pbx_octree *tree, double theta, int want, double *pot,
                       double *acc, int on_device);
/* potentials_at_points / accelerations_at_points (gravity.rs:348-445,
 * tree.rs:1498-1558): m query points (m x 3), no self skip */
int pbx_octree_at_points(pbx_octree *tree, const double *points, int64_t m,
                         double theta, int want, double *pot, double *acc,
                         int on_device);
/* One rank's shard of compute_*: the targets are the particles
 * [first, first + count) of the tree's leaf (DFS) order, self pairs skipped.
 * compact = 0: outputs at the particles' original indices (full-length
 * device arrays); compact = 1: count entries in leaf order.  d_cost
 * (optional, count int32): accepted nodes + leaf pairs per target, to
 * balance the next split.  Device pointers only. */
int pbx_octree_compute_range(pbx_octree *tree, double theta, int want, int64_t first,
                             int64_t count, int compact, double *d_pot, double *d_acc,
                             int32_t *d_cost);
/* positions (count x 3), masses and original indices (int64) of the leaf-order
 * particles [first, first + count), into device buffers (any may be NULL) */
int pbx_octree_leaf_particles(pbx_octree *tree, int64_t first, int64_t count, double *d_pos,
                              double *d_mass, int64_t *d_idx);
/* 3-D radial profile of a per-target field over the leaf-order targets
 * [first, first + count): d_f (device, count doubles in leaf order, e.g. the
 * potential of compute_range with compact = 1), nbins + 1 increasing host
 * edges; r = sqrt((x*x + y*y) + z*z) of the tree's own positions, bin as
 * BinsSet._assign_particles (bins.py:346-395).  Outputs (host): counts[nbins]
 * and moments[nbins][7] = {Σw, Σf·w, Σf²·w, Σf, Σf², Σ|f|·w, Σ|f|} with w =
 * the mass (pbx_profile_moments' columns, proarray.py:272-334).  Replaces
 * the select / assign / moments round trips of a tree's potential profile. */
int pbx_octree_radial_moments(pbx_octree *tree, int64_t first, int64_t count, const double *d_f,
                              const double *h_edges, int64_t nbins, int64_t *h_counts,
                              double *h_moments);
/* The same into DEVICE memory, no sync: d_out = nbins int64 counts followed
 * by nbins x 7 doubles (row-major), e.g. for an in-place all-reduce of the
 * ranks' partial profiles before one read-back. */
int pbx_octree_radial_moments_device(pbx_octree *tree, int64_t first, int64_t count,
                                     const double *d_f, const double *h_edges, int64_t nbins,
                                     void *d_out);
/* Multi-GPU load balance without an extra walk (the reference has one
 * process; its rayon pool splits targets dynamically, tree.rs:1443-1556):
 * cost_to_orig scatters per-target costs held in leaf order (n int32, e.g.
 * the d_cost of every rank's compute_range, all-gathered) to original
 * particle order; balance reads such costs through the CURRENT build's leaf
 * order and writes to host cuts[world + 1] the contiguous leaf-order ranges
 * [cuts[r], cuts[r+1]) of about equal summed max(cost, 1) — the split of
 * pynbodyext.parallel.balanced_ranges.  Device pointers; balance syncs. */
int pbx_octree_cost_to_orig(pbx_octree *tree, const int32_t *d_cost_leaf, int32_t *d_cost_orig);
int pbx_octree_balance(pbx_octree *tree, const int32_t *d_cost_orig, int world, int64_t *cuts);
/* What d_cost of compute_range holds: kind 0 (default) the target's accepted
 * nodes + leaf pairs; kind 1 its wave's work (the wave's node steps + its
 * 4-record leaf rounds, the same for the 64 targets of one wave), which is
 * what a walk's time follows — ShardedTree balances on it. */
int pbx_octree_set_cost_kind(pbx_octree *tree, int kind);
/* Walk statistics on (1, default) or off (0) for this tree's later walks of
 * order 3 with potential + acceleration, no softening, in fast mode (no
 * reference counterpart: instrumentation).  Off, pbx_octree_info reports zero
 * interaction and step counts for those walks; decisions and values are
 * unchanged. */
int pbx_octree_set_walk_counters(pbx_octree *tree, int enabled);
/* out[13] = {n, nodes, levels, has_mass_payload, has_hmax,
 *            accepted node interactions and leaf pairs of the last walk,
 *            path words, wave steps and active-lane steps of the last walk
 *            (SIMD efficiency = active / (64 * steps)), leaf wave steps,
 *            their active lanes, wave steps that descended} */
int pbx_octree_info(pbx_octree *tree, int64_t *out);
/* Node arrays for parity tests (any pointer may be NULL), node ids in the
 * device's breadth-first numbering:
 *   center nodes x 4 {cx, cy, cz, half}; com nodes x 4 {x, y, z, mass};
 *   hmax nodes; links nodes x 3 {first (-1 for a leaf), next, n_children};
 *   leaf nodes x 2 {start, count} into perm; perm n (leaf order -> index);
 *   moments nodes x ncoef(order) (order >= 2). */
int pbx_octree_export(pbx_octree *tree, double *center, double *com, double *hmax,
                      int64_t *links, int64_t *leaf, int64_t *perm, double *moments);

/* ------------------------------------------------------------------ */
/* radial profiles: binning + per-bin reduction                        */
/* ------------------------------------------------------------------ */
/* One opaque handle per profile holds the binned quantity x (and, after a
 * fused selection, the selection weights and original indices) in HBM.
 * Replaces, in pynbodyext/profiles:
 *   BinsSet._assign_particles        bins.py:346-395  (assign + csr)
 *   equal_number_bins_algorithm      bins.py:720-746  (edges_equaln)
 *   np.min / np.max in lin / log     bins.py:689-718  (minmax)
 *   ProfileArray._compute sums       proarray.py:272-334 (moments)
 * and the filter scope feeding it (Sphere & FamilyFilter + sim["r"],
 * filters/filt.py:42-86, profiles/spatial_profile.py:30-35) (select). */
int pbx_profile_create(void **handle);
int pbx_profile_destroy(void *handle);
/* x = host array of n doubles (the generic BinsSet path) */
int pbx_profile_set_x(void *handle, const double *h_x, int64_t n);
/* Fused selection: keep particle i when (no family ranges given, or
 * fam[2f] <= i < fam[2f+1] for some f < nfam) and (use_sphere == 0, or
 * ((x-cx)^2+(y-cy)^2)+(z-cz)^2 < sphere[3]) with sphere = {cx,cy,cz,R^2};
 * x = sqrt((x*x+y*y)+z*z) (ndim 3) or sqrt(x*x+y*y) (ndim 2), weights =
 * mass (or 1), kept in index order.  pos/mass are host (on_device = 0) or
 * device pointers (on_device = 1). */
int pbx_profile_select(void *handle, const double *pos, const double *mass, int64_t n,
                       int on_device, int use_sphere, const double *sphere,
                       const int64_t *fam, int nfam, int ndim, int64_t *n_kept);
/* The same for float32 snapshots without a host up-cast (pos_dtype /
 * mass_dtype PBX_F64 or PBX_F32).  numpy's dtype rules for a float32 pos
 * array: the Sphere distance against the float64 centre is evaluated in
 * double on the exactly widened coordinates; x = sim["r"] / sim["rxy"] of the
 * float32 array is float32 arithmetic ((x*x+y*y)+z*z, correctly rounded
 * sqrtf) and is held widened (exactly) as double; masses are widened. */
int pbx_profile_select_typed(void *handle, const void *pos, int pos_dtype, const void *mass,
                             int mass_dtype, int64_t n, int on_device, int use_sphere,
                             const double *sphere, const int64_t *fam, int nfam, int ndim,
                             int64_t *n_kept);
/* original indices (int64), x and weights of the selection (any may be NULL) */
int pbx_profile_get_selection(void *handle, int64_t *h_idx, double *h_x, double *h_w);
int pbx_profile_minmax(void *handle, double *mn, double *mx);
/* equaln edges into h_edges (capacity nbins + 1); *n_edges = nbins + 1, or
 * 2 for the reference's degenerate "< 2 values" case */
int pbx_profile_edges_equaln(void *handle, int64_t nbins, int has_min, double bin_min,
                             int has_max, double bin_max, double *h_edges,
                             int64_t *n_edges);
/* Distributed equaln (no reference counterpart — the
 * reference is single-process): the radix select of
 * pbx_profile_edges_equaln in stages.  Every rank: key_range (local
 * order-preserving u64 keys of x; (~0, 0) when empty) -> min/max over ranks
 * -> msel_begin(global range, same bounds on every rank; returns the level
 * count L) -> for level 0..L-1: msel_hist (this rank's digit histogram,
 * *count u32 at *d_hist on the device) -> sum *d_hist over ranks in place
 * (pbx_comm_allreduce, dtype u32) -> msel_resolve -> msel_edges (identical
 * on every rank; same results and errors as pbx_profile_edges_equaln on the
 * concatenated x).  nbins <= 1024. */
int pbx_profile_key_range(void *profile, uint64_t *kmin, uint64_t *kmax);
int pbx_profile_msel_begin(void *profile, int64_t nbins, int has_min, double bin_min, int has_max,
                           double bin_max, uint64_t kmin, uint64_t kmax, int *levels);
int pbx_profile_msel_hist(void *profile, int level, uint32_t **d_hist, int64_t *count);
int pbx_profile_msel_resolve(void *profile, int level);
int pbx_profile_msel_edges(void *profile, double *h_edges, int64_t *n_edges);
/* bin ids + counts (nb = n_edges - 1 int64) for ascending edges */
int pbx_profile_assign(void *handle, const double *h_edges, int64_t n_edges,
                       int64_t *h_counts, int64_t *n_valid);
/* CSR of the assignment (perm: n_valid int64, offsets: nb+1); NULL = skip */
int pbx_profile_csr(void *handle, int64_t *h_perm, int64_t *h_offsets);
/* per-bin sums h_out[nb][7] = {Σw, Σf·w, Σf²·w, Σf, Σf², Σ|f|·w, Σ|f|};
 * f_src / w_src: 0 = x, 1 = selection weights, 2 = host array (h_f / h_w,
 * n doubles in selection order), 3 = device array indexed by ORIGINAL
 * particle (gathered through the selection, e.g. a tree potential left in
 * HBM by pbx_octree_compute), PBX_SRC_KIN + code = a kinematic field (f_src
 * only, see below); w_src = -1: unweighted */
int pbx_profile_moments(void *handle, int f_src, const double *h_f, int w_src,
                        const double *h_w, double *h_out);
/* the same for the columns whose bit is set in cols (bit k = column k of
 * h_out; the others are 0): each statistic reads only some of the sums
 * (proarray.py:632-860 — Sum: Σf; weighted Mean: Σw, Σf·w; ...) */
int pbx_profile_moments_cols(void *handle, int f_src, const double *h_f, int w_src,
                             const double *h_w, uint32_t cols, double *h_out);
/* Kinematic fields of the kept particles, computed on the device from the
 * ORIGINAL particles' positions and velocities — pynbody's derived arrays
 * behind prof["vr"] (proarray.py:55-56, 179-187) and the profile's beta,
 * without a per-field column on the host.  In float64, no FMA contraction,
 * correctly rounded / and sqrt, in this order:
 *   rxy2 = x*x + y*y;  r2 = rxy2 + z*z;  rxy = sqrt(rxy2);  r = sqrt(r2);
 *   s = x*vx + y*vy;
 *   vr = (s + z*vz) / r;            vrxy = s / rxy;
 *   vphi = (x*vy - y*vx) / rxy;     vtheta = (z*vrxy - rxy*vz) / r;
 *   v2 = (vx*vx + vy*vy) + vz*vz;   vt = sqrt(v2 - vr*vr)
 * (0/0 on the z axis and at the origin is NaN, as numpy gives).  A field is
 * named by its code, and PBX_SRC_KIN + code is a source selector (f_src) of
 * pbx_profile_moments, pbx_profile_moments_cols and pbx_profile_percentiles:
 * the field is then computed into the handle's stage buffer in selection
 * order and consumed like any other source. */
#define PBX_KIN_VR 0
#define PBX_KIN_VTHETA 1
#define PBX_KIN_VPHI 2
#define PBX_KIN_VRXY 3
#define PBX_KIN_V2 4
#define PBX_KIN_VT 5
#define PBX_SRC_KIN 16
/* Register pos / vel, n x 3 doubles each, n = the length of the arrays the
 * handle's selection was made from (after pbx_profile_set_x: the handle's
 * own length, particle i = element i); another n is a PBX_ERR_VALUE.  Host
 * arrays (on_device = 0) are staged into the handle, only the index span the
 * selection covers, and may be released after the call; pos holds the
 * positions the selection was made from (a handle that kept its staged copy
 * of them reads that instead of staging pos again).  Device arrays
 * (on_device = 1) are borrowed: they must stay allocated and unchanged until
 * the next selection on this handle or until the registration is cleared.
 * pos = vel = NULL clears it; every new selection (and pbx_profile_set_x)
 * clears it too.  A kinematic source without a registration is a
 * PBX_ERR_VALUE. */
int pbx_profile_set_kinematics(void *handle, const double *pos, const double *vel, int64_t n,
                               int on_device);
/* field `code` of the kept particles in selection order into h_out (the
 * selection's length, host) */
int pbx_profile_kinematic_field(void *handle, int code, double *h_out);
/* The fused pass: h_out[n_fields][nb][7] = the seven sums of
 * pbx_profile_moments_cols for every field codes[k] under its column mask
 * cols[k] (columns not requested are 0), from ONE read of the selection and
 * the positions / velocities (64 B per kept particle) instead of a written
 * and re-read column per field.  1 <= n_fields <= 6; w_src / h_w as
 * pbx_profile_moments_cols (-1: unweighted, Σw and the weighted columns are
 * then 0).  The per-bin accumulators live in LDS, one slot per requested
 * (field, column) pair plus one shared Σw; when nb x slots exceeds the LDS
 * footprint of the generic sums the call runs them field by field instead
 * (same results to rounding). */
int pbx_profile_kinematic_moments(void *handle, int n_fields, const int *codes, int w_src,
                                  const double *h_w, const uint32_t *cols, double *h_out);
/* The frame a handle reads particles in: an optional position shift c, an
 * optional velocity shift vc, an optional periodic wrap of the positions
 * (box size L, lower bound lo per axis) and an optional rotation R
 * (row-major 3 x 3), packed as frame[15] = {c[3], vc[3], R[9]}, or as
 * frame[19] = {c[3], vc[3], R[9], L, lo[3]} with PBX_FRAME_WRAP, with one
 * PBX_FRAME_* flag per step.  Per particle, in float64 without FMA
 * contraction, in this order:
 *   dx = x - c0;  dy = y - c1;  dz = z - c2            (PBX_FRAME_POS)
 *   k  = floor((dx - lo0) / L) + 0.0;  dx = dx - k*L;  the same for dy, dz
 *                                                      (PBX_FRAME_WRAP)
 *   x' = (R00*dx + R01*dy) + R02*dz;  y' = (R10*dx + R11*dy) + R12*dz;
 *   z' = (R20*dx + R21*dy) + R22*dz                    (PBX_FRAME_ROT)
 * and the same for v with vc (PBX_FRAME_VEL, PBX_FRAME_ROT; a velocity is
 * never wrapped).  The wrap restates WrapBox of the reference
 * (transforms/wrap.py:117-213) into [lo, lo + L): lo[k] is -0.5*L (its
 * "center") or 0.0 ("upper"), "/" is IEEE division (no reciprocal), and the
 * "+ 0.0" turns a -0.0 from floor into +0.0, as the reference's integer k
 * does, so that -0.0 stays -0.0.  A non-finite coordinate follows the
 * statement (inf - inf*L is NaN).  frame[15..18] is read ONLY when
 * PBX_FRAME_WRAP is set: without it a frame is 15 numbers, as before.
 * PBX_FRAME_WRAP with L not finite or L <= 0, or with a lo[k] other than
 * -0.5*L or 0.0, is a PBX_ERR_VALUE whose message names PBX_FRAME_WRAP.  Bit
 * 8 is unassigned and, like every other unknown bit, an error.  A step whose
 * flag is off is skipped, not run with zeros or the identity (0 * inf would
 * turn an infinite coordinate into NaN).  Everything downstream is computed
 * from x', v' exactly as it is from x, v without a frame: the Sphere test of
 * every selection (its centre is given in frame coordinates), x = r / rxy,
 * and the kinematic fields (pbx_profile_kinematic_field,
 * pbx_profile_kinematic_moments, the PBX_SRC_KIN sources).  This replaces
 * the in-place array rewrites of the reference's transforms
 * (transforms/shift.py, transforms/rotate.py) for the device passes.
 * Sticky: the frame stays on the handle across selections (it is a property
 * of how the handle reads particles) until flags == 0 or frame == NULL
 * clears it.  Set it before the selection it should apply to; x of an
 * earlier selection is not recomputed.  The kinematic fields read the frame
 * the handle holds WHEN THEY ARE EVALUATED, not the one a selection was made
 * with: changing the frame between a selection and a kinematic call mixes
 * two frames without an error, so keep it unchanged across the two (after
 * pbx_profile_set_x there is no selection: set the frame any time before
 * the kinematic call).  With a frame set, float32 positions
 * in pbx_profile_select_typed and the distributed entry
 * pbx_profile_radial_equaln_comm are a PBX_ERR_VALUE, and so are unknown
 * flag bits. */
#define PBX_FRAME_POS 1
#define PBX_FRAME_VEL 2
#define PBX_FRAME_ROT 4
#define PBX_FRAME_WRAP 16
int pbx_profile_set_frame(void *handle, int flags, const double *frame);
/* The region a handle keeps particles in: a conjunction of nclauses <=
 * PBX_REGION_MAX clauses, each one primitive (kinds[c]), negated when
 * negate[c] != 0 (negate may be NULL: none), with its constants in
 * params[c][0..5].  Per particle, in float64 without FMA contraction, in this
 * order, on the coordinates the pass holds (after the frame when one is set;
 * centres and corners are given in frame coordinates), every comparison
 * strict, no periodic wrap:
 *   kind                params                     kept when
 *   PBX_REGION_SPHERE   cx, cy, cz, R^2            ((dx*dx + dy*dy) + dz*dz) < R^2
 *   PBX_REGION_DISC     cx, cy, cz, R^2, h         (dx*dx + dy*dy) < R^2 && fabs(dz) < h
 *   PBX_REGION_CUBOID   x1, y1, z1, x2, y2, z2     x > x1 && x < x2 && y > y1 && y < y2
 *                                                  && z > z1 && z < z2
 *   PBX_REGION_BAND     field, lo, hi, has_lo,     (!has_lo || f > lo) && (!has_hi || f < hi)
 *                       has_hi
 * with dx = x - cx (and so on), field one of PBX_BAND_X / _Y / _Z (the
 * coordinate itself), PBX_BAND_R (f = sqrt((x*x + y*y) + z*z)) or
 * PBX_BAND_RXY (f = sqrt(x*x + y*y)): a band compares the square root, not
 * the square, as sim["r"] > lo does.  A negated clause is the logical NOT of
 * its boolean, not the reversed comparison: a NaN coordinate fails a plain
 * clause and passes a negated one (numpy's ~mask).  This restates
 * pynbody.filt's Sphere, Disc, Cuboid, BandPass / HighPass / LowPass, and
 * Annulus = Sphere(max) & ~Sphere(min), SolarNeighborhood = Disc(max, h) &
 * ~Disc(min, h) as two clauses.
 * Sticky: the region stays on the handle across selections until
 * nclauses == 0 clears it.  Every later selection on the handle
 * (pbx_profile_select, pbx_profile_select_typed, pbx_profile_radial_equaln on
 * every path it takes) keeps a particle only when the region holds IN
 * ADDITION TO its own use_sphere / fam arguments; the kinds, flags and
 * constants are wave-uniform (the handle's device copy, read with scalar
 * loads), and the kernels that evaluate them are instantiations of their
 * own: without a region a selection runs the region-less code.  Set it before the selection it should
 * apply to; an earlier selection is not recomputed.  With a region set,
 * float32 positions in pbx_profile_select_typed and the distributed entry
 * pbx_profile_radial_equaln_comm are a PBX_ERR_VALUE, and so are more than
 * PBX_REGION_MAX clauses, an unknown kind and an unknown band field. */
#define PBX_REGION_MAX 8
#define PBX_REGION_SPHERE 1
#define PBX_REGION_DISC 2
#define PBX_REGION_CUBOID 3
#define PBX_REGION_BAND 4
#define PBX_BAND_X 0
#define PBX_BAND_Y 1
#define PBX_BAND_Z 2
#define PBX_BAND_R 3
#define PBX_BAND_RXY 4
int pbx_profile_set_region(void *handle, int nclauses, const int *kinds, const int *negate,
                           const double *params);
/* One equaln radial-profile pass after pbx_profile_select with a single host
 * round trip (bins.py:720-746 edges, :346-395 assignment, the CSR when
 * build_csr, and per-bin sums of n_stats <= 16 requests (f_src / w_src in
 * {0 x, 1 weights} / -1, column mask cols[k]) as h_moments[k][nb][7]).
 * Same results and errors as pbx_profile_edges_equaln + pbx_profile_assign
 * (+ pbx_profile_csr) + pbx_profile_moments_cols; *n_edges = nbins + 1 or 2
 * (the reference's degenerate case, then nb = 1).  nbins <= 1024. */
int pbx_profile_binned_equaln(void *handle, int64_t nbins, int has_min, double bin_min,
                              int has_max, double bin_max, int build_csr, int n_stats,
                              const int *f_src, const int *w_src, const uint32_t *cols,
                              double *h_edges, int64_t *n_edges, int64_t *h_counts,
                              int64_t *n_valid, double *h_moments);
/* pbx_profile_select + pbx_profile_binned_equaln with ONE host round trip
 * (the RadialProfileBuilder equaln path end to end: filters/filt.py:42-86,
 * bins.py:720-746 / :346-395, proarray.py:272-334 sums).  Same arguments,
 * results and errors as the two calls in sequence; *n_kept as
 * pbx_profile_select (also set when the binning then fails).
 * Lifetime: with on_device = 1 the selection is lazy — the weights of the
 * kept particles are read from the caller's `mass` device array by the
 * first later call on this handle that needs them (pbx_profile_moments*,
 * pbx_profile_get_selection with h_w, weighted percentiles) and held by the
 * handle from then on, so that array must stay allocated and unchanged
 * until that call (or the next selection).  The same holds for `pos`: a
 * repeated large (tiled) call that bins with the stored table
 * (pbx_profile_spec_stats) keeps no copy of x, and the first later call that
 * reads x (pbx_profile_get_selection with h_x, statistics or percentiles of
 * x, pbx_profile_edges_equaln / assign on this selection) recomputes it from
 * `pos`.  Host inputs (on_device = 0) are staged into the handle. */
int pbx_profile_radial_equaln(void *handle, const double *pos, const double *mass, int64_t n,
                              int on_device, int use_sphere, const double *sphere,
                              const int64_t *fam, int nfam, int ndim, int64_t nbins, int has_min,
                              double bin_min, int has_max, double bin_max, int build_csr,
                              int n_stats, const int *f_src, const int *w_src,
                              const uint32_t *cols, int64_t *n_kept, double *h_edges,
                              int64_t *n_edges, int64_t *h_counts, int64_t *n_valid,
                              double *h_moments);
/* pbx_profile_radial_equaln for one rank of a profile whose particles are
 * sharded over the ranks of `comm` (the reference is
 * single-process): pos / mass are this rank's particles, the edges are the
 * equaln order statistics of ALL ranks' kept x (identical on every rank),
 * h_counts / h_moments the global per-bin counts and sums, h_counts_local
 * (nbins, may be NULL) this rank's counts; *n_kept / *n_valid and the CSR
 * left in the handle are this rank's.  Every rank calls it with the same
 * nbins, window and statistics.  Device all-reduces between the kernels,
 * two host read-backs per call. */
int pbx_profile_radial_equaln_comm(void *comm, void *handle, const double *pos, const double *mass,
                                   int64_t n, int on_device, int use_sphere, const double *sphere,
                                   const int64_t *fam, int nfam, int ndim, int64_t nbins,
                                   int has_min, double bin_min, int has_max, double bin_max,
                                   int build_csr, int n_stats, const int *f_src, const int *w_src,
                                   const uint32_t *cols, int64_t *n_kept, double *h_edges,
                                   int64_t *n_edges, int64_t *h_counts, int64_t *h_counts_local,
                                   int64_t *n_valid, double *h_moments);
/* Telemetry of pbx_profile_radial_equaln on this handle (no reference
 * counterpart): out[3] = {calls run as the one-launch persistent kernel,
 * of those the calls discarded at a grid barrier and re-run by the
 * multi-kernel path (a silent ~2x slowdown if non-zero), calls that took
 * the multi-kernel path}. */
int pbx_profile_path_stats(void *handle, int64_t *out);
/* Telemetry of the one-launch calls (no reference counterpart): out[3] =
 * {one-launch calls, of those the calls whose level-0 digit histogram was
 * counted during the selection with the previous one-launch call's geometry
 * (every window key inside it: one grid barrier and the second count
 * skipped; the edges are the same either way), and the calls that found the
 * previous call's edges at their ranks (tried when the last two calls' edges
 * were identical: each edge's keys below / equal counted during the
 * selection; a hit skips the order-statistic phases and their barriers)}.
 * PBX_MONO_EDGE=0 disables the edge speculation. */
int pbx_profile_mono_stats(void *handle, int64_t *out);
/* Telemetry of the tiled (>= 1024 selection tiles) multi-kernel calls of
 * pbx_profile_radial_equaln on this handle (no reference counterpart):
 * out[2] = {tiled calls, of those the calls whose level-0 digit histogram
 * was counted by the selection kernel with the previous tiled call's digit
 * geometry (every window key inside it), so x was not read a second time}. */
int pbx_profile_level0_stats(void *handle, int64_t *out);
/* Telemetry of the speculative assignment of the tiled calls (no reference
 * counterpart): out[3] = {calls whose selection kernel also binned every key
 * with the bin table stored by an earlier call (launched when the previous
 * tiled call's level-0 digits of every rank matched that table), of those the
 * calls whose own digits matched it too, so the assignment pass (a second
 * read of x and the masses) was skipped, and of those the calls that also
 * binned the keys of edge-holding digits with the previous call's edges
 * (launched when the last two calls' edges were identical) and found every
 * edge at its rank: no deferred keys and no order-statistic finish}.  A
 * miss re-runs the assignment; results are identical either way.
 * A speculating call stores no x: it is rebuilt from the positions when a
 * later call reads it, so with on-device inputs the speculation runs only
 * after pbx_profile_set_source_stable(handle, 1) (host inputs are staged
 * into the handle and always qualify). */
int pbx_profile_spec_stats(void *handle, int64_t *out);
/* stable = 1: the caller's DEVICE positions (and masses) given to this
 * handle's radial_equaln calls stay alive and unchanged until the next
 * selection on the handle — a speculating call may then keep no copy of x
 * and rebuild it from them for a later reader (selection(x), statistics or
 * percentiles of x).  0 (default): on-device calls do not speculate, x is
 * stored (no lifetime contract on the positions beyond the call).  No
 * reference counterpart (numpy has no such hazard). */
int pbx_profile_set_source_stable(void *handle, int stable);
/* enabled = 0: this handle's tiled calls never use a level-0 digit
 * geometry they did not derive themselves (every call re-reads x for its
 * level-0 histogram); 1 (default): use the previous call's when it holds,
 * and on a first call one from a sample of the keys (sample_hint); 2:
 * forget the earlier calls (geometries, speculation state) — the next call
 * runs as a handle's first.  Results are identical in every mode. */
int pbx_profile_set_level0_hint(void *handle, int enabled);
/* Per-bin percentiles of the last assignment — replaces the per-bin loop of
 * ProfileArray._compute for Percentile / Median / Abs_pXX
 * (proarray.py:272-334 + :689-722): h_out[bin*nq + k] = np.interp(q[k],
 * cdf, sorted field) with cdf = (cumsum(w[order]) - c0) / (c_last - c0)
 * (np.cumsum order and rounding) or np.linspace(0, 1, m) when w_src = -1;
 * empty bins NaN.  f_src / w_src as above; absval: statistic of |f|;
 * q[k] = p/100, 1 <= nq <= 4096. */
int pbx_profile_percentiles(void *handle, int f_src, const double *h_f, int w_src,
                            const double *h_w, int absval, int nq, const double *q,
                            double *h_out);
/* The containment values of the handle's whole x as ONE group — replaces
 * ParamContain.calculate (properties/base.py:60-103): the stable sort of x
 * by value (the percentiles' key sort, no bin-id sort and no assignment),
 * cumsum of the weights in that order, h_out[k] = np.interp(q[k],
 * (cumsum - cumsum[0]) / denom, sorted x) with *denom = cumsum[-1] -
 * cumsum[0].  Runs after a selection or after pbx_profile_set_x; w_src = 1
 * (the selection weights) or 2 (the host array h_w, n doubles in selection
 * order); 1 <= nq <= 4096.  With fewer than 2 elements or denom <= 0, h_out
 * is not meaningful (*denom = 0 below 2 elements) and the status is still
 * PBX_OK: the caller raises the reference's error.  Ties keep index order
 * (the reference's default np.argsort leaves their order open).  The
 * cumulative sum runs sequentially on one lane on purpose: that reproduces
 * np.cumsum's rounding bit for bit.  Its cost grows linearly with the
 * selection (about 20 ns per element on an MI355X,
 * profiles/radius_at_density/README.md); a parallel scan would trade the bit
 * parity away and is left for later. */
int pbx_profile_contain(void *handle, int w_src, const double *h_w, int nq, const double *q,
                        double *h_out, double *denom);

/* ------------------------------------------------------------------ */
/* scalar properties: one streaming pass over a selection              */
/* ------------------------------------------------------------------ */
/* Replaces the numpy passes of pynbodyext/properties (properties/generic.py:
 * 39-198: CenPos, CenVel, AngMomVec, KappaRot, KappaRotMean, PatternSpeed;
 * properties/base.py:60-119: ParamContain, ParamSum).  A particle is kept
 * exactly as pbx_profile_select keeps it (family ranges, strict Sphere
 * test); for every kept particle a count and the sums of the requested
 * groups are accumulated in float64, every term evaluated without FMA
 * contraction in the order written here (m = mass, or 1.0 when mass is
 * NULL), with
 *   vc = (x*vy - y*vx) / sqrt(x*x + y*y);  ke = 0.5*((vx*vx + vy*vy) + vz*vz)
 * (0/0 on the z axis and ke == 0 give NaN / inf as numpy does, and they
 * propagate into the sum; a particle that is not kept contributes nothing,
 * whatever its values):
 *   group                sums    terms
 *   PBX_PROP_MASS        0       m
 *   PBX_PROP_COM         1-3     x*m, y*m, z*m
 *   PBX_PROP_COV         4-6     vx*m, vy*m, vz*m
 *   PBX_PROP_ANGMOM      7-9     m*(y*vz - z*vy), m*(z*vx - x*vz), m*(x*vy - y*vx)
 *   PBX_PROP_KAPPA       10, 11  (0.5*m)*(vc*vc), m*ke
 *   PBX_PROP_KAPPA_MEAN  12      (0.5*(vc*vc))/ke
 *   PBX_PROP_PATTERN     13-17   (m*x)*x, (m*y)*y, (m*x)*y, m*(x*vy + y*vx),
 *                                m*(x*vx - y*vy)
 * The order of summation is fixed by the particle count alone (no atomics):
 * the same call gives the same bits, and a sum's bits do not depend on which
 * other groups are requested. */
#define PBX_PROP_MASS 1
#define PBX_PROP_COM 2
#define PBX_PROP_COV 4
#define PBX_PROP_ANGMOM 8
#define PBX_PROP_KAPPA 16
#define PBX_PROP_KAPPA_MEAN 32
#define PBX_PROP_PATTERN 64
#define PBX_PROP_NSUMS 18
/* Stateless; pos / vel (n x 3) and mass (n, may be NULL) are host arrays
 * (only the span the families cover is staged) or device pointers
 * (on_device = 1); sphere, fam and nfam as in pbx_profile_select.  vel is
 * read only for a velocity group, pos only for a sphere or a position group
 * (either may be NULL otherwise).  h_sums[PBX_PROP_NSUMS]: unrequested sums
 * are 0.0; nothing kept: *n_kept = 0, all sums 0.0, PBX_OK.  PBX_ERR_VALUE:
 * groups == 0 or unknown bits, a needed array NULL, n < 0, nfam > 16. */
int pbx_property_moments(const double *pos, const double *vel, const double *mass, int64_t n,
                         int on_device, int use_sphere, const double *sphere,
                         const int64_t *fam, int nfam, uint32_t groups, int64_t *n_kept,
                         double *h_sums);
/* The same pass in a frame (flags / frame as in pbx_profile_set_frame: 15
 * numbers, and frame[15..18] read only when PBX_FRAME_WRAP is set;
 * flags == 0 or frame == NULL: exactly pbx_property_moments).  Positions and
 * velocities are taken to the frame first; the Sphere test (its centre in
 * frame coordinates) and every term are then evaluated from x', v' as above.
 * pos is read when there is a sphere or a position group, as before; vel for
 * a velocity group.  The frame constants are kernel arguments, and the
 * frame-less instantiations of the kernel are the ones pbx_property_moments
 * launches.  The summation order depends on the particle count alone, so the
 * sums equal, bit for bit, those of pbx_property_moments on arrays rewritten
 * with the restatement above. */
int pbx_property_moments_frame(const double *pos, const double *vel, const double *mass, int64_t n,
                               int on_device, int use_sphere, const double *sphere,
                               const int64_t *fam, int nfam, uint32_t groups, int flags,
                               const double *frame, int64_t *n_kept, double *h_sums);
/* The same pass in a frame and a region (nclauses / kinds / negate / params
 * as in pbx_profile_set_region; nclauses == 0: exactly
 * pbx_property_moments_frame; frame[15..18] is read only when
 * PBX_FRAME_WRAP is set).  A particle is kept when the families, the
 * Sphere (if any) and every clause of the region hold, the clauses evaluated
 * on the frame's coordinates.  pos is read whenever a region is present.  The
 * region is a template parameter of the kernel beside the frame: the
 * region-less instantiations are the ones the two entry points above launch.
 * The summation order depends on the particle count alone. */
int pbx_property_moments_region(const double *pos, const double *vel, const double *mass,
                                int64_t n, int on_device, int use_sphere, const double *sphere,
                                const int64_t *fam, int nfam, uint32_t groups, int flags,
                                const double *frame, int nclauses, const int *kinds,
                                const int *negate, const double *params, int64_t *n_kept,
                                double *h_sums);
/* Shrinking-sphere centre of the particles in the family ranges (all when
 * nfam = 0) — the centre CenPos("ssc") asks pynbody for
 * (properties/generic.py:54-55).  The particles are staged once (or
 * borrowed, on_device = 1) and the pass above runs with groups MASS | COM
 * and a moving sphere, one read-back per iteration:
 *   com = sum(m*pos) / sum(m) over the particles;  r = r0
 *   repeat: keep = ((dx*dx + dy*dy) + dz*dz) < r*r about com;  c = count(keep)
 *           if c <= min_particles: stop (com unchanged)
 *           com = sum_keep(m*pos) / sum_keep(m);  r *= shrink_factor
 * h_cen[3] = com, *iterations = completed shrink steps, *n_last = the
 * particle count the returned centre was computed from.  PBX_ERR_VALUE: r0
 * <= 0 or NaN, shrink_factor outside (0, 1), min_particles < 1. */
int pbx_property_shrink_center(const double *pos, const double *mass, int64_t n, int on_device,
                               const int64_t *fam, int nfam, double r0, double shrink_factor,
                               int64_t min_particles, double *h_cen, int64_t *iterations,
                               int64_t *n_last);
/* Enclosed mass at many radii in one streaming pass: what the bisection of
 * a virial radius asks of the particles (pynbody analysis.halo.virial_radius:
 * M(<r) = dot(mass, r_arr < r)), and the extrema VirialRadius and SpinParam
 * start from (x.max() - x.min(), r.max()).  Stateless; pos / mass, on_device,
 * the sphere, the families, flags / frame and the region clauses as in
 * pbx_property_moments_region, with the same meaning: a particle is kept as
 * that pass keeps it, and x, y, z below are the frame's coordinates
 * (frame[15..18] is read only when PBX_FRAME_WRAP is set).  Per
 * kept particle, without FMA contraction, with a correctly rounded sqrt and
 * m = mass (1.0 when mass is NULL):
 *   r = sqrt((x*x + y*y) + z*z)
 *   h_msum[j]  = sum of m over the kept particles with r < h_t[j]   (strict)
 *   h_count[j] = the number of those particles
 * for j < nt, 0 <= nt <= PBX_ENCLOSED_MAX; a NaN r or a NaN h_t[j] enters no
 * sum.  nt == 0: only the extrema and *n_kept (h_t, h_msum and h_count may be
 * NULL).  h_ext[PBX_ENCLOSED_NEXT] (NULL: not wanted) = min x, max x, min y,
 * max y, min z, max z, max r over the kept particles; a NaN among them makes
 * that extremum NaN, as numpy's min / max do; nothing kept: all seven NaN,
 * the sums 0.0.  *n_kept = the number of kept particles.  The thresholds sit
 * in registers, so they cost arithmetic and no bandwidth: the pass reads 32
 * bytes per particle whatever nt is.  (The device compares r*r with the
 * smallest double whose correctly rounded sqrt reaches h_t[j], found on the
 * host: sqrt is monotonic, so every particle is decided as r < h_t[j]
 * decides it, and max r is the sqrt of max r*r.)
 * No atomics: the order of summation is fixed by the particle count alone,
 * and every threshold has an accumulator of its own.  Two contracts follow:
 *   1. the bits of h_msum[j] depend on the particles, the scope and h_t[j]
 *      only;
 *   2. they do not depend on nt, on the other thresholds, on the position
 *      of h_t[j] in the list, or on whether the extrema are wanted.
 * So a batch of thresholds stands for as many single evaluations.  The
 * order is moreover that of the PBX_PROP_MASS sum of the pass above: on
 * the same n particles with m replaced by 0.0 wherever the particle is not
 * kept or r < h_t[j] fails, that pass returns the bits of h_msum[j].
 * PBX_ERR_VALUE: nt outside [0, PBX_ENCLOSED_MAX], a needed array NULL,
 * pos NULL, n < 0, nfam > 16, a bad frame or region. */
#define PBX_ENCLOSED_MAX 31
#define PBX_ENCLOSED_NEXT 7
int pbx_property_enclosed(const double *pos, const double *mass, int64_t n, int on_device,
                          int use_sphere, const double *sphere, const int64_t *fam, int nfam,
                          int flags, const double *frame, int nclauses, const int *kinds,
                          const int *negate, const double *params, int nt, const double *h_t,
                          int64_t *n_kept, double *h_msum, int64_t *h_count, double *h_ext);
/* The virial radius of the kept particles: the radius at which the mean
 * enclosed density M(<r) / (4 pi r^3 / 3) equals target_rho, by the bisection
 * of pynbody's analysis.halo.virial_radius (util.bisect with epsilon = 0).
 * The scope arguments are those of the enclosed pass (frame[15..18] is read
 * only when PBX_FRAME_WRAP is set).  The particles are
 * staged once (or borrowed, on_device = 1) and the enclosed pass runs over
 * them, one read-back per pass.  Without has_rmax, r_max = max x - min x of
 * the kept particles, from one extrema pass (nt = 0).  The loop, in host
 * doubles, pow being libm's:
 *   left = 0.0; right = r_max
 *   for i in 0 .. niter_max - 1:
 *     if (right - left) < 0: return (right + left) / 2
 *     mid = (left + right) / 2
 *     z = target_rho - M(<mid) / (4 * pi * pow(mid, 3.0) / 3)
 *     if fabs(z) < eta: return mid
 *     else if z < 0: left = mid
 *     else: right = mid
 *   not converged
 * A pass evaluates the 2^L - 1 midpoints the next L iterations can reach,
 * each computed by the same (left + right) / 2 from the bounds its branch
 * would hold, so it is the value the loop would reach; the decisions are
 * then walked on the host (contracts 1 and 2 above: the result does not
 * depend on L).  levels = L, 1 <= L <= PBX_ENCLOSED_LEVELS; 0: the
 * library's choice (PBX_VIRIAL_LEVELS).  *h_radius = the loop's return value
 * (NaN when not converged); *iterations = the midpoints the loop evaluated
 * (niter_max when not converged); *passes = the enclosed passes, the
 * extrema pass included; *n_kept = the kept particles; *status =
 * PBX_VIRIAL_CONVERGED or PBX_VIRIAL_NOT_CONVERGED, the latter with PBX_OK:
 * it is a result, not an error.  Nothing kept and no r_max: r_max is NaN and
 * the loop cannot converge; that result is returned after the extrema pass.
 * PBX_ERR_VALUE: target_rho NaN or <= 0, eta NaN or < 0, niter_max < 1,
 * levels outside [0, PBX_ENCLOSED_LEVELS], and what the enclosed pass
 * rejects. */
#define PBX_ENCLOSED_LEVELS 5
#define PBX_VIRIAL_LEVELS 4
#define PBX_VIRIAL_CONVERGED 0
#define PBX_VIRIAL_NOT_CONVERGED 1
int pbx_property_virial_radius(const double *pos, const double *mass, int64_t n, int on_device,
                               int use_sphere, const double *sphere, const int64_t *fam, int nfam,
                               int flags, const double *frame, int nclauses, const int *kinds,
                               const int *negate, const double *params, double target_rho,
                               double eta, int niter_max, int has_rmax, double r_max, int levels,
                               double *h_radius, int64_t *iterations, int64_t *passes,
                               int64_t *n_kept, int *status);

/* The extents WrapBox("minirange") chooses its convention from
 * (transforms/wrap.py:161-211 of the reference: both candidate wraps of every
 * axis, their max() - min(), the smaller range wins): one streaming pass over
 * pos[0:n] (n x 3 doubles, host or device), every particle, no predicate.
 * flags / frame as in pbx_profile_set_frame, restricted to what can precede a
 * wrap: PBX_FRAME_POS (the shift is applied first) and PBX_FRAME_VEL (ignored:
 * velocities are not read); PBX_FRAME_ROT or PBX_FRAME_WRAP is a
 * PBX_ERR_VALUE, and so is L not finite or L <= 0.  Per axis a, with the wrap
 * step of the frame for lo = -0.5*L (wc) and lo = 0.0 (wu):
 *   h_ext[4*a + 0] = min wc,  h_ext[4*a + 1] = max wc,
 *   h_ext[4*a + 2] = min wu,  h_ext[4*a + 3] = max wu
 * with numpy's rule for min / max: a NaN among an axis's values makes its
 * four numbers NaN (and the other axes' none).  The values are numpy's bit
 * for bit, except the sign of an extremum that is a zero when both zeros
 * occur (numpy's own choice there depends on its reduction order); a range
 * max - min does not depend on it.  n == 0: the identities, +inf for a min
 * and -inf for a max, PBX_OK.  No atomics; a min / max does not depend on the
 * order of the fold.  The axis choice is the caller's. */
int pbx_property_wrap_extents(const double *pos, int64_t n, int on_device, int flags,
                              const double *frame, double L, double *h_ext);

/* ------------------------------------------------------------------ */
/* multi-GPU: RCCL communicator (one process per GPU, over xGMI)       */
/* ------------------------------------------------------------------ */
/* No reference counterpart: the reference is single-process (rayon
 * threads).  North-star multi-GPU design: targets are
 * sharded across ranks, source records are all-gathered, profile partials
 * are all-reduced.  The unique id (pbx_comm_unique_id_size() bytes) is
 * created on rank 0 and distributed by the caller's control plane. */
int pbx_comm_unique_id_size(void);
int pbx_comm_unique_id(unsigned char *buf, int buflen);
int pbx_comm_init(void **comm, int nranks, int rank, const unsigned char *uid);
int pbx_comm_destroy(void *comm);
/* In-place all-gather-v of byte segments: segment r is
 * [displs[r], displs[r]+counts[r]) of d_buf, this rank's already in place. */
int pbx_comm_allgatherv(void *comm, void *d_buf, const int64_t *counts,
                        const int64_t *displs);
int pbx_comm_allreduce_f64(void *comm, const double *d_send, double *d_recv,
                           int64_t count);
/* generic: dtype 0 f64, 1 i64, 2 u64, 3 u32; op 0 sum, 1 min, 2 max */
int pbx_comm_allreduce(void *comm, const void *d_send, void *d_recv, int64_t count, int dtype,
                       int op);
int pbx_comm_allreduce_i64(void *comm, const int64_t *d_send, int64_t *d_recv,
                           int64_t count);
/* all-reduce of a small HOST array in place (dtype / op as above) through
 * the communicator's persistent device + pinned staging: no allocation per
 * call, one stream sync (the profile partials of ShardedProfile) */
int pbx_comm_allreduce_host(void *comm, void *h_buf, int64_t count, int dtype, int op);
/* Control plane on the same communicator: device barrier (returns after
 * every rank reached it and the stream drained) and max over ranks of a
 * host double. */
int pbx_comm_barrier(void *comm);
int pbx_comm_max_f64(void *comm, double value, double *out);

/* A communicator whose collectives go through a caller-supplied HOST
 * transport instead of RCCL (no reference counterpart).  Every collective
 * of the library — the pbx_comm_* calls above and the all-reduces inside
 * pbx_profile_radial_equaln_comm — stages its device bytes through pinned
 * host memory (D2H, stream sync), calls `fn`, and copies the result back.
 * fn(ctx, kind, h_buf, count, dtype, op, counts, displs) returns 0 on
 * success:
 *   kind PBX_COLL_ALLREDUCE: reduce `count` elements of `dtype` (codes as
 *     pbx_comm_allreduce) with `op` over the ranks, in place in h_buf;
 *   kind PBX_COLL_ALLGATHERV: h_buf holds the whole byte buffer with this
 *     rank's segment [displs[rank], +counts[rank]) in place; fill in the
 *     others (count = nranks).
 * While fn runs, a library call that issued the collective has released
 * the device lock, so the ranks of one process may be threads sharing one
 * device (the one-GPU multi-rank tests) — or processes on a host transport
 * (MPI, shared memory) where RCCL is unavailable. */
#define PBX_COLL_ALLREDUCE 0
#define PBX_COLL_ALLGATHERV 1
typedef int (*pbx_host_collective_fn)(void *ctx, int kind, void *h_buf, int64_t count, int dtype,
                                      int op, const int64_t *counts, const int64_t *displs);
int pbx_comm_init_host(void **comm, int nranks, int rank, pbx_host_collective_fn fn, void *ctx);

/* ------------------------------------------------------------------ */
/* cumulative table of a profile handle: RadiusAtSurfaceDensity        */
/* ------------------------------------------------------------------ */
/* Replaces RadiusAtSurfaceDensity.calculate (properties/base.py:172-284):
 * the radii sorted, the cumulative mass in that order, the surface density
 * read off the two (_sigma_at_radius), a scan of 256 radii for the first
 * sign change of sigma - target and 80 bisection steps.
 *
 * pbx_profile_cum_build runs after a selection or after pbx_profile_set_x:
 * the stable value sort of the handle's whole x (the one
 * pbx_profile_contain launches; ties keep index order), then one block
 * writes two arrays of n doubles kept on the handle,
 *     xs[k] = x[e[k]],  cum[k] = np.cumsum(w[e])[k]
 * with e the sorted element ids and the sum running sequentially on one
 * lane (np.cumsum's rounding, bit for bit; linear in n, see
 * pbx_profile_contain), from one element on.  w_src = 1 (the selection
 * weights) or 2 (the host array h_w, n doubles in selection order).
 * *r_min = xs[0], *r_max = xs[n-1], *total = cum[n-1].  n == 0 is a
 * PBX_ERR_VALUE.  Whatever replaces the handle's x drops the table: a new
 * selection (pbx_profile_select*, pbx_profile_radial_equaln*),
 * pbx_profile_set_x, pbx_profile_set_frame, pbx_profile_set_region.
 *
 * pbx_profile_cum_get reads the table back (n doubles each).
 *
 * pbx_profile_cum_sigma: h_sigma[k] = _sigma_at_radius of h_r[k], 1 <= nr
 * <= 4096, one thread per radius; mode 1 = "total" (M(<=r) / (pi r^2)),
 * mode 0 = the shell [max(r - eps/2, 0), r + eps/2].  Every statement of
 * the reference in its order, without FMA contraction: the r <= 0, hi <= 0,
 * hi <= lo and area <= 0 guards, searchsorted right for the outer radius
 * and left for the inner one, cum[hi-1] - (lo > 0 ? cum[lo-1] : 0.0),
 * pi * (rout^2 - rin^2) with both squares rounded first.  A square is the
 * rounded product r*r (the reference's r**2 on scalars is libm pow, which
 * differs from the product by one ulp for about 0.085 % of doubles).
 *
 * pbx_profile_cum_solve: ONE launch of one 256-thread block and ONE
 * read-back.  The threads evaluate sigma on the uploaded grid (2 <= ngrid <=
 * 4096 radii) into LDS; the block finds the first k with
 * signbit(sigma[k] - target) != signbit(sigma[k+1] - target); one lane then
 * runs the reference's loop from left = grid[k], right = grid[k+1]: up to 80
 * times mid = 0.5*(left + right), stop with left = right = mid when
 * |sigma(mid) - target| < 1e-10, else right = mid when
 * (sigma(left) - target) * (sigma(mid) - target) <= 0 and left = mid
 * otherwise.  *radius = 0.5*(left + right).  info[4] = {status (0 solved, 1
 * no sign change: *radius is NaN), k, iterations run (the one that stopped
 * early included), 1 if it stopped early}.
 *
 * PBX_ERR_VALUE: a NULL argument, nr / ngrid out of range, a mode other
 * than 0 or 1, and cum_get / cum_sigma / cum_solve without a valid table. */
int pbx_profile_cum_build(void *handle, int w_src, const double *h_w, double *r_min,
                          double *r_max, double *total);
int pbx_profile_cum_get(void *handle, double *h_xs, double *h_cum);
int pbx_profile_cum_sigma(void *handle, int mode, double eps, int nr, const double *h_r,
                          double *h_sigma);
int pbx_profile_cum_solve(void *handle, int mode, double eps, double target, int ngrid,
                          const double *h_grid, double *radius, int64_t *info);

#ifdef __cplusplus
}
#endif
#endif /* PBX_H */
